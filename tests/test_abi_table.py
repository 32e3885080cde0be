"""CPU test: the library answers every recorded rejected or no-op call
(tests/golden/abi_errors.json, recorded from the revision before the entry
points shared their argument checks; tests/golden/gen_abi_errors.py) with the
same return value and the same ptmi_last_error() text. No case reaches a HIP
call, so no GPU is needed."""
import collections

import abi_table
from ptmi import _lib


def test_table_covers_every_checking_entry_point():
    cases = abi_table.load_table()
    by_fn = collections.Counter(c['fn'] for c in cases)
    # every export but the three without arguments and the host-side BVH builder
    assert set(by_fn) == set(_lib.EXPORTS) - {'ptmi_version', 'ptmi_node_bytes', 'ptmi_last_error',
                                              'ptmi_bvh_build_sah'}
    noops = [c for c in cases if c['ret'] == 0 and c['err'] == abi_table.SENTINEL]
    silent = {c['fn'] for c in noops}
    assert {'ptmi_mk_render', 'ptmi_mk_render_ws', 'ptmi_mk_trace_ws', 'ptmi_mk_resolve_ws', 'ptmi_wf_render',
            'ptmi_clear', 'ptmi_stats_clear', 'ptmi_mk_trace_tiles_ws', 'ptmi_mk_resolve_stats_ws',
            'ptmi_wf_render_stats'} <= silent
    assert len(cases) > 600 and len({(c['fn'], c['ret'], c['err']) for c in cases}) > 400


def test_library_reproduces_the_recorded_answers():
    lib = _lib.load()
    wrong = []
    for c in abi_table.load_table():
        got = abi_table.call(lib, c['fn'], c['args'])
        if got != (c['ret'], c['err']):
            wrong.append((c['fn'], c['args'], got, (c['ret'], c['err'])))
    assert not wrong, f'{len(wrong)} cases differ, first: {wrong[0]}'
