"""CPU test: the library derives the same tile grid, batch limit and workspace
sizes, and refuses the same batches with the same words, as the revision
tests/golden/plan_sizes.json was recorded from (the last one before the launch
plans moved into pt_mk_plan.hpp and pt_wf_plan.hpp;
tests/golden/gen_plan_sizes.py). No call reaches the HIP runtime."""
import plan_table
from ptmi import _lib


def test_table_covers_the_frames_and_limits():
    cases = plan_table.load_table()
    assert len(cases) == 11
    assert {tuple(c['grid'][:2]) for c in cases} == {(8, 8), (16, 4), (32, 2), (64, 1)}
    for c in cases:
        batches = [b['batch'] for b in c['batches']]
        assert {1, 2, 3, 4, 5, 16, 64, 1024, 0, -1, c['max_batch'], c['max_batch'] + 1} == set(batches)
        assert [t[0] for t in c['trace']] == [_lib.PTMI_ECAPACITY, _lib.PTMI_EINVAL]
    # the issue's own sample: 800 x 800, band (4, 8, 3)
    band = next(c for c in cases if c['frame'].get('band_stride') == 8 and c['frame']['band_rows'] == 4)
    assert band['grid'] == [16, 4, 50, 25] and band['max_batch'] == 53430
    assert next(b for b in band['batches'] if b['batch'] == 64)['wf'][0] == 2989347840


def test_library_reproduces_the_recorded_plans():
    lib = _lib.load()
    for c in plan_table.load_table():
        n = len(c['batches']) - 2  # answer() appends max_batch and max_batch + 1 itself
        got = plan_table.answer(lib, c['frame'], [b['batch'] for b in c['batches'][:n]])
        assert got == c, (c['frame'], got)
