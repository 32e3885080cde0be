"""The oracle against the reference's own kernel text, path by path.

tests/golden/kernel_paths_<scene>.npz hold, for tiny frames, what the
reference's kernels.py computed for every path when executed over the Taichi
stand-in tests/golden/ti_shim.py (gen_kernel_paths.py): colour, counters,
number of random draws and one record per segment. oracle.trace_path_log must
reproduce all of it bit for bit, for both integrators. Nothing here reads the
reference, and ti_shim.py is not imported: its tables are read as literals.
"""
import ast
import os

import numpy as np
import pytest

import oracle

from kernel_path_fixtures import FIXTURES, GOLDEN, SCENES, VARIANTS, frame_args, load

# coverage case -> minimum number of paths, in at least one fixture, per variant
# (20 / 20 / 10 as the cases were specified; 5 elsewhere, the controls' bound)
COVERAGE_MIN = dict(
    {f'mat{m}_on_{p}': 5 for m in range(5) for p in ('sphere', 'triangle', 'quad')},
    metal_fuzz_absorb=20, dielectric_tir_draw=20, front_face_true=5, front_face_false=5,
    tex_solid=5, tex_checker_even=5, tex_checker_odd=5, tex_noise_scale_a=5, tex_noise_scale_b=5,
    tex_image_sphere=5, tex_image_not_sphere=5,
    medium_scatter_sphere=10, medium_scatter_box=10, medium_scatter_fog=10, medium_passthrough=10,
    medium_fallback=10, medium_scatter_then_hit_inside=10,
    rr_kill=5, rr_survive=5, depth_cap=5, defocus_on=5, defocus_off=5,
    stack_overflow_drop=5, coincident_tie=5, stackless=5, sah_tree=5,
)
WF_ONLY = dict(wf_unnormalised_dir=5, wf_passthrough_wave=10, wf_rr_kill=5)


def test_every_scene_has_its_fixture():
    assert tuple(FIXTURES) == SCENES


_oracle_colors = {}


def oracle_paths(name, variant):
    """Replays every path of a fixture through oracle.trace_path_log and
    compares as it goes; returns the oracle's colours (P, 3)."""
    if (name, variant) in _oracle_colors:
        return _oracle_colors[(name, variant)]
    z, sa, cam = load(name)
    osc = oracle.OracleScene(sa)
    fr = oracle.make_frame(*frame_args(z, cam))
    Wd, Ht, spp = cam['width'], cam['height'], int(z['spp'])
    g = {k: z[f'{variant}_{k}'] for k in ('color', 'nseg', 'medium', 'rr', 'cap', 'draws', 'seg_off', 'seg_rng_n',
                                          'seg_hit', 'seg_t', 'seg_type', 'seg_idx', 'seg_kind')}
    colors = np.zeros_like(g['color'])
    for s in range(spp):
        for py in range(Ht):
            for px in range(Wd):
                q = (s * Ht + py) * Wd + px
                where = f'{name} {variant} pixel ({px}, {py}) sample {s}'
                col, st, segs, draws = oracle.trace_path_log(osc, fr, variant, px, py, s)
                colors[q] = col
                a, b = int(g['seg_off'][q]), int(g['seg_off'][q + 1])
                rec = {'rng_n': g['seg_rng_n'][a:b], 'hit': g['seg_hit'][a:b], 't': g['seg_t'][a:b],
                       'prim_type': g['seg_type'][a:b], 'prim_idx': g['seg_idx'][a:b], 'kind': g['seg_kind'][a:b]}
                for k in range(min(len(segs), b - a)):
                    for fld in ('rng_n', 'hit', 't', 'prim_type', 'prim_idx', 'kind'):
                        x, y = segs[fld][k], rec[fld][k]
                        same = x.tobytes() == np.asarray(y, x.dtype).tobytes()
                        assert same, f'{where}: segment {k} field {fld}: oracle {x!r}, reference text {y!r}'
                assert len(segs) == b - a, f'{where}: {len(segs)} segments, reference text {b - a}'
                assert st['segments'] == g['nseg'][q], f'{where}: segment counter'
                assert st['medium'] == g['medium'][q], f'{where}: medium exits {st["medium"]} vs {g["medium"][q]}'
                assert st['rr'] == g['rr'][q], f'{where}: RR flag {st["rr"]} vs {g["rr"][q]}'
                assert st['depth_cap'] == g['cap'][q], f'{where}: depth-cap flag {st["depth_cap"]} vs {g["cap"][q]}'
                assert draws == g['draws'][q], f'{where}: {draws} draws, reference text {g["draws"][q]}'
                assert col.tobytes() == g['color'][q].tobytes(), \
                    f'{where}: colour {col!r} vs {g["color"][q]!r} (all {len(segs)} segment records equal)'
    _oracle_colors[(name, variant)] = colors
    return colors


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('name', SCENES)
def test_oracle_equals_reference_text(name, variant):
    oracle_paths(name, variant)


@pytest.mark.parametrize('variant', VARIANTS)
def test_coverage_minimums(variant):
    table = dict(COVERAGE_MIN, **(WF_ONLY if variant == 'wf' else {}))
    for case, least in table.items():
        best = max(int(load(n)[0][f'{variant}_coverage_{case}']) for n in SCENES)
        assert best >= least, f'{variant}: {case} is reached on {best} paths at most, {least} needed'


def _shim_tables():
    with open(os.path.join(GOLDEN, 'ti_shim.py')) as f:
        tree = ast.parse(f.read())
    out = {}
    for node in tree.body:
        if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name)
                and node.targets[0].id in ('SEMANTICS', 'SWITCHES')):
            out[node.targets[0].id] = ast.literal_eval(node.value)
    return out['SEMANTICS'], out['SWITCHES']


def _stored(prefix):
    found = {}
    for n in SCENES:
        z = load(n)[0]
        for key in z.files:
            v, _, rest = key.partition('_')
            if v in VARIANTS and rest.startswith(prefix):
                found.setdefault(rest[len(prefix):], []).append((n, v))
    return found


def test_shim_table_switches_and_controls_agree():
    semantics, switches = _shim_tables()
    rows = [r[0] for r in semantics]
    assert len(rows) == len(set(rows)) and all(len(r) == 3 and r[1] for r in semantics)
    for name, sw in switches.items():
        assert sw['row'] in rows, f'switch {name} flips a row the table does not have'
    controls, invariants = _stored('control_'), _stored('invariant_')
    assert set(controls) == {k for k, sw in switches.items() if sw['control']}
    assert set(invariants) == {k for k, sw in switches.items() if not sw['control']}
    for where in list(controls.values()) + list(invariants.values()):
        assert {v for _, v in where} == set(VARIANTS)


@pytest.mark.parametrize('variant', VARIANTS)
def test_controls_differ_from_the_oracle(variant):
    """A quirk restated the other way in the oracle would make it agree with
    that control's colours: each control differs from the oracle on >= 5 paths.
    The one switch that cannot change an image (ti_shim.SWITCHES: c_mod) equals it."""
    for kind, store in (('control_', _stored('control_')), ('invariant_', _stored('invariant_'))):
        for sw, where in store.items():
            for name, v in where:
                if v != variant:
                    continue
                col = oracle_paths(name, variant)
                ctl = load(name)[0][f'{variant}_{kind}{sw}']
                differ = int(np.sum(np.any(col.view(np.uint32) != ctl.view(np.uint32), axis=1)))
                if kind == 'control_':
                    assert differ >= 5, f'{name} {variant}: control {sw} differs from the oracle on {differ} paths'
                else:
                    assert differ == 0, f'{name} {variant}: {sw} differs from the oracle on {differ} paths'
