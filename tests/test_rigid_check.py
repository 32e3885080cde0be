"""CPU tests of the rigid-body pose ABI's arithmetic (csrc/pt_rigid_math.hpp,
the functions the kernel of csrc/pt_rigid.hip calls), run by the stand-alone
csrc/rigid_check.cpp against the Python definition (ptmi/rigid.py): the row
floats and the leaf boxes equal ``scene_compiler.update_records`` of the posed
objects and update_helpers' box rules bit for bit, also under the sanitizers; a
body that neither turns nor moves leaves every row float ``==`` the rest row;
the rotated rest vectors agree with the constructors on the posed points to an
f32 ulp; and the leaf box at any time lies within ``rigid.swept_box``, which is
what DeviceScene.set_tracks' shell hint relies on for a body that turns."""
import os
import subprocess

import numpy as np
import pytest

import rigid_helpers as rh
from ptmi import core, rigid, scene_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
MODE = {'spheres': 'sphere', 'quads': 'quad', 'triangles': 'tri'}
N_PRIMS = 200


@pytest.fixture(scope='module')
def data():
    """Per kind 200 random primitives, magnitudes 1e-3 .. 1e4, in 16 bodies, made once."""
    out = {}
    for seed, kind in enumerate(rh.KINDS):
        objs = rh.random_prims(kind, N_PRIMS, seed)
        out[kind] = (objs, rh.random_bodies(kind, objs, 50 + seed))
    return out


def run(exe, kind, objs, bodies, t, tmp_path):
    src, dst = str(tmp_path / f'{kind}.in'), str(tmp_path / f'{kind}.out')
    rh.check_input(kind, objs, bodies, t).astype('<f8').tofile(src)
    subprocess.run([exe, MODE[kind], src, dst], check=True, timeout=60)
    return np.fromfile(dst, f32)


def check_all(exe, data, tmp_path):
    for kind in rh.KINDS:
        objs, bodies = data[kind]
        for t in rh.TIMES:
            got = run(exe, kind, objs, bodies, t, tmp_path)
            want = rh.expected(kind, objs, bodies, t)
            assert got.tobytes() == want.tobytes(), (kind, t)
    # bad arguments: an unknown mode, records that are not whole, a missing file
    src = str(tmp_path / 'spheres.in')
    assert subprocess.run([exe, 'box', src, src + '.x'], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'quad', src, src + '.x'], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'sphere', src + '.none', src + '.x'], capture_output=True).returncode == 2


def test_inputs_cover_the_magnitudes_the_pivots_the_angles_and_the_axes(data):
    for kind in rh.KINDS:
        objs, bodies = data[kind]
        assert len(bodies) == rigid.MAX_BODIES and sorted(rigid.members_of(bodies)[kind]) == list(range(N_PRIMS))
        rec = rigid.body_records(bodies, rh.prim_lists(kind, objs))[rh.STORAGE_POS[kind]][2]
        assert rec.shape == (N_PRIMS, rigid.REC_DOUBLES[kind])
        mag = np.abs(rec[:, :3])
        assert mag.min() < 1e-2 and mag.max() > 1e3
        assert sorted({b.turn for b in bodies}) == sorted(set(rh.ANGLES) | {-2.5})
        far = [i % 2 == 1 for i in range(len(bodies))]  # random_bodies' order: near, far, near, ...
        assert all(min(abs(x) for x in b.pivot.to_list()) >= 5e3 for b, f in zip(bodies, far) if f)
        on_axis = [sorted(abs(x) for x in b.axis.to_list()) == [0.0, 0.0, 1.0] for b in bodies]
        # every angle with a near and a far pivot; coordinate axes and others among both
        assert sum(far) == 8 and {(f, o) for f, o in zip(far, on_axis)} == {(a, b) for a in (False, True)
                                                                            for b in (False, True)}
        for b in bodies:
            a = b.axis
            assert abs((a.x * a.x + a.y * a.y + a.z * a.z) - 1.0) < 4e-16
        # a pose changes the rows, and t = 1 turns every body by its own angle
        at1 = rigid.body_at(bodies[6], 1.0)
        assert at1[:9] == rigid.rotation_matrix(bodies[6].axis, rh.ANGLES[3])
        rest = rh.expected(kind, objs, [rigid.Body(core.vec3(0, 0, 0), core.vec3(0, 0, 1), 0.0,
                                                   **{kind: range(N_PRIMS)})], 0.5)
        assert rh.expected(kind, objs, bodies, 0.5).tobytes() != rest.tobytes()


def test_check_program_equals_the_python_definition(data, tmp_path):
    exe = str(tmp_path / 'rigid_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'rigid_check', f'RIGID_CHECK={exe}'], check=True)
    check_all(exe, data, tmp_path)


def test_check_program_under_sanitizers(data, tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same inputs."""
    exe = str(tmp_path / 'rigid_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'rigid_check', f'RIGID_CHECK={exe}',
                    'RIGID_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    check_all(exe, data, tmp_path)


def _rest_rows(kind, objs):
    return scene_compiler.update_records(**{kind: objs})[rh.STORAGE_POS[kind]][0]


def test_a_body_that_neither_turns_nor_moves_leaves_every_row_float_equal(data):
    """ω = 0, d = 0: R is exactly the identity and a vector's row float is the rest row's; a point is (p - c) + c,
    which is p for the pivot at the origin (p - 0 is exact). Checked at several times, as numbers (==)."""
    for kind in rh.KINDS:
        objs, _ = data[kind]
        still = [rigid.Body(core.vec3(0, 0, 0), core.vec3(1, 2, -3), 0.0, **{kind: range(0, N_PRIMS, 2)}),
                 rigid.Body(core.vec3(0, 0, 0), core.vec3(0, -1, 0), 0.0, core.vec3(0, 0, 0),
                            **{kind: range(1, N_PRIMS, 2)})]
        rest = _rest_rows(kind, objs)
        for t in (0.0, 0.5, 1.0 / 3.0, 7.25):
            assert rigid.body_at(still[0], t)[:9] == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
            rows = rigid.posed_records(still, rh.prim_lists(kind, objs), t)[rh.STORAGE_POS[kind]][1]
            assert np.array_equal(rows, rest), (kind, t)
        # a pivot elsewhere: the vectors still compare ==, whatever the pivot
        moved = [rigid.Body(core.vec3(3.5, -1e4, 0.125), core.vec3(1, 2, -3), 0.0, **{kind: range(N_PRIMS)})]
        rows = rigid.posed_records(moved, rh.prim_lists(kind, objs), 0.5)[rh.STORAGE_POS[kind]][1]
        vectors = {'spheres': [3], 'quads': [0, 1, 2] + list(range(7, 16)), 'triangles': list(range(3, 12))}[kind]
        assert np.array_equal(rows[:, vectors], rest[:, vectors]), kind


def test_the_identity_turns_a_negative_zero_into_a_positive_one(tmp_path):
    """Q.x = -0.0 under the identity body: (Q.x - 0.0) is -0.0, the row sum adds +0.0 products to it, and the row
    float is +0.0: equal as a number, another bit pattern. No other float of the row changes but in a zero's sign.
    This is why the rest state comes back by unpose(), not by a pose with the identity."""
    exe = str(tmp_path / 'rigid_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'rigid_check', f'RIGID_CHECK={exe}'], check=True)
    q = core.quad(core.vec3(-0.0, 1.0, 2.0), core.vec3(0, 0, 3.0), core.vec3(0, 2.0, 0), rh.MAT)
    body = [rigid.Body(core.vec3(0, 0, 0), core.vec3(0, 1, 0), 0.0, quads=[0])]
    rest = _rest_rows('quads', [q])
    got = run(exe, 'quads', [q], body, 0.0, tmp_path)
    assert got.tobytes() == rh.expected('quads', [q], body, 0.0).tobytes()
    row = got[:16].reshape(1, 16)
    assert np.array_equal(row, rest)  # equal as numbers
    diff = row.view(np.uint32) ^ rest.view(np.uint32)
    assert diff[0, 4] == 0x80000000 and rest[0, 4] == 0.0 and np.signbit(rest[0, 4]) and not np.signbit(row[0, 4])
    assert set(np.unique(diff).tolist()) <= {0, 0x80000000} and not np.any(rest[0, np.flatnonzero(diff[0])])


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, f32)))


def test_rotated_rest_vectors_agree_with_the_constructors_to_an_f32_ulp(data):
    """``quad(Q', R u, R v)`` and ``triangle(v0', v1', v2')`` built by the constructors from the posed float64
    values against ``transformed``. The points are the same float64 values on both sides: their row floats are
    equal. Every stored float of a vector is within one f32 ulp of the other side's, per component
    (``np.spacing`` of the larger of the two magnitudes): the float64 values differ by a few 2^-53 relative, times
    the conditioning of the cross product or of the edge difference, against an f32 ulp of 2^-23, so the cast can
    only flip a boundary case. D within 2^-22 (|n.x Q.x| + |n.y Q.y| + |n.z Q.z|)."""
    differing = total = 0
    for kind, spans in (('quads', [(0, 3), (7, 10), (10, 13), (13, 16)]), ('triangles', [(3, 6), (6, 9), (9, 12)])):
        objs, bodies = data[kind]
        members = rigid.members_of(bodies)[kind]
        for t in (1.0, 1.0 / 3.0):
            at = [rigid.body_at(b, t) for b in bodies]
            posed = [rigid.posed_object(kind, objs[i], at[members[i]]) for i in range(N_PRIMS)]
            if kind == 'quads':
                built = [core.quad(p.Q, p.u, p.v, p.mat) for p in posed]
            else:
                built = [core.triangle(p.v0, p.v1, p.v2, p.mat) for p in posed]
            a, b = _rest_rows(kind, posed), _rest_rows(kind, built)
            points = slice(4, 7) if kind == 'quads' else slice(0, 3)
            assert a[:, points].tobytes() == b[:, points].tobytes()
            for lo, hi in spans:
                va, vb = a[:, lo:hi].astype(np.float64), b[:, lo:hi].astype(np.float64)
                tol = _ulp(np.maximum(np.abs(va), np.abs(vb))).astype(np.float64)  # per component
                assert np.all(np.abs(va - vb) <= tol), (kind, t, lo)
                differing += int(np.count_nonzero(va != vb))
                total += va.size
            if kind == 'quads':
                bound = np.array([2.0 ** -22 * (abs(p.normal.x * p.Q.x) + abs(p.normal.y * p.Q.y)
                                                + abs(p.normal.z * p.Q.z)) for p in posed])
                assert np.all(np.abs(a[:, 3].astype(np.float64) - b[:, 3].astype(np.float64)) <= bound), t
                differing += int(np.count_nonzero(a[:, 3] != b[:, 3]))
                total += N_PRIMS
    print(f'floats that differ from the constructors\' after the cast: {differing} of {total}')


def test_the_leaf_box_at_any_time_lies_within_the_swept_box():
    """500 random bodies that turn, one primitive each, 20 random times in the body's range each: the f32 leaf box
    of ``posed_records`` lies inside ``rigid.swept_box`` of the f32 rest leaf box. No case is skipped."""
    rng = np.random.default_rng(23)
    checked = 0
    for b in range(500):
        kind = rh.KINDS[b % 3]
        obj = rh.random_prims(kind, 1, 1000 + b)[0]
        near = rh._origin(kind, obj) + rh.psh._vec(rng, -3.0, 1.0)
        pivot = near if b % 4 else core.vec3(*(rng.uniform(-1, 1, 3) * 1e4))
        body = rigid.Body(pivot, rh.psh._vec(rng, -1.0, 1.0), float(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 2)),
                          rh.psh._vec(rng, -3.0, 2.0), **{kind: [0]})
        assert body.turn != 0.0
        t0 = float(rng.uniform(-2.0, 2.0))
        t1 = t0 + float(rng.uniform(0.0, 2.0))
        prims = rh.prim_lists(kind, [obj])
        pos = rh.STORAGE_POS[kind]
        rest_mn, rest_mx = rh.psh.BOX_RULE[kind](scene_compiler.update_records(**{kind: [obj]})[pos][1])
        lo, hi = rigid.swept_box(rest_mn[0], rest_mx[0], body, t0, t1)
        for t in [t0, t1] + rng.uniform(t0, t1, 18).tolist():
            mn, mx = rh.psh.BOX_RULE[kind](rigid.posed_records([body], prims, t)[pos][2])
            assert np.all(mn[0].astype(np.float64) >= lo) and np.all(mx[0].astype(np.float64) <= hi), (b, kind, t)
            checked += 1
    assert checked == 500 * 20
