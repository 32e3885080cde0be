"""CPU tests of the enclosing medium shell (include/ptmi.h, `shell`): which
scenes scene_data.find_shell takes, how pack_device encodes the hint, what the
library rejects, and the megakernel's inline decision (shell_hit,
pt_device.hpp: the shell leaf's own box, then its sphere) restated in numpy
f32 against the oracle's full traversal, for the medium's exit search and for
the segment after a passthrough."""
import ctypes as C
import math

import numpy as np
import pytest

import shell_scenes as ss
from parity_helpers import fixture
from ptmi import _lib, scene_data as sd
from ptmi.core import Sphere, color, constant_medium, lambertian, point3
from ptmi.scenes import box

f32 = np.float32


def decode(layout):
    """(sphere row, leaf code) of the leaf the layout's hint points at."""
    v = layout.shell - 1
    off, child = v & ~1, v & 1
    assert off % sd.NODE_BYTES == 0 and off // sd.NODE_BYTES < layout.n_inner
    ref = int(layout.nodes[off // sd.NODE_BYTES, 12 + child].view(np.int32))
    assert ref < 0 and (ref >> 28) & 3 == sd.PRIM_SPHERE and (ref >> 25) & 7 == sd.CLASS_MEDIUM
    return ref & 0x01ffffff, ref


@pytest.mark.parametrize('name', ['vol2_final_scene', 'vol2_final_scene_comparison'])
def test_vol2_fog_is_the_shell(name):
    layout = sd.pack_device(fixture(name))
    assert layout.shell > 0
    row, _ = decode(layout)
    assert layout.spheres[row].tolist() == [0.0, 0.0, 0.0, 5000.0]
    v = layout.shell - 1
    assert layout.nodes[(v & ~1) // sd.NODE_BYTES, (v & 1):12:2].tolist() == [-5000.0] * 3 + [5000.0] * 3


@pytest.mark.parametrize('name', ['cornell_smoke', 'cornell_mesh_fog', 'wavefront_comparison'])
def test_scenes_without_a_shell(name):
    assert sd.pack_device(fixture(name, 96)).shell == 0


def _probe(R, frac):
    """A small sphere on the x axis whose box's farthest corner is frac * R from the origin."""
    r = R / 100.0
    x = math.sqrt((frac * R) ** 2 - 2 * r * r) - r
    return Sphere.stationary(point3(x, 0, 0), r, lambertian.from_color(color(0.5, 0.5, 0.5)))


def test_synthetic_shells():
    R = 100.0
    assert sd.pack_device(ss.shell_arrays(R)).shell > 0
    near = sd.pack_device(ss.shell_arrays(R, extra=[_probe(R, 0.49)]))
    assert near.shell > 0 and near.spheres[decode(near)[0], 3] == R
    # the farthest other leaf at 0.51 R
    assert sd.pack_device(ss.shell_arrays(R, extra=[_probe(R, 0.51)])).shell == 0
    # a second copy of the shell sphere, as a surface
    twin = Sphere.stationary(point3(0, 0, 0), R, lambertian.from_color(color(0.5, 0.5, 0.5)))
    assert sd.pack_device(ss.shell_arrays(R, extra=[twin])).shell == 0
    # a medium that is a box of quads
    fog = constant_medium.from_color(box(point3(-R, -R, -R), point3(R, R, R), lambertian.from_color(color(1, 1, 1))),
                                     color(1, 1, 1), 0.005)
    assert sd.pack_device(ss.shell_arrays(R, shell=False, extra=[fog])).shell == 0
    # the shell as the only primitive: its leaf is the root
    sa = ss.shell_arrays(R)
    only = sd.compile_world(ss._wrap([o for o in ss.shell_world(R).objects if isinstance(o, constant_medium)]))
    assert only.num_spheres == 1 and only.num_bvh_nodes == 1 and sd.pack_device(only).shell == 0
    # leaf depth past 62: the reference's own stack walk runs, no hint
    assert sd.find_shell(sa, 62) > 0 and sd.find_shell(sa, 63) == -1


def test_malformed_shell_values_are_rejected():
    lib = _lib.load()
    v = _lib.SceneView()
    v.num_spheres, v.n_inner, v.max_leaf_depth, v.num_bvh_nodes = 3, 2, 2, 5
    v.nodes = v.spheres = v.mats = v.perlin_vec = v.perlin_perm = 16
    nb = lib.ptmi_node_bytes()
    for ok in (0, 1, 2, 1 + nb, 2 + nb):
        v.shell = ok
        assert lib.ptmi_scene_check(C.byref(v)) == _lib.PTMI_OK, ok
    for bad in (-1, -nb, 3, 17, nb, 1 + 2 * nb, 2 + 2 * nb, 1 + 16 * nb, 0x7fffffff):
        v.shell = bad
        assert lib.ptmi_scene_check(C.byref(v)) == _lib.PTMI_EINVAL, bad
        assert 'shell' in lib.ptmi_last_error().decode()


# ------------------------------------------------- the inline decision, numpy f32
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def inv_dir(d):  # kernels.py:642-646 (Q15)
    return np.array([f32(1) / x if abs(x) > f32(1e-8) else f32(1e8) for x in d], f32)


def shell_hit(lo, hi, sph, o, d, inv, tmin):
    """pt_device.hpp shell_hit: the leaf box's slab test with closest = 1e10
    (min(X, 1e10) >= E), then hit_sphere_t in [tmin, 1e10). (hit, t)."""
    t0, t1 = (lo - o) * inv, (hi - o) * inv
    mn, mx = np.fmin(t0, t1), np.fmax(t0, t1)
    E = np.fmax(np.fmax(mn[0], mn[1]), np.fmax(mn[2], tmin))
    X = np.fmin(np.fmin(mx[0], mx[1]), mx[2])
    if not np.fmin(X, f32(1e10)) >= E:
        return False, None
    oc = sph[:3] - o
    a, h = dot(d, d), dot(d, oc)
    disc = h * h - a * (dot(oc, oc) - sph[3] * sph[3])
    if disc >= 0:
        sq = np.sqrt(disc)
        root = (h - sq) / a
        if root < tmin or root > f32(1e10):
            root = (h + sq) / a
        if root >= tmin and root < f32(1e10):
            return True, root
    return False, None


def rays(R, n_random, seed):
    """(origin, direction) f32 pairs: origins within the gate (R / 2 of the
    centre, here the origin of the scene) and at the centre; random directions
    and directions within 0 .. 1e-3 of the six axes, at four lengths."""
    rng = np.random.default_rng(seed)

    def origin():
        while True:
            p = rng.uniform(-0.5, 0.5, 3)
            if p @ p <= 0.2499:
                return (p * R).astype(f32)

    out = []
    for k in range(n_random):
        d = rng.normal(size=3)
        d = d / np.linalg.norm(d) * (1.0, 0.37, 1e-3, 30.0)[k % 4]
        out.append((origin() if k % 8 else np.zeros(3, f32), d.astype(f32)))
    for axis in range(3):
        for sign in (1.0, -1.0):
            for eps in (0.0, 1e-9, 1e-7, 1e-5, 1e-3):
                for length in (1.0, 0.37, 1e-3, 30.0):
                    for k in range(4):
                        d = eps * rng.uniform(-1, 1, 3)
                        d[axis] = sign
                        out.append((np.zeros(3, f32) if k == 0 else origin(), (d * length).astype(f32)))
    return out


def check_inline_decision(sa, n_random, seed):
    import oracle
    osc = oracle.OracleScene(sa)
    layout = sd.pack_device(sa, leaf_order=False)  # device sphere rows = the oracle's sphere indices
    row, _ = decode(layout)
    v = layout.shell - 1
    box6 = layout.nodes[(v & ~1) // sd.NODE_BYTES, (v & 1):12:2]
    lo, hi, sph = box6[:3].copy(), box6[3:].copy(), layout.spheres[row].copy()
    R = float(sph[3])
    assert not sph[:3].any()
    n_shell = n_pass = n_fall = 0
    all_rays = rays(R, n_random, seed)
    for o, d in all_rays:
        assert f32(4) * dot(o, o) <= sph[3] * sph[3]  # the gate
        hit, t, ty, ix = oracle.traverse(osc, o, d)
        if not (hit and ty == sd.PRIM_SPHERE and ix == row):
            continue
        n_shell += 1
        inv = inv_dir(d)
        t_entry = f32(t)
        tmin2 = t_entry + f32(0.0001)
        want = oracle.traverse(osc, o, d, float(tmin2))
        got = shell_hit(lo, hi, sph, o, d, inv, tmin2)
        assert got[0] == want[0], (o, d, got, want)
        if not got[0]:
            n_fall += 1  # no exit: the shell is shaded as a surface
            continue
        assert f32(want[1]) == got[1] and want[2:] == (sd.PRIM_SPHERE, row), (o, d, got, want)
        if np.fmax(t_entry, f32(0.001)) < np.fmin(got[1], f32(1e10)) or not got[1] > 0:
            continue  # a scatter inside the medium is possible: not the passthrough studied here
        n_pass += 1
        # passthrough (kernels.py:1100-1110), then the segment from outside
        o2 = o + d * (got[1] + f32(0.001) / np.sqrt(dot(d, d)))
        assert o2.dtype == f32
        want = oracle.traverse(osc, o2, d)
        got = shell_hit(lo, hi, sph, o2, d, inv, f32(0.001))
        assert got[0] == want[0], (o, d, o2, got, want)
        if got[0]:
            assert f32(want[1]) == got[1] and want[2:] == (sd.PRIM_SPHERE, row), (o, d, o2, got, want)
    print(f'R={R}: {len(all_rays)} rays, {n_shell} shell hits, {n_pass} passthroughs, {n_fall} fallbacks')
    assert 3 * n_shell >= len(all_rays)
    return n_shell, n_pass, n_fall


def test_inline_decision_matches_traversal_vol2():
    _, n_pass, _ = check_inline_decision(fixture('vol2_final_scene'), 2520, 11)
    assert n_pass > 0


@pytest.mark.parametrize('R', [5000.0, 100.0])
def test_inline_decision_matches_traversal_synthetic(R):
    _, n_pass, n_fall = check_inline_decision(ss.shell_scene(R)[0], 1000, 12)
    assert (n_pass if R == 5000.0 else n_fall) > 0
