"""CPU tests of the pose ABI (include/ptmi_pose.h): its symbol is in the library
and in ptmi.pose's own table and in none of the other ABIs'; every rejected
argument returns PTMI_EINVAL with its message before a HIP call (no device is
needed: the device pointers are never dereferenced); the shutter sequence
(pose.vdc, pose.slice_times) and the checks of set_tracks' arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ptmi import _lib, build, core, guide, material, motion, pose, post, temporal, tree, update, validate, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h', 'ptmi_tree.h', 'ptmi_validate.h', 'ptmi_material.h', 'ptmi_build.h')


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_pose.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_pose_primitives'} == set(pose.EXPORTS) == set(pose.SIGNATURES)
    assert hasattr(pose.load(), 'ptmi_pose_primitives')
    assert int(re.search(r'#define PTMI_POSE_VERSION (\d+)', txt).group(1)) == pose.POSE_VERSION == 1
    for other in (_lib, post, guide, temporal, wf_tiles, update, motion, tree, validate, material, build):
        assert 'ptmi_pose_primitives' not in other.SIGNATURES
    for other in OTHER_HEADERS:
        assert 'ptmi_pose' not in header(other) and 'PTMI_POSE' not in header(other)
    restype, argtypes = pose.SIGNATURES['ptmi_pose_primitives']
    assert restype is C.c_int and len(argtypes) == 8 and argtypes[4] is C.c_double
    assert C.sizeof(pose.PoseList) == 32  # three pointers and a count
    # the stress library links the shipped object: the symbol is there too
    stress = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libptmi_stress.so')
    if os.path.exists(stress):
        assert hasattr(C.CDLL(stress), 'ptmi_pose_primitives')


def test_pose_rejects_bad_arguments_before_touching_device():
    lib = pose.load()
    ends = (C.c_int32 * 3)(2, 3, 4)

    def scene(n_inner=4, ns=3, nq=2, nt=2, ref=4096, nodes=8192, nb=None, spheres=256):
        v = _lib.SceneView()
        v.n_inner, v.num_spheres, v.num_quads, v.num_triangles = n_inner, ns, nq, nt
        v.num_bvh_nodes = (2 * n_inner + 1 if ns + nq + nt else 0) if nb is None else nb
        v.ref_nodes, v.nodes = ref, nodes
        v.spheres, v.quads, v.tris = spheres, 512, 1024
        return v

    def lst(count=1, prim=16, leaf=32, rec=64):
        return pose.PoseList(prim, leaf, rec, count)

    def call(v=None, s=None, q=None, t=None, time=0.5, order=128, slot=160, level_end=ends, n_levels=3, root=192,
             topo=True, null_scene=False, flags=0):
        v = scene() if v is None else v
        tp = update.UpdateTopology(order, slot, level_end, n_levels, flags)
        return lib.ptmi_pose_primitives(None if null_scene else C.byref(v),
                                        *(C.byref(x) if x is not None else None for x in (s, q, t)), time,
                                        C.byref(tp) if topo else None, C.c_void_p(root) if root else None, None)

    E = _lib.PTMI_EINVAL
    assert call(null_scene=True) == E and err() == 'pose: scene is NULL'
    assert call(v=scene(nb=8)) == E and 'pose: bad scene counts' in err()
    # the time
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(time=bad) == E and err() == 'pose: t is not finite'
    # counts
    assert call(s=lst(-1)) == E and 'pose: sphere count negative or above num_spheres' in err()
    assert call(s=lst(4)) == E and 'sphere count' in err()
    assert call(q=lst(-1)) == E and 'quad count' in err()
    assert call(q=lst(3)) == E and 'pose: quad count negative or above num_quads' in err()
    assert call(t=lst(-2)) == E and 'triangle count' in err()
    assert call(t=lst(3)) == E and 'pose: triangle count negative or above num_triangles' in err()
    # lists
    for name, key in (('sphere', 's'), ('quad', 'q'), ('triangle', 't')):
        for field in ('prim', 'leaf'):
            assert call(**{key: lst(**{field: None})}) == E and f'pose: a {name} list pointer is NULL/misaligned' in err()
            assert call(**{key: lst(**{field: 18})}) == E and f'a {name} list pointer is NULL/misaligned' in err()
        for rec in (None, 68, 60, 65):  # NULL; 4-byte aligned is not enough for f64
            assert call(**{key: lst(rec=rec)}) == E and f"pose: a {name} list's rec is NULL or not 8-byte aligned" in err()
    assert call(v=scene(spheres=None), s=lst()) == E and 'a sphere list pointer is NULL/misaligned' in err()
    # the scene's own arrays and the topology: the update call's cases, by the same code
    assert call(v=scene(ref=None)) == E and 'pose: ref_nodes NULL/misaligned' in err()
    assert call(v=scene(n_inner=0, ns=1, nq=0, nt=0, ref=None), s=lst()) == E and 'ref_nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=None)) == E and 'pose: nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=8200)) == E and 'nodes NULL/misaligned' in err()
    assert call(topo=False) == E and 'pose: topo is NULL' in err()
    assert call(order=None) == E and 'pose: order NULL/misaligned' in err()
    assert call(slot=None) == E and 'slot NULL/misaligned' in err()
    assert call(slot=162) == E and 'pose: slot NULL/misaligned' in err()
    assert call(root=None) == E and 'pose: root_box NULL/misaligned' in err()
    assert call(level_end=None) == E and 'pose: level_end is NULL or n_levels < 1' in err()
    assert call(n_levels=0) == E and 'level_end is NULL or n_levels < 1' in err()
    for bad in ((2, 2, 4), (2, 1, 4), (0, 3, 4), (2, 3, 5), (1, 2, 3)):
        assert call(level_end=(C.c_int32 * 3)(*bad)) == E and 'pose: level ends must ascend strictly to n_inner' in err()
    assert call(n_levels=2) == E and 'level ends' in err()
    assert call(flags=2) == E and 'pose: unknown flags' in err()
    assert call(flags=-1) == E and 'unknown flags' in err()
    many = (C.c_int32 * 65)(*(list(range(1, 65)) + [70]))
    assert call(v=scene(n_inner=70, ns=71, nq=0, nt=0), level_end=many, n_levels=65, flags=update.ONE_GROUP) == E \
        and 'pose: too many levels for PTMI_UPDATE_ONE_GROUP' in err()
    # an empty world: nothing to do, no launch, whatever else is passed
    assert call(v=scene(n_inner=0, ns=0, nq=0, nt=0), topo=False, root=None) == _lib.PTMI_OK


# ------------------------------------------------------------------ the shutter sequence
def test_vdc_is_the_bit_reversal():
    assert [pose.vdc(j) for j in range(8)] == [0.0, 0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875]
    assert pose.vdc(0xffffffff) == (2 ** 32 - 1) / 2 ** 32 and pose.vdc(1 << 32) == 0.0  # the low 32 bits
    assert pose.vdc(0x80000000) == 2.0 ** -32


@pytest.mark.parametrize('m', [0, 1, 3, 6])
def test_the_first_2_to_the_m_slice_times_are_the_multiples_of_2_to_the_minus_m(m):
    n, spp = 1 << m, 4
    got = pose.slice_times(0, n * spp, spp, (0.0, 1.0))
    assert [(j, b, c) for j, _, b, c in got] == [(j, j * spp, spp) for j in range(n)]
    assert sorted(t for _, t, _, _ in got) == [k / n for k in range(n)]
    assert sum(t for _, t, _, _ in got) / n == (n - 1) / (2 * n)  # the mean is not 1/2
    lo, hi = 0.25, 0.75
    assert [t for _, t, _, _ in pose.slice_times(0, n * spp, spp, (lo, hi))] == \
        [lo + (hi - lo) * pose.vdc(j) for j in range(n)]


def test_slices_are_global_whatever_the_chunks():
    def per_sample(chunks, spp):
        return [(j, t) for b, c in chunks for j, t, begin, n in pose.slice_times(b, c, spp, (0.0, 1.0))
                for _ in range(n)]

    for spp in (1, 2, 3, 16):
        whole = per_sample([(0, 8)], spp)
        assert whole == per_sample([(0, 3), (3, 5)], spp) == per_sample([(k, 1) for k in range(8)], spp)
        assert whole == [(s // spp, pose.vdc(s // spp)) for s in range(8)]
    assert pose.slice_times(3, 5, 2, (0.0, 1.0)) == [(1, 0.5, 3, 1), (2, 0.25, 4, 2), (3, 0.75, 6, 2)]
    assert pose.slice_times(5, 0, 2, (0.0, 1.0)) == []
    assert pose.SLICE_SPP == 16 and len(pose.slice_times(0, 1024, pose.SLICE_SPP, (0.0, 1.0))) == 64
    for bad in ((1.0, 0.0), (0.0, float('nan')), (0.0,), None):
        with pytest.raises(ValueError, match='shutter must be'):
            pose.slice_times(0, 8, 2, bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='slice_spp must be'):
            pose.slice_times(0, 8, bad, (0.0, 1.0))


# ------------------------------------------------------------------ tracks
def test_tracks_of_and_track_records():
    mat = core.lambertian(core.solid_color(core.vec3(0.5, 0.5, 0.5)))
    still = core.Sphere.stationary(core.vec3(1, 2, 3), 0.5, mat)
    moving = core.Sphere.moving(core.vec3(1, 2, 3), core.vec3(1, 2.5, 3), 0.5, mat)
    q = core.quad(core.vec3(0, 0, 0), core.vec3(1, 0, 0), core.vec3(0, 1, 0), mat)
    t = core.triangle(core.vec3(0, 0, 0), core.vec3(1, 0, 0), core.vec3(0, 1, 0), mat)
    prims = {'spheres': [still, moving], 'quads': [q, q], 'triangles': [t]}
    tracks = pose.tracks_of(prims, {'quads': {1: core.vec3(0, 0, 2)}, 'triangles': {0: core.vec3(3, 0, 0)}})
    assert {k: sorted(v) for k, v in tracks.items()} == {'spheres': [1], 'quads': [1], 'triangles': [0]}
    (si, sr), (qi, qr), (ti, tr) = pose.track_records(tracks)
    assert si.tolist() == [1] and sr.tolist() == [[1, 2, 3, 0, 0.5, 0]]
    assert qi.tolist() == [1] and qr.tolist() == [[0, 0, 0, 0, 0, 2, 0, 0, 1]]
    assert ti.tolist() == [0] and tr.tolist() == [[0, 0, 0, 1, 0, 0, 0, 1, 0, 3, 0, 0]]
    assert pose.track_records(pose.tracks_of({'spheres': [still], 'quads': [], 'triangles': []})) == (None, None, None)
    # the posed sphere is center.at(t), and a translated triangle keeps its edges
    s_half = pose.posed_object('spheres', moving, moving.center.direction, 0.5)
    assert s_half.center.at(0.0).to_list() == moving.center.at(0.5).to_list() == [1, 2.25, 3]
    moved = core.triangle.translated(t, core.vec3(0.1, 0.2, 0.3))
    assert moved.edge1 is t.edge1 and moved.normal is t.normal and moved.v1.to_list() == [1.1, 0.2, 0.3]
    assert moved.bbox.x.min == 0.1 and moved.bbox.y.max == 1.2


def test_check_tracks_raises_every_error_with_its_message():
    counts = (3, 2, 2)  # by code: spheres, triangles, quads
    good = {'spheres': (np.array([0, 2]), np.zeros((2, 6))), 'quads': (np.array([1]), np.ones((1, 9))),
            'triangles': (np.array([0, 1]), np.ones((2, 12)))}
    got = pose.check_tracks(counts, **good)
    assert sorted(got) == [0, 1, 2] and got[2][1].shape == (1, 9) and got[1][1].dtype == np.float64
    assert pose.check_tracks(counts) == {} == pose.check_tracks(counts, spheres=(np.zeros(0, np.int64), np.zeros((0, 6))))

    def bad(kind, message, idx=None, rec=None):
        arg = tuple(g if v is None else v for g, v in zip(good[kind], (idx, rec)))
        with pytest.raises(ValueError, match='^' + re.escape(f'{kind}: {message}') + '$'):
            pose.check_tracks(counts, **{kind: arg})

    bad('spheres', 'indices must be a 1-D integer array', idx=np.array([[0, 2]]))
    bad('spheres', 'indices must be a 1-D integer array', idx=np.array([0.0, 2.0]))
    bad('spheres', 'an index is outside [0, 3)', idx=np.array([0, 3]))
    bad('quads', 'an index is outside [0, 2)', idx=np.array([-1]))
    bad('triangles', 'an index is repeated', idx=np.array([1, 1]))
    bad('spheres', 'track records must be (n, 6) f64', rec=np.zeros((2, 9)))
    bad('quads', 'track records must be (n, 9) f64', rec=np.zeros((1, 6)))
    bad('triangles', 'track records must be (n, 12) f64', rec=np.zeros((1, 12)))
    for value in (np.nan, np.inf):
        rec = np.zeros((2, 6))
        rec[1, 4] = value
        bad('spheres', 'track records must be finite', rec=rec)
