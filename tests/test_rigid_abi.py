"""CPU tests of the rigid-body pose ABI (include/ptmi_rigid.h): its symbol is in
the library and in ptmi.rigid's own table and in none of the other ABIs'; every
rejected argument returns PTMI_EINVAL with its message before a HIP call (no
device is needed: the device pointers are never dereferenced); the host model's
own errors (rigid.Body, rigid.members_of, rigid.check_bodies) and
MI355XRenderer.set_bodies' (checked on a renderer without a device)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ptmi import (_lib, build, core, guide, material, motion, pose, post, renderer, rigid, temporal, tree, update,
                  validate, wf_tiles)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h', 'ptmi_tree.h', 'ptmi_validate.h', 'ptmi_material.h', 'ptmi_build.h', 'ptmi_pose.h')
V = core.vec3


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_rigid.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_pose_rigid'} == set(rigid.EXPORTS) == set(rigid.SIGNATURES)
    assert hasattr(rigid.load(), 'ptmi_pose_rigid')
    assert int(re.search(r'#define PTMI_RIGID_VERSION (\d+)', txt).group(1)) == rigid.RIGID_VERSION == 1
    assert int(re.search(r'#define PTMI_RIGID_MAX_BODIES (\d+)', txt).group(1)) == rigid.MAX_BODIES == 16
    for other in (_lib, post, guide, temporal, wf_tiles, update, motion, tree, validate, material, build, pose):
        assert 'ptmi_pose_rigid' not in other.SIGNATURES
    assert 'ptmi_pose_rigid' not in _lib.EXPORTS
    for other in OTHER_HEADERS:
        assert 'ptmi_rigid' not in header(other) and 'PTMI_RIGID' not in header(other) \
            and 'ptmi_pose_rigid' not in header(other)
    restype, argtypes = rigid.SIGNATURES['ptmi_pose_rigid']
    assert restype is C.c_int and len(argtypes) == 9 and argtypes[5] is C.c_int32
    assert C.sizeof(rigid.RigidList) == 40  # four pointers and a count
    assert C.sizeof(rigid.RigidBody) == 120 == 8 * rigid.BODY_DOUBLES  # 16 of them: 1920 B of kernel arguments
    # the stress library links the shipped object: the symbol is there too
    stress = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libptmi_stress.so')
    if os.path.exists(stress):
        assert hasattr(C.CDLL(stress), 'ptmi_pose_rigid')


def test_rigid_rejects_bad_arguments_before_touching_device():
    lib = rigid.load()
    ends = (C.c_int32 * 3)(2, 3, 4)
    good = rigid.body_table([rigid.Body(V(0, 0, 0), V(0, 1, 0), 0.5)] * 16, 0.25)

    def scene(n_inner=4, ns=3, nq=2, nt=2, ref=4096, nodes=8192, nb=None, spheres=256):
        v = _lib.SceneView()
        v.n_inner, v.num_spheres, v.num_quads, v.num_triangles = n_inner, ns, nq, nt
        v.num_bvh_nodes = (2 * n_inner + 1 if ns + nq + nt else 0) if nb is None else nb
        v.ref_nodes, v.nodes = ref, nodes
        v.spheres, v.quads, v.tris = spheres, 512, 1024
        return v

    def lst(count=1, prim=16, leaf=32, body=48, rec=64):
        return rigid.RigidList(prim, leaf, body, rec, count)

    def call(v=None, s=None, q=None, t=None, bodies=good, n_bodies=1, order=128, slot=160, level_end=ends,
             n_levels=3, root=192, topo=True, null_scene=False, flags=0):
        v = scene() if v is None else v
        tp = update.UpdateTopology(order, slot, level_end, n_levels, flags)
        return lib.ptmi_pose_rigid(None if null_scene else C.byref(v),
                                   *(C.byref(x) if x is not None else None for x in (s, q, t)), bodies, n_bodies,
                                   C.byref(tp) if topo else None, C.c_void_p(root) if root else None, None)

    E = _lib.PTMI_EINVAL
    assert call(null_scene=True) == E and err() == 'rigid: scene is NULL'
    assert call(v=scene(nb=8)) == E and 'rigid: bad scene counts' in err()
    # the body table
    for bad in (-1, 17, 1 << 20):
        assert call(n_bodies=bad) == E and err() == 'rigid: n_bodies outside [0, 16]'
    assert call(bodies=None, n_bodies=1) == E and err() == 'rigid: bodies is NULL'
    for b, k, value in ((0, 0, math.nan), (2, 8, math.inf), (15, 9, -math.inf), (3, 14, math.nan)):
        table = rigid.body_table([rigid.Body(V(0, 0, 0), V(0, 1, 0), 0.5)] * 16, 0.25)
        C.cast(C.byref(table[b]), C.POINTER(C.c_double))[k] = value
        assert call(bodies=table, n_bodies=16) == E and err() == f'rigid: body {b} has a value that is not finite'
        if b:  # a body past n_bodies is not read
            assert call(bodies=table, n_bodies=b, topo=False) == E and 'rigid: topo is NULL' in err()
    # counts
    assert call(s=lst(-1)) == E and 'rigid: sphere count negative or above num_spheres' in err()
    assert call(s=lst(4)) == E and 'sphere count' in err()
    assert call(q=lst(-1)) == E and 'quad count' in err()
    assert call(q=lst(3)) == E and 'rigid: quad count negative or above num_quads' in err()
    assert call(t=lst(-2)) == E and 'triangle count' in err()
    assert call(t=lst(3)) == E and 'rigid: triangle count negative or above num_triangles' in err()
    # lists
    for name, key in (('sphere', 's'), ('quad', 'q'), ('triangle', 't')):
        for field in ('prim', 'leaf'):
            assert call(**{key: lst(**{field: None})}) == E and f'rigid: a {name} list pointer is NULL/misaligned' in err()
            assert call(**{key: lst(**{field: 18})}) == E and f'a {name} list pointer is NULL/misaligned' in err()
        for rec in (None, 68, 60, 65):  # NULL; 4-byte aligned is not enough for f64
            assert call(**{key: lst(rec=rec)}) == E and f"rigid: a {name} list's rec is NULL or not 8-byte aligned" in err()
        for body in (None, 50, 49):
            assert call(**{key: lst(body=body)}) == E \
                and f"rigid: a {name} list's body is NULL or not 4-byte aligned" in err()
        # an empty list's pointers are not looked at
        assert call(**{key: lst(count=0, prim=None, leaf=None, body=None, rec=None)}, topo=False) == E \
            and 'topo is NULL' in err()
    assert call(v=scene(spheres=None), s=lst()) == E and 'a sphere list pointer is NULL/misaligned' in err()
    # the scene's own arrays and the topology: the update call's cases, by the same code
    assert call(v=scene(ref=None)) == E and 'rigid: ref_nodes NULL/misaligned' in err()
    assert call(v=scene(n_inner=0, ns=1, nq=0, nt=0, ref=None), s=lst()) == E and 'ref_nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=None)) == E and 'rigid: nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=8200)) == E and 'nodes NULL/misaligned' in err()
    assert call(topo=False) == E and 'rigid: topo is NULL' in err()
    assert call(order=None) == E and 'rigid: order NULL/misaligned' in err()
    assert call(slot=None) == E and 'slot NULL/misaligned' in err()
    assert call(slot=162) == E and 'rigid: slot NULL/misaligned' in err()
    assert call(root=None) == E and 'rigid: root_box NULL/misaligned' in err()
    assert call(level_end=None) == E and 'rigid: level_end is NULL or n_levels < 1' in err()
    assert call(n_levels=0) == E and 'level_end is NULL or n_levels < 1' in err()
    for bad in ((2, 2, 4), (2, 1, 4), (0, 3, 4), (2, 3, 5), (1, 2, 3)):
        assert call(level_end=(C.c_int32 * 3)(*bad)) == E and 'rigid: level ends must ascend strictly to n_inner' in err()
    assert call(n_levels=2) == E and 'level ends' in err()
    assert call(flags=2) == E and 'rigid: unknown flags' in err()
    assert call(flags=-1) == E and 'unknown flags' in err()
    many = (C.c_int32 * 65)(*(list(range(1, 65)) + [70]))
    assert call(v=scene(n_inner=70, ns=71, nq=0, nt=0), level_end=many, n_levels=65, flags=update.ONE_GROUP) == E \
        and 'rigid: too many levels for PTMI_UPDATE_ONE_GROUP' in err()
    # an empty world: nothing to do, no launch, whatever else is passed
    assert call(v=scene(n_inner=0, ns=0, nq=0, nt=0), topo=False, root=None) == _lib.PTMI_OK
    assert call(v=scene(n_inner=0, ns=0, nq=0, nt=0), topo=False, root=None, bodies=None, n_bodies=0) == _lib.PTMI_OK


# ------------------------------------------------------------------ the host model
def test_rotation_matrix_and_body_at():
    I = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    for axis in (V(0, 0, 1), V(1, 2, -3), V(-1e-3, 5, 0)):
        b = rigid.Body(V(1, 2, 3), axis, 0.0, V(0.5, 0, -1))
        assert rigid.rotation_matrix(b.axis, 0.0) == I  # -0.0 == 0.0
        assert rigid.body_at(b, 0.5) == I + (1.0, 2.0, 3.0) + (1.25, 2.0, 2.5)
    R = np.array(rigid.rotation_matrix(V(0, 0, 1), math.pi / 2)).reshape(3, 3)
    assert np.allclose(R @ [1, 0, 0], [0, 1, 0], atol=1e-15) and np.allclose(R @ [0, 0, 1], [0, 0, 1], atol=0)
    b = rigid.Body(V(0, 0, 0), V(3, 0, 4), 2.0)
    assert b.axis.to_list() == [3 / 5.0, 0.0, 4 / 5.0]  # normalised once: x * x, sqrt, /
    R = np.array(rigid.body_at(b, 0.25)[:9]).reshape(3, 3)
    assert R.tolist() == np.array(rigid.rotation_matrix(b.axis, 0.5)).reshape(3, 3).tolist()
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.allclose(R @ b.axis.to_list(), b.axis.to_list())
    # a point and a vector in the documented order of operations
    p, c, ct = V(1.5, -2.25, 0.1), V(0.3, 0.2, 0.1), V(7.0, 8.0, 9.0)
    flat = tuple(R.reshape(-1).tolist())
    q = p - c
    want = [(flat[3 * k] * q.x + flat[3 * k + 1] * q.y) + flat[3 * k + 2] * q.z + x for k, x in enumerate(ct.to_list())]
    assert core.rigid_point(flat, c, ct, p).to_list() == want


def test_transformed_objects_rotate_the_rest_vectors():
    mat = core.lambertian(core.solid_color(V(0.5, 0.5, 0.5)))
    q = core.quad(V(1, 0, 0), V(2, 0, 0), V(0, 3, 0), mat)
    t = core.triangle(V(1, 0, 0), V(2, 0, 0), V(1, 1, 0), mat)
    R = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)  # a quarter turn about z, exactly
    c, ct = V(0, 0, 0), V(0, 0, 5)
    q2 = core.quad.transformed(q, R, c, ct)
    assert q2.Q.to_list() == [0, 1, 5] and q2.u.to_list() == [0, 2, 0] and q2.v.to_list() == [-3, 0, 0]
    assert q2.normal.to_list() == [0, 0, 1] and q2.D == 5.0 and q2.w.to_list() == [0, 0, 1 / 6.0] and q2.mat is mat
    assert (q2.bbox.x.min, q2.bbox.x.max, q2.bbox.y.min, q2.bbox.y.max) == (-3, 0, 1, 3)
    assert q2.bbox.z.max - q2.bbox.z.min == pytest.approx(1e-4)  # padded, as the constructor pads
    t2 = core.triangle.transformed(t, R, c, ct)
    assert [v.to_list() for v in (t2.v0, t2.v1, t2.v2)] == [[0, 1, 5], [0, 2, 5], [-1, 1, 5]]
    assert t2.edge1.to_list() == [0, 1, 0] and t2.edge2.to_list() == [-1, 0, 0] and t2.normal.to_list() == [0, 0, 1]
    assert (t2.bbox.x.min, t2.bbox.y.max) == (-1, 2) and t2.mat is mat
    s = core.Sphere.stationary(V(1, 0, 0), 0.5, mat)
    at = R + tuple(c.to_list()) + tuple(ct.to_list())
    s2 = rigid.posed_object('spheres', s, at)
    assert s2.center.origin.to_list() == [0, 1, 5] and s2.radius == 0.5 and s2.center.direction.to_list() == [0, 0, 0]


def test_body_raises_every_error_with_its_message():
    ok = dict(pivot=V(0, 0, 0), axis=V(0, 1, 0), turn=1.0)
    rigid.Body(**ok, spheres=[2, 0], quads=(1,), triangles=range(3))
    for key, value, message in (('axis', V(0, 0, 0), 'the axis must not be zero'),
                                ('axis', V(0, math.nan, 0), 'axis must be a finite vec3'),
                                ('axis', (0, 1, 0), 'axis must be a finite vec3'),
                                ('pivot', V(math.inf, 0, 0), 'pivot must be a finite vec3'),
                                ('turn', math.nan, 'turn must be finite'),
                                ('turn', -math.inf, 'turn must be finite')):
        with pytest.raises(ValueError, match='^body: ' + re.escape(message) + '$'):
            rigid.Body(**dict(ok, **{key: value}))
    with pytest.raises(ValueError, match='^body: displacement must be a finite vec3$'):
        rigid.Body(**ok, displacement=V(0, 0, math.nan))
    with pytest.raises(ValueError, match='^body: an index of quads is repeated$'):
        rigid.Body(**ok, quads=[1, 2, 1])
    with pytest.raises(ValueError, match='^body: triangles must be primitive indices >= 0$'):
        rigid.Body(**ok, triangles=[-1])
    with pytest.raises(ValueError, match='^body: spheres must be primitive indices >= 0$'):
        rigid.Body(**ok, spheres=[0.5])


def test_members_of_and_check_bodies_raise_every_error():
    ok = dict(pivot=V(0, 0, 0), axis=V(0, 1, 0), turn=1.0)
    a, b = rigid.Body(**ok, spheres=[0, 2], quads=[1]), rigid.Body(**ok, spheres=[1], triangles=[0, 1])
    assert rigid.members_of([a, b]) == {'spheres': {0: 0, 2: 0, 1: 1}, 'quads': {1: 0}, 'triangles': {0: 1, 1: 1}}
    assert rigid.members_of([]) == {'spheres': {}, 'quads': {}, 'triangles': {}}
    with pytest.raises(ValueError, match=r'^spheres\[2\] is in bodies 0 and 1$'):
        rigid.members_of([a, rigid.Body(**ok, spheres=[2])])
    with pytest.raises(ValueError, match='^at most 16 bodies, not 17$'):
        rigid.members_of([rigid.Body(**ok, triangles=[i]) for i in range(17)])
    rigid.members_of([rigid.Body(**ok, triangles=[i]) for i in range(16)])
    with pytest.raises(ValueError, match=r'^bodies\[1\] is not a rigid.Body$'):
        rigid.members_of([a, 'b'])
    mat = core.lambertian(core.solid_color(V(0.5, 0.5, 0.5)))
    prims = {'spheres': [core.Sphere.stationary(V(i, 2, 3), 0.5, mat) for i in range(3)],
             'quads': [core.quad(V(0, 0, i), V(1, 0, 0), V(0, 1, 0), mat) for i in range(2)],
             'triangles': [core.triangle(V(0, 0, i), V(1, 0, i), V(0, 1, i), mat) for i in range(2)]}
    (si, sb, sr), (qi, qb, qr), (ti, tb, tr) = records = rigid.body_records([a, b], prims)
    assert si.tolist() == [0, 1, 2] and sb.tolist() == [0, 1, 0] and sb.dtype == np.int32
    assert sr.tolist() == [[0, 2, 3], [1, 2, 3], [2, 2, 3]]
    assert qi.tolist() == [1] and qr.tolist() == [[0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1]]
    assert ti.tolist() == [0, 1] and tb.tolist() == [1, 1]
    assert tr[1].tolist() == [0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert rigid.body_records([], prims) == (None, None, None)
    with pytest.raises(ValueError, match=r'^quads: no primitive 5 \(the scene has 2\)$'):
        rigid.body_records([rigid.Body(**ok, quads=[5])], prims)
    counts = (3, 2, 2)  # by code: spheres, triangles, quads
    bodies, got = rigid.check_bodies(counts, [a, b], records)
    assert bodies == [a, b] and sorted(got) == [0, 1, 2] and got[2][2].shape == (1, 15) and got[1][1].dtype == np.int32
    assert rigid.check_bodies(counts, [], (None, None, None)) == ([], {})

    def bad(kind, message, **change):
        pos = rigid.KIND_NAMES.index(kind)
        arg = dict(zip(('idx', 'body', 'rec'), records[pos]))
        arg.update(change)
        new = list(records)
        new[pos] = (arg['idx'], arg['body'], arg['rec'])
        with pytest.raises(ValueError, match='^' + re.escape(f'{kind}: {message}') + '$'):
            rigid.check_bodies(counts, [a, b], tuple(new))

    bad('spheres', 'an index is outside [0, 3)', idx=np.array([0, 1, 3]))
    bad('triangles', 'an index is repeated', idx=np.array([1, 1]))
    bad('spheres', 'body indices must be n integers in [0, 2)', body=np.array([0, 2, 0], np.int32))
    bad('spheres', 'body indices must be n integers in [0, 2)', body=np.array([0, -1, 0], np.int32))
    bad('quads', 'body indices must be n integers in [0, 2)', body=np.array([0.0]))
    bad('quads', 'body indices must be n integers in [0, 2)', body=np.array([0, 0], np.int32))
    bad('quads', 'rest records must be (n, 15) f64', rec=np.zeros((1, 9)))
    bad('triangles', 'rest records must be (n, 18) f64', rec=np.zeros((2, 12)))
    rec = np.zeros((3, 3))
    rec[1, 1] = np.nan
    bad('spheres', 'rest records must be finite', rec=rec)
    with pytest.raises(ValueError, match='^rigid records must be'):
        rigid.check_bodies(counts, [a, b], records[:2])


def test_set_bodies_raises_every_error_without_a_device():
    """set_bodies' checks need no device: a renderer object with only its primitive lists and motion."""
    mat = core.lambertian(core.solid_color(V(0.5, 0.5, 0.5)))
    r = renderer.MI355XRenderer.__new__(renderer.MI355XRenderer)
    r._prims = {'spheres': [core.Sphere.stationary(V(0, 0, 0), 0.5, mat),
                            core.Sphere.moving(V(2, 0, 0), V(2, 1, 0), 0.5, mat)],
                'quads': [core.quad(V(0, 0, i), V(1, 0, 0), V(0, 1, 0), mat) for i in range(3)],
                'triangles': [core.triangle(V(0, 0, i), V(1, 0, i), V(0, 1, i), mat) for i in range(20)]}
    r._motion = {'quads': {2: V(0, 0, 1)}, 'triangles': {}}
    r._motion_edits, r._bodies = 0, []
    ok = dict(pivot=V(0, 0, 0), axis=V(0, 1, 0), turn=1.0)
    r.set_bodies([rigid.Body(**ok, spheres=[0], quads=[0, 1]), rigid.Body(**ok, triangles=range(20))])
    assert len(r._bodies) == 2 and r._motion_edits == 1
    for bodies, message in (
            ([rigid.Body(**ok, quads=[0]), rigid.Body(**ok, quads=[1, 0])], r'quads\[0\] is in bodies 0 and 1'),
            ([rigid.Body(**ok, quads=[2])], r'quads\[2\] is in a body and moves linearly'),
            ([rigid.Body(**ok, spheres=[1])], r'spheres\[1\] is in a body and moves linearly'),
            ([rigid.Body(**ok, quads=[3])], r'quads: no primitive 3 \(the scene has 3\)'),
            ([rigid.Body(**ok, triangles=[i]) for i in range(17)], 'at most 16 bodies, not 17')):
        with pytest.raises(ValueError, match='^' + message + '$'):
            r.set_bodies(bodies)
        assert len(r._bodies) == 2 and r._motion_edits == 1  # a refused call changes nothing
    r.set_bodies([rigid.Body(**ok, triangles=[i]) for i in range(16)])
    assert len(r._bodies) == 16
    r.set_bodies([])
    assert r._bodies == [] and r._motion_edits == 3
    # the digest a checkpoint carries: of the parameters and the members
    a, b = rigid.Body(**ok, quads=[0, 1]), rigid.Body(**ok, quads=[0], triangles=[1])
    assert rigid.digest([a]) == rigid.digest([rigid.Body(**ok, quads=[1, 0])]) != rigid.digest([b])
    assert rigid.digest([a]) != rigid.digest([rigid.Body(**dict(ok, turn=1.5), quads=[0, 1])])
    assert rigid.digest([a, b]) != rigid.digest([b, a]) and rigid.digest([]) != rigid.digest([a])
