"""CPU tests of the scene-update ABI (include/ptmi_update.h): its symbol is in
the library and in ptmi.update's own table and in none of the other five ABIs';
every rejected argument returns PTMI_EINVAL with its message before a HIP call
(no device is needed: the device pointers are never dereferenced); the numpy
reference (update_helpers.refit) is the identity on the built trees and undoes
an edit by its inverse; the arithmetic the kernels call, run on the CPU by
csrc/update_check.cpp, equals numpy bit for bit, also under the sanitizers; and
the host-side topology orders every node after its children."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import parity_helpers as ph
import update_helpers as uh
from ptmi import _lib, guide, post, scene_data as sd, temporal, update, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
SCENES = [('vol2_final_scene', None), ('coverage', 64), ('cornell_mesh_fog', 64)]


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_update.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_update_primitives'} == set(update.EXPORTS) == set(update.SIGNATURES)
    assert hasattr(update.load(), 'ptmi_update_primitives')
    assert int(re.search(r'#define PTMI_UPDATE_VERSION (\d+)', txt).group(1)) == update.UPDATE_VERSION == 1
    for other in (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES, wf_tiles.SIGNATURES):
        assert 'ptmi_update_primitives' not in other
    for other in ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h'):
        assert 'ptmi_update' not in header(other) and 'PTMI_UPDATE' not in header(other)
    restype, argtypes = update.SIGNATURES['ptmi_update_primitives']
    assert restype is C.c_int and len(argtypes) == 7
    # the structs are the header's: four pointers and a count; two device pointers, a host pointer and a count
    assert C.sizeof(update.UpdateList) == 40 and C.sizeof(update.UpdateTopology) == 32


def test_update_rejects_bad_arguments_before_touching_device():
    lib = update.load()
    ends = (C.c_int32 * 3)(2, 3, 4)

    def scene(n_inner=4, ns=3, nq=2, nt=2, ref=4096, nodes=8192, nb=None):
        v = _lib.SceneView()
        v.n_inner, v.num_spheres, v.num_quads, v.num_triangles = n_inner, ns, nq, nt
        v.num_bvh_nodes = (2 * n_inner + 1 if ns + nq + nt else 0) if nb is None else nb
        v.ref_nodes, v.nodes = ref, nodes
        v.spheres, v.quads, v.tris = 256, 512, 1024
        return v

    def lst(count=1, prim=16, leaf=32, row=48, build=64):
        return update.UpdateList(prim, leaf, row, build, count)

    def call(v=None, s=None, q=None, t=None, order=128, slot=160, level_end=ends, n_levels=3, root=192, topo=True,
             null_scene=False, flags=0):
        v = scene() if v is None else v
        tp = update.UpdateTopology(order, slot, level_end, n_levels, flags)
        return lib.ptmi_update_primitives(None if null_scene else C.byref(v), *(C.byref(x) if x is not None else None
                                                                              for x in (s, q, t)),
                                          C.byref(tp) if topo else None, C.c_void_p(root) if root else None, None)

    E = _lib.PTMI_EINVAL
    assert call(null_scene=True) == E and 'scene is NULL' in err()
    assert call(v=scene(nb=8)) == E and 'bad scene counts' in err()
    # counts
    assert call(s=lst(-1)) == E and 'sphere count negative or above num_spheres' in err()
    assert call(s=lst(4)) == E and 'sphere count' in err()
    assert call(q=lst(-1)) == E and 'quad count' in err()
    assert call(q=lst(3)) == E and 'quad count negative or above num_quads' in err()
    assert call(t=lst(-2)) == E and 'triangle count' in err()
    assert call(t=lst(3)) == E and 'triangle count negative or above num_triangles' in err()
    # lists
    for field in ('prim', 'leaf', 'row', 'build'):
        assert call(s=lst(**{field: None})) == E and 'a sphere list pointer is NULL/misaligned' in err()
        assert call(q=lst(**{field: 18})) == E and 'a quad list pointer is NULL/misaligned' in err()
        assert call(t=lst(**{field: None})) == E and 'a triangle list pointer is NULL/misaligned' in err()
    # the scene's own arrays and the topology
    assert call(v=scene(ref=None)) == E and 'ref_nodes NULL/misaligned' in err()
    assert call(v=scene(n_inner=0, ns=1, nq=0, nt=0, ref=None), s=lst()) == E and 'ref_nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=None)) == E and 'nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=8200)) == E and 'nodes NULL/misaligned' in err()
    assert call(topo=False) == E and 'topo is NULL' in err()
    assert call(order=None) == E and 'order NULL/misaligned' in err()
    assert call(slot=None) == E and 'slot NULL/misaligned' in err()
    assert call(slot=162) == E and 'slot NULL/misaligned' in err()
    assert call(root=None) == E and 'root_box NULL/misaligned' in err()
    assert call(level_end=None) == E and 'level_end is NULL or n_levels < 1' in err()
    assert call(n_levels=0) == E and 'level_end is NULL or n_levels < 1' in err()
    for bad in ((2, 2, 4), (2, 1, 4), (0, 3, 4), (2, 3, 5), (1, 2, 3)):
        assert call(level_end=(C.c_int32 * 3)(*bad)) == E and 'level ends must ascend strictly to n_inner' in err()
    assert call(n_levels=2) == E and 'level ends' in err()  # ends at 3, not at n_inner
    assert call(flags=2) == E and 'unknown flags' in err()
    assert call(flags=-1) == E and 'unknown flags' in err()
    many = (C.c_int32 * 65)(*(list(range(1, 65)) + [70]))  # 65 levels: one more than the single-workgroup form takes
    assert call(v=scene(n_inner=70, ns=71, nq=0, nt=0), level_end=many, n_levels=65, flags=update.ONE_GROUP) == E \
        and 'too many levels for PTMI_UPDATE_ONE_GROUP' in err()
    # an empty world: nothing to do, no launch, whatever else is passed
    assert call(v=scene(n_inner=0, ns=0, nq=0, nt=0), topo=False, root=None) == _lib.PTMI_OK


@pytest.mark.parametrize('name,width', SCENES)
def test_reference_refit_is_the_identity_and_undoes_an_edit(name, width):
    sa = ph.fixture(name, width)
    assert uh.arrays_equal(uh.refit(sa), sa)  # internal boxes are exact unions of their children's
    rng = np.random.default_rng(5)
    ns = sa.num_spheres
    idx = rng.choice(ns, size=min(ns, 7), replace=False)
    edits = {'spheres': uh.sphere_edit(idx, sa.sphere_data[idx, 0:3] + rng.uniform(-40, 40, (len(idx), 3)).astype(f32),
                                       sa.sphere_data[idx, 3] * f32(0.5))}
    if sa.num_quads:
        edits['quads'] = uh.quad_edit([0], [((1.0, 2.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 5.0))])
    if sa.num_triangles:
        edits['triangles'] = uh.tri_edit([sa.num_triangles - 1], [((0.0, 0.0, 0.0), (9.0, 1.0, 0.0), (0.0, 7.0, 2.0))])
    moved = uh.refit(sa, edits)
    assert not uh.arrays_equal(moved, sa)
    back = uh.refit(moved, {k: uh.current(sa, k, e[0]) for k, e in edits.items()})
    assert uh.arrays_equal(back, sa)
    # and the packed image follows: pack_device of the refit arrays differs from, then equals, the original's
    assert uh.layouts_equal(sd.pack_device(moved), sd.pack_device(sa))
    assert uh.layouts_equal(sd.pack_device(back), sd.pack_device(sa)) == []


@pytest.mark.parametrize('name,width', SCENES)
def test_topology_orders_children_before_parents(name, width):
    sa = ph.fixture(name, width)
    order, level_end, slot = update.topology(sa.bvh)
    left, right, pidx = sa.bvh['bvh_left_child'], sa.bvh['bvh_right_child'], sa.bvh['bvh_prim_idx']
    inner = np.nonzero(pidx < 0)[0]
    assert sorted(order.tolist()) == inner.tolist() and level_end[-1] == len(inner) and np.all(np.diff(level_end) > 0)
    assert np.array_equal(slot, sd.node_slots(left, right, pidx >= 0)[0])
    level = np.full(len(left), len(level_end), np.int64)  # leaves: below every level
    for j, (a, b) in enumerate(zip([0] + level_end[:-1].tolist(), level_end.tolist())):
        level[order[a:b]] = len(level_end) - 1 - j
    assert level[0] == 0  # the root is alone in the last level
    for i in inner:  # both children lie in the level launched just before the node's, or are leaves
        for c in (left[i], right[i]):
            assert level[c] == level[i] + 1 or pidx[c] >= 0
    assert len(level_end) == int(sd.leaf_depths(sa.bvh)[inner].max()) + 1


# ------------------------------------------------------------------ the numpy halves of DeviceScene.update_primitives
# every count differs (9 spheres, 7 quads, 5 triangles; 6, 9, 3002), so a swap of two kinds changes a shape or a byte
HOST_SCENES = [('kernel_paths_materials', None), ('coverage', 64)]
KIND_NAMES = {'spheres': 0, 'triangles': 1, 'quads': 2}  # the API name -> the type code, restated here


@pytest.mark.parametrize('name,width', HOST_SCENES)
def test_index_maps_agree_with_the_reference_and_invert_prim_perm(name, width):
    sa = ph.fixture(name, width)
    lay = sd.pack_device(sa)
    counts = (sa.num_spheres, sa.num_triangles, sa.num_quads)
    assert len(set(counts)) == 3 and min(counts) > 0
    maps = update.index_maps(sa.bvh, lay.prim_perm, counts)
    assert tuple(sd.counts_by_code(sa)) == counts == tuple(sd.counts_by_code(lay))
    for kind, t in KIND_NAMES.items():
        leaf_of, dev_of = getattr(maps['leaf_of'], kind), getattr(maps['dev_of'], kind)
        assert leaf_of is maps['leaf_of'][t] and dev_of is maps['dev_of'][t]
        assert leaf_of.dtype == dev_of.dtype == np.int64 and leaf_of.shape == dev_of.shape == (counts[t],)
        assert np.array_equal(leaf_of, uh.leaf_of(sa, t))
        assert np.array_equal(lay.prim_perm[t][dev_of], np.arange(counts[t]))  # the inverse, from both sides
        assert np.array_equal(dev_of[lay.prim_perm[t]], np.arange(counts[t]))
        assert lay.prim_perm[t] is getattr(lay.prim_perm, kind)
    order, level_end, slot = update.topology(sa.bvh)
    assert np.array_equal(maps['order'], order) and np.array_equal(maps['level_end'], level_end)
    assert np.array_equal(maps['slot_np'], slot)
    inner = np.nonzero(sa.bvh['bvh_prim_idx'] < 0)[0]
    assert np.array_equal(maps['inner'], inner) and np.array_equal(maps['rows'], slot[inner])
    assert np.array_equal(maps['left'], sa.bvh['bvh_left_child'][inner])
    assert np.array_equal(maps['right'], sa.bvh['bvh_right_child'][inner])


def test_check_edits_raises_every_error_with_its_message():
    sa = ph.fixture('kernel_paths_materials')
    counts = (sa.num_spheres, sa.num_triangles, sa.num_quads)
    widths = {'spheres': (4, 4), 'quads': (16, 9), 'triangles': (12, 9)}

    def bad(kind, message, idx=None, rows=None, build=None):
        good = uh.current(sa, kind, [0, 2])
        arg = tuple(g if v is None else v for g, v in zip(good, (idx, rows, build)))
        with pytest.raises(ValueError, match='^' + re.escape(f'{kind}: {message}') + '$'):
            update.check_edits(counts, **{kind: arg})

    for kind, (nrow, nbuild) in widths.items():
        n = counts[KIND_NAMES[kind]]
        idx, rows, build = uh.current(sa, kind, [0, 2])
        assert rows.shape == (2, nrow) and build.shape == (2, nbuild)
        got = update.check_edits(counts, **{kind: (idx, rows, build)})
        assert list(got) == [KIND_NAMES[kind]]
        for a, b in zip(got[KIND_NAMES[kind]], (idx, rows, build)):
            assert a.tobytes() == b.tobytes() and a.shape == b.shape
        bad(kind, 'indices must be a 1-D integer array', idx=np.array([[0, 2]]))
        bad(kind, 'indices must be a 1-D integer array', idx=np.array([0.0, 2.0]))
        bad(kind, f'an index is outside [0, {n})', idx=np.array([0, n]))
        bad(kind, f'an index is outside [0, {n})', idx=np.array([-1, 2]))
        bad(kind, 'an index is repeated', idx=np.array([2, 2]))
        shape = f'rows must be (n, {nrow}) and build records (n, {nbuild}) f32'
        bad(kind, shape, rows=rows[:, :-1])
        bad(kind, shape, build=build[:1])
        bad(kind, shape, idx=np.array([0, 1, 2]))
        for value in (np.nan, np.inf):
            broken = rows.copy()
            broken[1, -1] = value
            bad(kind, 'rows and build records must be finite', rows=broken)
            broken = build.copy()
            broken[0, 0] = -value
            bad(kind, 'rows and build records must be finite', build=broken)
        moved = build.copy()
        moved[1, 0] = np.nextafter(moved[1, 0], f32(np.inf))
        bad(kind, 'a row and its build record name different points', build=moved)
    # an edit the rows of another kind would fit is a shape error, not a silent swap
    with pytest.raises(ValueError, match=re.escape('quads: rows must be (n, 16)')):
        update.check_edits(counts, quads=uh.current(sa, 'triangles', [0]))
    assert update.check_edits(counts) == {} == update.check_edits(counts, spheres=uh.current(sa, 'spheres', []))


@pytest.mark.parametrize('name,width', HOST_SCENES)
def test_refreshed_mirror_is_pack_device_of_the_refit_arrays(name, width):
    """update.refresh_mirror, given the edits and the ref_nodes the device holds after them, leaves the mirror and
    the layout byte for byte what update_helpers.refit and pack_device of its result give."""
    sa = ph.fixture(name, width)
    edits = {'spheres': uh.sphere_edit([1, 4], sa.sphere_data[[1, 4], 0:3] + f32(0.75), sa.sphere_data[[1, 4], 3]),
             'quads': uh.quad_edit([0, 5], [((1.0, 2.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 5.0)),
                                            ((-2.0, 0.5, 1.0), (0.0, 1.5, 0.0), (0.25, 0.0, 1.0))]),
             'triangles': uh.tri_edit([2], [((0.0, 0.0, 0.0), (9.0, 1.0, 0.0), (0.0, 7.0, 2.0))])}
    want = uh.refit(sa, edits)
    want_lay = sd.pack_device(want)
    mirror, lay = uh.refit(sa), sd.pack_device(sa)  # copies of their own: the refresh writes in place
    assert uh.arrays_equal(mirror, sa) and uh.layouts_equal(lay, want_lay)
    maps = update.index_maps(mirror.bvh, lay.prim_perm, (sa.num_spheres, sa.num_triangles, sa.num_quads))
    checked = update.check_edits((sa.num_spheres, sa.num_triangles, sa.num_quads), **edits)
    assert sorted(checked) == [0, 1, 2]
    update.refresh_mirror(mirror, lay, maps, checked, want_lay.ref_nodes.reshape(-1))
    assert uh.layouts_equal(lay, want_lay) == [] and uh.arrays_equal(mirror, want)
    assert all(np.array_equal(a, b) for a, b in zip(lay.prim_perm, want_lay.prim_perm))
    assert not uh.arrays_equal(sa, want)  # and the fixture was not written


def test_refit_form_by_tree_size():
    txt = header('ptmi_update.h')
    assert int(re.search(r'#define PTMI_UPDATE_ONE_GROUP (\d+)', txt).group(1)) == update.ONE_GROUP
    levels = re.search(r'#define PTMI_UPDATE_ONE_GROUP_MAX_LEVELS (\d+)', txt).group(1)
    assert int(levels) == update.ONE_GROUP_MAX_LEVELS
    assert update.refit_flags(0, 0) == 0 and update.refit_flags(1, 1) == update.ONE_GROUP
    assert update.refit_flags(3407, 15) == update.ONE_GROUP == update.refit_flags(update.ONE_GROUP_MAX_INNER, 64)
    assert update.refit_flags(update.ONE_GROUP_MAX_INNER + 1, 20) == 0 and update.refit_flags(100, 65) == 0


# ------------------------------------------------------------------ update_check
def _records():
    rng = np.random.default_rng(11)
    sph = np.concatenate([rng.uniform(-1e3, 1e3, (200, 4)), rng.normal(0, 1e-3, (50, 4))]).astype(f32)
    sph[:, 3] = np.abs(sph[:, 3])
    sph[0, 3] = 0.0  # a zero-radius sphere
    sph[1] = (5000.0, -0.0, 0.0, 0.0)

    def nine(n, scale):
        return (rng.uniform(-1, 1, (n, 9)) * scale).astype(f32)

    quad = np.concatenate([nine(200, 500.0), nine(50, 1e-4)])
    tri = np.concatenate([nine(200, 500.0), nine(50, 1e-4)])
    for k in range(3):  # axis-aligned: zero extent along k, padded
        quad[10 + k, 3 + k] = quad[10 + k, 6 + k] = 0.0
        tri[10 + k, 3 + k] = tri[10 + k, 6 + k] = tri[10 + k, k]
    # extents exactly 0.0001f, one ulp below and one above: the pad rule's comparison
    d = f32(0.0001)
    for j, e in enumerate((d, np.nextafter(d, f32(0)), np.nextafter(d, f32(1)))):
        quad[20 + j] = (0, 0, 0, e, 0, 0, 0, e, e)
        tri[20 + j] = (0, 0, 0, e, e, 0, 0, 0, e)
        quad[30 + j] = (1, 2, 3, e, 0, 0, 0, e, 0)  # offset: the sums round
        tri[30 + j] = (1, 2, 3, 1 + e, 2, 3, 1, 2 + e, 3)
    boxes = np.sort(rng.uniform(-100, 100, (300, 2, 2, 3)).astype(f32), axis=2).reshape(300, 12)
    boxes[0, 0:3], boxes[0, 6:9] = 0.0, -0.0  # equal under <: the second operand is kept
    boxes[1] = boxes[2]
    return {'sphere': sph, 'quad': quad, 'tri': tri, 'union': boxes}


def _expected(mode, rec):
    if mode == 'union':
        l, r = (rec[:, 0:3], rec[:, 3:6]), (rec[:, 6:9], rec[:, 9:12])
        return np.concatenate(uh.union(*l, *r) + (uh.centre(*l), uh.centre(*r)), axis=1)
    rule = {'sphere': uh.sphere_boxes, 'quad': uh.quad_boxes, 'tri': uh.tri_boxes}[mode]
    return np.concatenate(rule(rec), axis=1)


def _run_check(exe, tmp_path):
    for mode, rec in _records().items():
        src, dst = str(tmp_path / f'{mode}.in'), str(tmp_path / f'{mode}.out')
        rec.tofile(src)
        subprocess.run([exe, mode, src, dst], check=True, timeout=60)
        got = np.fromfile(dst, f32)
        want = _expected(mode, rec).astype(f32)
        assert got.tobytes() == want.tobytes(), mode
    # 250 records of 9 f32 are no whole number of 4-f32 records
    assert subprocess.run([exe, 'sphere', str(tmp_path / 'quad.in'), str(tmp_path / 'x')]).returncode == 2
    assert subprocess.run([exe, 'box', src, dst], capture_output=True).returncode == 2


def test_pad_cases_are_exercised():
    """The records do reach both sides of the pad rule, and the exact-delta extent is not padded."""
    rec = _records()
    for mode, rule in (('quad', uh.quad_boxes), ('tri', uh.tri_boxes)):
        mn, mx = rule(rec[mode])
        ext = mx - mn
        assert (ext[20] == f32(0.0001)).all() and (ext[22] > f32(0.0001)).all()  # kept as they are
        assert np.all(ext > 0) and np.any(ext < f32(0.00011)) and np.any(ext > 1.0)
    mn, mx = uh.sphere_boxes(rec['sphere'])
    assert (mn[0] == mx[0]).all()  # a zero-radius sphere keeps a zero-extent box: spheres are not padded


def test_check_program_equals_numpy(tmp_path):
    exe = str(tmp_path / 'update_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'update_check', f'UPDATE_CHECK={exe}'], check=True)
    _run_check(exe, tmp_path)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same records."""
    exe = str(tmp_path / 'update_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'update_check', f'UPDATE_CHECK={exe}',
                    'UPDATE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    _run_check(exe, tmp_path)


def test_update_records_are_the_compilers_rows():
    """scene_compiler.update_records gives, per primitive, the rows pack_device makes of compile_scene's arrays."""
    from ptmi import bvh, core, scene_compiler as sc
    mat = core.lambertian(core.solid_color(core.vec3(0.5, 0.5, 0.5)))
    s = [core.Sphere.stationary(core.vec3(0.1, 0.2, 0.3), 0.7, mat)]
    q = [core.quad(core.vec3(1, 2, 3), core.vec3(0.3, 0, 0.1), core.vec3(0, 0.7, 0), mat)]
    t = [core.triangle(core.vec3(0, 0, 0.1), core.vec3(1.1, 0, 0), core.vec3(0, 1.3, 0), mat)]
    (sr, sb), (qr, qb), (tr, tb) = sc.update_records(s, q, t)
    world = core.hittable_list()
    for o in s + q + t:
        world.add(o)
    sa = sd.compile_world(world)
    lay = sd.pack_device(sa, leaf_order=False)
    assert sr.tobytes() == lay.spheres.tobytes() == sb.tobytes()
    assert qr.tobytes() == lay.quads.tobytes() and tr.tobytes() == lay.tris.tobytes()
    bs, bq, bt = bvh.primitive_inputs(s, q, t)
    assert qb.tobytes() == bq.tobytes() and tb.tobytes() == bt.tobytes()
    assert qb.tobytes() == qr[:, 4:13].tobytes() and tb[:, 0:3].tobytes() == tr[:, 0:3].tobytes()


def test_kind_table_is_consistent_with_the_compiler_and_the_packer():
    """scene_data.KINDS against what the code makes of one object of each kind: update_records' row and build
    widths, the build columns of a row against the head of its build record, and pack_device's array widths."""
    from ptmi import core, scene_compiler as sc
    mat = core.lambertian(core.solid_color(core.vec3(0.5, 0.5, 0.5)))
    objs = {'spheres': core.Sphere.stationary(core.vec3(0.1, 0.2, 0.3), 0.7, mat),
            'quads': core.quad(core.vec3(1, 2, 3), core.vec3(0.3, 0, 0.1), core.vec3(0, 0.7, 0), mat),
            'triangles': core.triangle(core.vec3(0, 0, 0.1), core.vec3(1.1, 0, 0), core.vec3(0, 1.3, 0), mat)}
    assert [k.code for k in sd.KINDS] == [0, 1, 2] == [sd.PRIM_SPHERE, sd.PRIM_TRIANGLE, sd.PRIM_QUAD]
    assert [k.name for k in sd.KINDS] == list(sd.ByCode._fields) == ['spheres', 'triangles', 'quads']
    assert [k.name for k in sd.STORAGE] == list(objs) and [k.rows for k in sd.STORAGE] == list(sd.ByStorage._fields)
    assert all(k is sd.KINDS[k.code] for k in sd.STORAGE) and len({k.code for k in sd.STORAGE}) == 3
    assert [k.tensor for k in sd.STORAGE] == ['t_spheres', 't_quads', 't_tris']
    assert sc.PRIM_SPHERE is sd.PRIM_SPHERE and (sc.PRIM_TRIANGLE, sc.PRIM_QUAD) == (1, 2)
    world = core.hittable_list()
    for o in objs.values():
        world.add(o)
    sa = sd.compile_world(world)
    lay = sd.pack_device(sa, leaf_order=False)
    records = sc.update_records(*([o] for o in objs.values()))
    for k, (rows, build) in zip(sd.STORAGE, records):
        assert type(objs[k.name]).__name__ == k.class_name
        assert rows.shape == (1, k.row_floats) and build.shape == (1, k.build_floats)
        head = rows[:, k.build_columns]
        assert head.shape[1] in (3, 4, 9) and head.tobytes() == build[:, :head.shape[1]].tobytes()
        assert getattr(lay, k.rows).shape == (1, k.row_floats) and getattr(lay, k.rows).tobytes() == rows.tobytes()
        assert getattr(sa, k.count) == getattr(lay, k.count) == 1 and sa.mats(k.code) is getattr(sa, k.materials)
        geometry = getattr(sa, k.geometry)
        assert geometry is {'spheres': sa.sphere_data, 'quads': sa.quads, 'triangles': sa.tris}[k.name]
        assert update.check_edits((1, 1, 1), **{k.name: ([0], rows, build)})[k.code][1].shape == rows.shape
    assert tuple(sd.mat_bases(sd.ByCode(spheres=9, triangles=5, quads=7))) == (0, 16, 9)  # spheres | quads | triangles
