"""CPU tests of the tree-quality ABI (include/ptmi_tree.h): its symbols are in
the library and in ptmi.tree's own table and in none of the other seven; every
rejected argument returns PTMI_EINVAL with its message before a HIP call (no
device is needed: the pointers are never dereferenced); the arithmetic the
kernels call, run on the CPU in the kernels' order by csrc/tree_check.cpp,
equals the numpy reference (tree_helpers) bit for bit, also under the
sanitizers; the growth figure is exactly 1 on an unmoved, a restored and a
rebuilt tree and above 1 on a scattered one; and the host half of the in-place
rebuild gives the layout a compile of the edited arrays gives."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import parity_helpers as ph
import tree_helpers as th
import update_helpers as uh
from ptmi import _lib, guide, motion, post, scene_data as sd, temporal, tree, update, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
SCENES = [('vol2_final_scene', None), ('coverage', 64), ('cornell_mesh_fog', 64)]
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h')
NAMES = {'ptmi_tree_areas', 'ptmi_tree_growth', 'ptmi_ids_remap'}


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbols_are_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_tree.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == NAMES == set(tree.EXPORTS) == set(tree.SIGNATURES)
    lib = tree.load()
    assert all(hasattr(lib, s) for s in NAMES)
    assert int(re.search(r'#define PTMI_TREE_VERSION (\d+)', txt).group(1)) == tree.TREE_VERSION == 1
    assert int(re.search(r'#define PTMI_TREE_GROWTH_LANES (\d+)', txt).group(1)) == tree.GROWTH_LANES == th.LANES
    others = (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES, wf_tiles.SIGNATURES,
              update.SIGNATURES, motion.SIGNATURES)
    assert len(others) == 7 and not any(NAMES & set(o) for o in others)
    for other in OTHER_HEADERS:
        assert not any(word in header(other) for word in ('ptmi_tree', 'PTMI_TREE', 'ids_remap'))
    assert [len(tree.SIGNATURES[s][1]) for s in ('ptmi_tree_areas', 'ptmi_tree_growth', 'ptmi_ids_remap')] == [3, 4, 8]
    assert C.sizeof(tree.IdsCounts) == 12  # three int32 by value


def test_tree_calls_reject_bad_arguments_before_touching_device():
    lib = tree.load()
    E = _lib.PTMI_EINVAL

    def scene(nb=9, ref=4096):
        v = _lib.SceneView()
        v.num_bvh_nodes, v.ref_nodes = nb, ref
        return v

    def areas(v=None, out=256, null_scene=False):
        v = scene() if v is None else v
        return lib.ptmi_tree_areas(None if null_scene else C.byref(v), out, None)

    def growth(v=None, base=256, out=512, null_scene=False):
        v = scene() if v is None else v
        return lib.ptmi_tree_growth(None if null_scene else C.byref(v), base, out, None)

    assert areas(null_scene=True) == E and 'tree_areas: scene is NULL' in err()
    assert areas(v=scene(nb=-1)) == E and 'tree_areas: num_bvh_nodes is negative' in err()
    assert areas(v=scene(ref=None)) == E and 'tree_areas: ref_nodes NULL/misaligned' in err()
    assert areas(v=scene(ref=4098)) == E and 'tree_areas: ref_nodes NULL/misaligned' in err()
    assert areas(out=None) == E and 'tree_areas: areas NULL/misaligned' in err()
    assert areas(out=258) == E and 'tree_areas: areas NULL/misaligned' in err()
    assert areas(v=scene(nb=0, ref=None), out=None) == _lib.PTMI_OK  # an empty tree: nothing runs, nothing is checked

    assert growth(null_scene=True) == E and 'tree_growth: scene is NULL' in err()
    assert growth(v=scene(nb=-3)) == E and 'tree_growth: num_bvh_nodes is negative' in err()
    assert growth(v=scene(ref=None)) == E and 'tree_growth: ref_nodes NULL/misaligned' in err()
    assert growth(v=scene(ref=4097)) == E and 'tree_growth: ref_nodes NULL/misaligned' in err()
    assert growth(base=None) == E and 'tree_growth: base_areas NULL/misaligned' in err()
    assert growth(base=257) == E and 'tree_growth: base_areas NULL/misaligned' in err()
    assert growth(out=None) == E and 'tree_growth: out NULL/misaligned' in err()
    assert growth(out=514) == E and 'tree_growth: out NULL/misaligned' in err()
    # the empty tree still writes {1, 1, 0, 0}: out is needed whatever the count
    assert growth(v=scene(nb=0, ref=None), base=None, out=None) == E and 'tree_growth: out NULL/misaligned' in err()

    def remap(ids_in=1024, ids_out=2048, n=16, ms=64, mt=128, mq=192, counts=(3, 2, 2)):
        return lib.ptmi_ids_remap(ids_in, ids_out, n, ms, mt, mq, tree.IdsCounts(*counts), None)

    assert remap(n=-1) == E and 'ids_remap: n is negative' in err()
    for bad in ((-1, 2, 2), (3, -2, 2), (3, 2, -7)):
        assert remap(counts=bad) == E and 'ids_remap: a count is negative' in err()
    assert remap(ms=None) == E and 'ids_remap: map_spheres NULL/misaligned' in err()
    assert remap(ms=66) == E and 'ids_remap: map_spheres NULL/misaligned' in err()
    assert remap(mt=None) == E and 'ids_remap: map_tris NULL/misaligned' in err()
    assert remap(mq=None) == E and 'ids_remap: map_quads NULL/misaligned' in err()
    assert remap(mq=193) == E and 'ids_remap: map_quads NULL/misaligned' in err()
    assert remap(n=0, mt=None) == E and 'ids_remap: map_tris' in err()  # a map is checked by its own count
    assert remap(ids_in=None) == E and 'ids_remap: ids_in NULL/misaligned' in err()
    assert remap(ids_in=1026) == E and 'ids_remap: ids_in NULL/misaligned' in err()
    assert remap(ids_out=None) == E and 'ids_remap: ids_out NULL/misaligned' in err()
    assert remap(ids_out=2049) == E and 'ids_remap: ids_out NULL/misaligned' in err()
    assert remap(ids_in=1024, ids_out=1024 + 60) == E and 'overlap without being equal' in err()
    assert remap(ids_in=1024 + 4, ids_out=1024) == E and 'overlap without being equal' in err()
    # nothing to do: no launch; a type without primitives needs no map
    assert remap(n=0, ids_in=None, ids_out=None) == _lib.PTMI_OK
    assert remap(n=0, ms=None, mt=None, mq=None, counts=(0, 0, 0), ids_in=None, ids_out=None) == _lib.PTMI_OK


# ------------------------------------------------------------------ the trees
def _hand_tree(ext):
    """A 3-node tree whose boxes have extents ``ext`` (root) and ext / 1 (leaves), written by hand."""
    rn = np.zeros((3, 12), f32)
    words = rn.view(np.int32)
    rn[0, 4:7] = ext
    rn[1, 4:7] = ext
    rn[2, 0:3], rn[2, 4:7] = 1.0, f32(1.0) + f32(ext)
    words[0, 3], words[0, 7], words[0, 8] = 1, 2, -1
    words[1:, 3] = words[1:, 7] = -1
    return rn


def tree_cases():
    """name -> (ref_nodes now, baseline areas): the fixtures scattered and refitted,
    and the synthetic trees (1 node; 3 nodes; 1023, 1024, 1025 internal nodes
    around the lane stride; a zero-radius pair whose baseline is 0; extents of
    exactly 0.0001f)."""
    out = {}
    for name, width in SCENES:
        sa = ph.fixture(name, width)
        out[name] = (sd.pack_device(uh.refit(sa, {'spheres': th.scatter(sa, 0.25)})).ref_nodes,
                     th.areas(sd.pack_device(sa).ref_nodes))
    for n_inner in (0, 1, 1023, 1024, 1025):
        sa = th.synthetic(n_inner)
        idx = np.arange(sa.num_spheres)[::3]
        moved = uh.refit(sa, {'spheres': uh.sphere_edit(idx, sa.sphere_data[idx, 0:3] * f32(1.5) + f32(7.0),
                                                        sa.sphere_data[idx, 3] * f32(2.0))})
        out[f'synthetic{n_inner}'] = (sd.pack_device(moved).ref_nodes, th.areas(sd.pack_device(sa).ref_nodes))
    sa = th.synthetic(1, zero_radius=True)
    moved = uh.refit(sa, {'spheres': uh.sphere_edit([0, 1], sa.sphere_data[:, 0:3] + f32(1.0), [2.0, 3.0])})
    base = th.areas(sd.pack_device(sa).ref_nodes)
    assert base[1] == 0 and base[2] == 0  # the leaves; the root's box spans the two points
    base[0] = 0.0  # and a root without a baseline: its term is 1 whatever its box is now
    out['zero_radius'] = (sd.pack_device(moved).ref_nodes, base)
    d = f32(0.0001)
    out['delta'] = (_hand_tree(np.full(3, d * f32(3.0), f32)), th.areas(_hand_tree(np.full(3, d, f32))))
    return out


_cases = {}


def cases():
    if not _cases:
        _cases.update(tree_cases())
    return _cases


def test_cases_reach_what_they_are_for():
    c = cases()
    assert [int(th.is_inner(c[f'synthetic{n}'][0]).sum()) for n in (0, 1, 1023, 1024, 1025)] == [0, 1, 1023, 1024, 1025]
    assert c['synthetic0'][0].shape == (1, 12) and c['synthetic1'][0].shape == (3, 12)
    assert th.growth(*c['synthetic0']).tolist() == [1.0, 1.0, 0.0, 0.0]  # no internal node: the mean of nothing is 1
    assert th.growth(*c['zero_radius']).tolist() == [1.0, 1.0, 1.0, 0.0] and th.areas(c['zero_radius'][0])[0] > 0
    ext = _hand_tree(np.full(3, f32(0.0001), f32))
    assert (ext[0, 4:7] - ext[0, 0:3] == f32(0.0001)).all() and c['delta'][1][0] > 0
    g = th.growth(*c['delta'])
    assert 8.9 < g[0] < 9.1 and g[2] == 1  # extents tripled: the area grows ninefold, up to rounding
    for n in (1023, 1024, 1025):
        g = th.growth(*c[f'synthetic{n}'])
        assert g[2] == n and g[1] >= g[0] > 1.0


def _run_check(exe, tmp_path):
    rng = np.random.default_rng(2)
    for name, (now, base) in cases().items():
        ref, bs, dst = (str(tmp_path / f'{name}.{k}') for k in ('ref', 'base', 'out'))
        np.ascontiguousarray(now, f32).tofile(ref)
        np.ascontiguousarray(base, f32).tofile(bs)
        subprocess.run([exe, 'areas', ref, dst], check=True, timeout=60)
        assert np.fromfile(dst, f32).tobytes() == th.areas(now).tobytes(), name
        subprocess.run([exe, 'growth', ref, bs, dst], check=True, timeout=60)
        assert np.fromfile(dst, f32).tobytes() == th.growth(now, base).tobytes(), name
    for counts in ((7, 5, 3), (1000, 0, 2)):
        maps = [rng.permutation(c).astype(np.int32) for c in counts]
        maps[0][1], maps[0][2] = -1, counts[0]  # entries outside [0, count)
        ids = th.hostile_ids(counts, rng)
        paths = [str(tmp_path / f'remap.{k}') for k in ('ids', 's', 't', 'q', 'out')]
        for p, a in zip(paths, [ids] + maps):
            a.tofile(p)
        subprocess.run([exe, 'remap'] + paths, check=True, timeout=60)
        assert np.fromfile(paths[4], np.int32).tobytes() == th.remap(ids, maps).tobytes()
    # 13 words are no whole number of rows; a base of another length; an unknown mode
    np.zeros(13, f32).tofile(str(tmp_path / 'odd'))
    assert subprocess.run([exe, 'areas', str(tmp_path / 'odd'), dst], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'growth', ref, str(tmp_path / 'odd'), dst], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'boxes', ref, dst], capture_output=True).returncode == 2


def test_check_program_equals_numpy(tmp_path):
    exe = str(tmp_path / 'tree_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'tree_check', f'TREE_CHECK={exe}'], check=True)
    _run_check(exe, tmp_path)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same inputs."""
    exe = str(tmp_path / 'tree_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'tree_check', f'TREE_CHECK={exe}',
                    'TREE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    _run_check(exe, tmp_path)


# ------------------------------------------------------------------ properties
def test_growth_is_one_unmoved_above_one_scattered_and_one_again_restored_or_rebuilt():
    sa = ph.fixture('vol2_final_scene')
    ref = sd.pack_device(sa).ref_nodes
    base = th.areas(ref)
    n_inner = int(th.is_inner(ref).sum())
    assert th.growth(ref, base).tolist() == [1.0, 1.0, float(n_inner), 0.0]
    edit = th.scatter(sa, 0.25)
    moved = uh.refit(sa, {'spheres': edit})
    g = th.growth(sd.pack_device(moved).ref_nodes, base)
    assert g[0] > 1.0 and g[1] > g[0] and g[2] == n_inner
    wide = th.growth(sd.pack_device(uh.refit(sa, {'spheres': th.scatter(sa, 1.0)})).ref_nodes, base)
    assert wide[0] > g[0]  # the further the spheres scatter, the larger the figure
    back = uh.refit(moved, {'spheres': uh.current(sa, 'spheres', edit[0])})
    assert th.growth(sd.pack_device(back).ref_nodes, base).tolist() == [1.0, 1.0, float(n_inner), 0.0]
    new_ref = sd.pack_device(th.rebuilt(moved)).ref_nodes
    assert th.growth(new_ref, th.areas(new_ref)).tolist() == [1.0, 1.0, float(n_inner), 0.0]


def test_builder_on_the_arrays_reproduces_the_fixture_tree():
    """build_sah on the arrays' builder-form records is the tree the fixture was compiled with."""
    sa = ph.fixture('vol2_final_scene')
    assert uh.arrays_equal(th.rebuilt(sa), sa)


@pytest.mark.parametrize('frac,seed', [(0.01, 1), th.DEPTH_CASE])
def test_rebuilt_mirror_packs_to_the_layout_of_a_compile_of_the_edited_arrays(frac, seed):
    """The CPU half of DeviceScene.rebuild: the refit mirror, given the builder's
    new tree, packs to what a scene compiled from the edited geometry packs to
    (its boxes never saw a refit), and the new leaf order is another one."""
    sa = ph.fixture('vol2_final_scene')
    edit = th.scatter(sa, frac, seed)
    mirror = uh.refit(sa, {'spheres': edit})  # what the device and the mirror hold after update_primitives
    spheres = sa.sphere_data.copy()
    spheres[edit[0]] = edit[1]
    edited = dataclasses.replace(sa, sphere_data=spheres, bvh=None)  # a compile knows the geometry only
    lay_rebuilt, lay_compiled = sd.pack_device(th.rebuilt(mirror)), sd.pack_device(th.rebuilt(edited))
    assert uh.layouts_equal(lay_rebuilt, lay_compiled) == []
    assert all(np.array_equal(a, b) for a, b in zip(lay_rebuilt.prim_perm, lay_compiled.prim_perm))
    old = sd.pack_device(mirror)
    assert 'nodes' in uh.layouts_equal(lay_rebuilt, old)
    maps = tree.device_maps(old.prim_perm, lay_rebuilt.prim_perm)
    assert [m.dtype for m in maps] == [np.int32] * 3 and [len(m) for m in maps] == [sa.num_spheres, sa.num_triangles,
                                                                                    sa.num_quads]
    assert not np.array_equal(maps[0], np.arange(sa.num_spheres))  # not the identity: the scatter reorders the leaves
    assert np.array_equal(np.sort(maps[0]), np.arange(sa.num_spheres))
    # the map sends every old device row to the new row of the same primitive
    assert old.spheres.tobytes() == lay_rebuilt.spheres[maps[0]].tobytes()
    assert old.quads.tobytes() == lay_rebuilt.quads[maps[2]].tobytes()
    if (frac, seed) == th.DEPTH_CASE:  # the rendering test's case: the rebuilt tree has another leaf depth
        assert (old.max_leaf_depth, lay_rebuilt.max_leaf_depth) == (15, 16)


@pytest.mark.parametrize('name,width', [('kernel_paths_materials', None), ('coverage', 64)])
def test_index_maps_of_a_rebuilt_tree_follow_the_row_maps(name, width):
    """The numpy half of DeviceScene.rebuild on scenes whose three counts differ: the index maps made anew for
    the rebuilt tree agree with the reference and invert its prim_perm per kind, and device_maps, by field name,
    carries every old device row to the new row of the same reference primitive."""
    sa = ph.fixture(name, width)
    counts = (sa.num_spheres, sa.num_triangles, sa.num_quads)
    mirror = uh.refit(sa, th.mixed_edit(sa))
    new_sa = th.rebuilt(mirror)
    old, new = sd.pack_device(mirror), sd.pack_device(new_sa)
    before = update.index_maps(mirror.bvh, old.prim_perm, counts)
    after = update.index_maps(new_sa.bvh, new.prim_perm, counts)
    maps = tree.device_maps(old.prim_perm, new.prim_perm)
    assert maps._fields == ('spheres', 'triangles', 'quads') == old.prim_perm._fields
    assert [m.shape for m in maps] == [(c,) for c in counts] and {m.dtype for m in maps} == {np.dtype(np.int32)}
    for t, (kind, old_rows, new_rows) in enumerate((('spheres', old.spheres, new.spheres),
                                                    ('triangles', old.tris, new.tris),
                                                    ('quads', old.quads, new.quads))):
        m = getattr(maps, kind)
        assert m is maps[t] and np.array_equal(np.sort(m), np.arange(counts[t]))
        assert np.array_equal(after['leaf_of'][t], uh.leaf_of(new_sa, t))
        assert np.array_equal(new.prim_perm[t][after['dev_of'][t]], np.arange(counts[t]))
        assert np.array_equal(after['dev_of'][t], m[before['dev_of'][t]])  # reference index -> old row -> new row
        assert old_rows.tobytes() == new_rows[m].tobytes()
    assert any(not np.array_equal(m, np.arange(len(m))) for m in maps)  # the edit did reorder some leaves


def test_ids_remap_reference_on_hostile_ids():
    maps = [np.array([2, 0, 1, -1, 5], np.int32), np.array([1, 0], np.int32), np.zeros(0, np.int32)]
    S, T, Q = 0, 1 << 28, 2 << 28
    ids = np.array([-1, -7, S | 0, S | 1, S | 2, S | 3, S | 4, S | 5, T | 0, T | 1, T | 2, Q | 0, 3 << 28, 4 << 28 | 1,
                    5 << 28, 6 << 28, 7 << 28 | 1, -(1 << 31)], np.int64).astype(np.int32)
    want = [-1, -1, S | 2, S | 0, S | 1, -1, -1, -1, T | 1, T | 0, -1, -1, -1, -1, -1, -1, -1, -1]
    #       negative    the map         -1  =count  prim=count      prim=count  no quads  types 3 .. 7       sign bit
    assert th.remap(ids, maps).tolist() == want
    assert th.remap(ids.reshape(3, 6), maps).shape == (3, 6)
    rng = np.random.default_rng(4)
    hostile = th.hostile_ids((5, 2, 0), rng)
    got = th.remap(hostile, maps)
    assert set(np.unique(got >> 28).tolist()) <= {-1, 0, 1} and (got[hostile < 0] == -1).all()
