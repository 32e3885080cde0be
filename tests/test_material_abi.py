"""CPU tests of the material-edit ABI (include/ptmi_material.h): its symbol is in
the library and in ptmi.material's own table and in none of the other nine;
every rejected argument returns PTMI_EINVAL with its message before a HIP call
(no device is needed: the pointers are never dereferenced); the integer rules
the kernel calls, run on the CPU by csrc/material_check.cpp, equal
scene_data.material_class and scene_data.leaf_code, also under the sanitizers;
check_edits refuses what the device call must never see; and the numpy halves
(material_helpers.apply, material.refresh_mirror) agree with pack_device and
undo themselves byte for byte."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import material_helpers as mh
import parity_helpers as ph
import update_helpers as uh
from ptmi import _lib, guide, material, motion, post, scene_data as sd, temporal, tree, update, validate, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h', 'ptmi_tree.h', 'ptmi_validate.h')
NAMES = {'ptmi_update_materials'}


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_material.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == NAMES == set(material.EXPORTS) == set(material.SIGNATURES)
    lib = material.load()
    assert all(hasattr(lib, s) for s in NAMES)
    assert int(re.search(r'#define PTMI_MATERIAL_VERSION (\d+)', txt).group(1)) == material.MATERIAL_VERSION == 1
    others = (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES, wf_tiles.SIGNATURES,
              update.SIGNATURES, motion.SIGNATURES, tree.SIGNATURES, validate.SIGNATURES)
    assert len(others) == 9 and not any(NAMES & set(o) for o in others)
    for other in OTHER_HEADERS:
        assert not any(word in header(other) for word in ('ptmi_material', 'PTMI_MATERIAL', 'update_materials'))
    assert int(re.search(r'#define PTMI_ABI_VERSION (\d+)', header('ptmi.h')).group(1)) == _lib.ABI_VERSION == 9
    assert len(material.SIGNATURES['ptmi_update_materials'][1]) == 6
    assert C.sizeof(material.MaterialList) == 32  # three pointers, an int32, padding
    stress = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libptmi_stress.so')
    assert hasattr(C.CDLL(stress), 'ptmi_update_materials')  # the stress build links the shipped object


def test_update_materials_rejects_bad_arguments_before_touching_device():
    lib = material.load()
    E = _lib.PTMI_EINVAL

    def scene(ns=6, nq=4, nt=2, n_inner=11, nodes=1 << 20, mats=2 << 20, ref=3 << 20):
        v = _lib.SceneView()
        v.num_spheres, v.num_quads, v.num_triangles, v.n_inner = ns, nq, nt, n_inner
        v.num_bvh_nodes = 2 * n_inner + 1 if ns + nq + nt else 0
        v.nodes, v.mats, v.ref_nodes = nodes, mats, ref
        return v

    def lst(count=1, prim=4096, leaf=8192, row=16384):
        return material.MaterialList(prim, leaf, row, count)

    def call(v=None, s=None, q=None, t=None, slot=4 << 20, null_scene=False):
        v = scene() if v is None else v
        by = [C.byref(x) if x is not None else None for x in (s, q, t)]
        return lib.ptmi_update_materials(None if null_scene else C.byref(v), by[0], by[1], by[2], slot, None)

    assert call(null_scene=True, s=lst()) == E and 'materials: scene is NULL' in err()
    for key, name, cap in (('s', 'sphere', 'num_spheres'), ('q', 'quad', 'num_quads'), ('t', 'triangle', 'num_triangles')):
        assert call(**{key: lst(-1)}) == E and f'materials: {name} count negative or above {cap}' in err()
        assert call(**{key: lst(7)}) == E and f'materials: {name} count negative or above {cap}' in err()
        for field in ('prim', 'leaf', 'row'):
            assert call(**{key: lst(**{field: None})}) == E and f'materials: a {name} list pointer' in err()
            assert call(**{key: lst(**{field: 4098})}) == E and f'materials: a {name} list pointer' in err()
        assert call(**{key: lst(0, None, None, None)}) == _lib.PTMI_OK  # an empty list is not looked at
    assert call(v=scene(mats=None), s=lst()) == E and 'materials: mats NULL/misaligned' in err()
    assert call(v=scene(mats=(2 << 20) + 2), q=lst()) == E and 'materials: mats NULL/misaligned' in err()
    assert call(v=scene(ref=None), t=lst()) == E and 'materials: ref_nodes NULL/misaligned' in err()
    assert call(v=scene(nodes=None), s=lst()) == E and 'materials: nodes NULL/misaligned' in err()
    assert call(s=lst(), slot=None) == E and 'materials: slot NULL/misaligned' in err()
    assert call(s=lst(), slot=(4 << 20) + 1) == E and 'materials: slot NULL/misaligned' in err()
    # all counts zero: a no-op, whatever else is NULL
    assert call(v=scene(nodes=None, mats=None, ref=None), slot=None) == _lib.PTMI_OK
    assert call(v=scene(nodes=None, mats=None, ref=None), s=lst(0), q=lst(0), t=lst(0), slot=None) == _lib.PTMI_OK
    assert call(v=scene(0, 0, 0, 0, None, None, None), slot=None) == _lib.PTMI_OK


# ------------------------------------------------------------------ the check program
def _words(path, a, dtype=np.uint32):
    np.ascontiguousarray(a, dtype).tofile(path)
    return path


def _run_check(exe, tmp_path):
    p = {k: str(tmp_path / k) for k in ('a', 'b', 'c', 'out')}
    # every material type x texture type x medium bit, and again with an image index and the unused bits set:
    # the class reads bits 0 - 8 only
    low = np.array([mt | tt << 4 | med << 8 for med in (0, 1) for tt in range(16) for mt in range(16)], np.uint32)
    assert low.size == 16 * 16 * 2
    for high in (0, 3 << 16, 0xffff << 16, 0xfe00):
        flags = low | np.uint32(high)
        subprocess.run([exe, 'classes', _words(p['a'], flags), p['out']], check=True, timeout=60)
        got = np.fromfile(p['out'], np.uint32)
        assert np.array_equal(got, sd.material_class(flags)), hex(high)
        assert np.array_equal(got, sd.material_class(low))
    assert set(sd.material_class(low).tolist()) == set(range(6))
    # the code patch: all three types, every old and new class, the first and the last primitive index
    cases = [(t, prim, old, new) for t in range(3) for prim in (0, 1, (1 << 25) - 1) for old in range(6)
             for new in range(6)]
    codes = np.array([sd.leaf_code(t, prim, old) for t, prim, old, _ in cases], np.int32)
    want = np.array([sd.leaf_code(t, prim, new) for t, prim, _, new in cases], np.int32)
    subprocess.run([exe, 'patch', _words(p['a'], codes, np.int32), _words(p['b'], [c[3] for c in cases]), p['out']],
                   check=True, timeout=60)
    got = np.fromfile(p['out'], np.int32)
    assert got.tobytes() == want.tobytes() == material.patch_codes(codes, [c[3] for c in cases]).tobytes()
    assert ((got ^ codes) & ~np.int32(7 << 25) == 0).all()  # nothing but the class bits changed
    # does a code name a primitive: the type, the index, an internal node's 0 and a word without the leaf flag
    names = [(sd.leaf_code(t, prim, cls), t2, prim2) for t in range(3) for cls in (0, 5) for prim in (0, 7, (1 << 25) - 1)
             for t2 in range(3) for prim2 in (prim, prim ^ 1)]
    names += [(0, 0, 0), (7, 0, 7), (np.int32(sd.leaf_code(1, 3)) & 0x7fffffff, 1, 3), (sd.leaf_code(2, 3), 2, -1)]
    subprocess.run([exe, 'names', _words(p['a'], [c[0] for c in names], np.int32),
                    _words(p['b'], [c[1] for c in names], np.int32), _words(p['c'], [c[2] for c in names], np.int32),
                    p['out']], check=True, timeout=60)
    ref = []
    for code, t, prim in names:
        w = int(np.int32(code)) & 0xffffffff
        ref.append(int(w >> 31 == 1 and (w >> 28) & 7 == t and (w & 0x1ffffff) == prim and prim >= 0))
    got = np.fromfile(p['out'], np.uint32).tolist()
    assert got == ref and 0 < sum(ref) < len(ref)
    # the image bound: image index + 1 against num_images
    flags = np.array([(img + 1) << 16 | 2 << 4 for img in (-1, 0, 1, 2, 15, 16, 0xfffe)], np.uint32)
    for num_images, ok in ((0, [1, 0, 0, 0, 0, 0, 0]), (2, [1, 1, 1, 0, 0, 0, 0]), (16, [1, 1, 1, 1, 1, 0, 0])):
        subprocess.run([exe, 'images', _words(p['a'], flags), str(num_images), p['out']], check=True, timeout=60)
        assert np.fromfile(p['out'], np.uint32).tolist() == ok
    # inputs of different lengths; an unknown mode; a file that is no whole number of words
    assert subprocess.run([exe, 'patch', _words(p['a'], [1, 2]), _words(p['b'], [1]), p['out']],
                          capture_output=True).returncode == 2
    assert subprocess.run([exe, 'rows', p['a'], p['out']], capture_output=True).returncode == 2
    with open(p['c'], 'wb') as f:
        f.write(b'12345')
    assert subprocess.run([exe, 'classes', p['c'], p['out']], capture_output=True).returncode == 2


def test_check_program_equals_numpy(tmp_path):
    exe = str(tmp_path / 'material_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'material_check', f'MATERIAL_CHECK={exe}'], check=True)
    _run_check(exe, tmp_path)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same inputs."""
    exe = str(tmp_path / 'material_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'material_check', f'MATERIAL_CHECK={exe}',
                    'MATERIAL_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    _run_check(exe, tmp_path)


# ------------------------------------------------------------------ the numpy halves
def test_check_edits_rejects_what_the_device_must_not_see():
    counts = sd.ByCode(spheres=6, triangles=2, quads=4)
    good = mh.row(mh.METAL, albedo=(.5, .5, .5))
    e = material.check_edits(counts, 1, spheres=([4, 1], np.stack([good, good])), triangles=(np.zeros(0, np.int64), []))
    assert list(e) == [sd.PRIM_SPHERE] and e[0][0].dtype == np.int64 and e[0][1].shape == (2, 20)
    assert material.check_edits(counts, 0) == {}
    nan = good.copy()
    nan[5] = np.nan
    for kw, msg in (({'spheres': ([6], [good])}, 'outside [0, 6)'), ({'quads': ([-1], [good])}, 'outside [0, 4)'),
                    ({'triangles': ([2], [good])}, 'outside [0, 2)'),
                    ({'spheres': ([1, 1], [good, good])}, 'repeated'), ({'spheres': ([1.5], [good])}, 'integer'),
                    ({'spheres': ([[1]], [good])}, '1-D'), ({'spheres': ([1], [good[:19]])}, '(n, 20)'),
                    ({'spheres': ([1, 2], [good])}, '(n, 20)'), ({'quads': ([1], [nan])}, 'finite'),
                    ({'spheres': ([1], [mh.row(mh.LAMBERTIAN, mh.IMAGE, image=1)])}, 'names image 1, the scene has 1'),
                    ({'spheres': ([1], [np.append(good[:19], np.array([1 << 9], np.uint32).view(f32))])}, 'bits 9 - 15')):
        with pytest.raises(ValueError, match=re.escape(msg)):
            material.check_edits(counts, 1, **kw)
    # an image the scene has, and a flags word whose f32 reading is a NaN or a denormal, are fine
    material.check_edits(counts, 1, spheres=([1], [mh.row(mh.LAMBERTIAN, mh.IMAGE, image=0)]))
    material.check_edits(counts, 0xffff, spheres=([1], [mh.row(mh.LAMBERTIAN, mh.IMAGE, image=0x7fc0 - 1)]))


def test_row_layout_of_the_helpers_is_the_packers():
    for name, width in (('vol2_final_scene', None), ('coverage', 64), ('cornell_mesh_fog', 64)):
        sa = ph.fixture(name, width)
        lay = sd.pack_device(sa, leaf_order=False)
        assert np.concatenate([mh.rows_of(sa, k.name) for k in sd.STORAGE]).tobytes() == lay.mats.tobytes()
        for k in sd.STORAGE:
            back = sd.unpack_mats(mh.rows_of(sa, k.name))
            assert set(back) == set(sd.MAT_KEYS)
            assert all(back[key].tobytes() == sa.mats(k.code)[key].tobytes() and back[key].dtype == sa.mats(k.code)[key].dtype
                       for key in sd.MAT_KEYS)
    walk = mh.class_walk(1)
    assert [mh.CLASS[c] for c, _ in walk] == sd.material_class(mh.flags_of(np.stack([r for _, r in walk]))).tolist()
    assert {c for c, _ in walk} == set(mh.CLASS)


@pytest.mark.parametrize('name,width', [('coverage', 64), ('vol2_final_scene', None), ('cornell_mesh_fog', 64)])
def test_apply_then_the_inverse_restores_every_byte_and_the_mirror_follows(name, width):
    """apply() against pack_device, and material.refresh_mirror (the host half of DeviceScene.update_materials)
    against both: after the edit the patched layout is pack_device of the edited arrays, after the inverse it
    is the layout it began as, and the caller's arrays are never written."""
    sa = ph.fixture(name, width)
    lay0 = sd.pack_device(sa)
    edits = mh.walk_edits(sa, offset=1)
    assert mh.classes_of(edits) == set(range(6))
    ref = mh.apply(sa, edits)
    want = sd.pack_device(ref)
    assert set(uh.layouts_equal(want, lay0)) >= {'nodes', 'ref_nodes', 'mats'}
    assert not {'spheres', 'quads', 'tris', 'root_min', 'root_max', 'max_leaf_depth'} & set(uh.layouts_equal(want, lay0))
    assert uh.arrays_equal(ref, sa) and not mh.mats_equal(ref, sa)
    inverse = {k: mh.current(sa, k, e[0]) for k, e in edits.items()}
    back = mh.apply(ref, inverse)
    assert mh.mats_equal(back, sa) and uh.layouts_equal(sd.pack_device(back), lay0) == []
    # the mirror: its own copies, refreshed in place
    mirror = dataclasses.replace(sa, **{k.materials: {key: v.copy() for key, v in sa.mats(k.code).items()}
                                        for k in sd.KINDS})
    lay = sd.pack_device(mirror)
    maps = update.index_maps(sa.bvh, lay.prim_perm, sd.counts_by_code(sa))
    checked = material.check_edits(sd.counts_by_code(sa), len(sa.images), **edits)
    material.refresh_mirror(mirror, lay, maps, checked)
    assert uh.layouts_equal(lay, want) == [] and mh.mats_equal(mirror, ref)
    material.refresh_mirror(mirror, lay, maps, material.check_edits(sd.counts_by_code(sa), len(sa.images), **inverse))
    assert uh.layouts_equal(lay, lay0) == [] and mh.mats_equal(mirror, sa)
    assert mh.mats_equal(sa, ph.fixture(name, width))


def test_mirror_of_a_one_primitive_scene_patches_the_root_ref():
    import random
    from ptmi import core
    random.seed(7)
    w = core.hittable_list()
    w.add(core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))))
    sa = sd.compile_world(w)
    lay = sd.pack_device(sa)
    assert lay.n_inner == 0 and lay.root_ref == int(sd.leaf_code(0, 0, mh.CLASS['lambertian']))
    edits = {'spheres': (np.array([0]), mh.class_walk()[4][1][None])}  # dielectric
    ref = mh.apply(sa, edits)
    mirror = dataclasses.replace(sa, sphere_mats={k: v.copy() for k, v in sa.sphere_mats.items()})
    maps = update.index_maps(sa.bvh, lay.prim_perm, sd.counts_by_code(sa))
    material.refresh_mirror(mirror, lay, maps, material.check_edits(sd.counts_by_code(sa), 0, **edits))
    assert lay.root_ref == int(sd.leaf_code(0, 0, mh.CLASS['dielectric'])) == sd.pack_device(ref).root_ref
    assert uh.layouts_equal(lay, sd.pack_device(ref)) == []
