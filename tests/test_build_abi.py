"""CPU tests of the device-build ABI (include/ptmi_build.h): its symbols are in
the library and in ptmi.build's own table and in none of the other ten; every
rejected argument returns PTMI_EINVAL or PTMI_ECAPACITY with its message before
a HIP call (no device is needed: the pointers are never dereferenced); the
workspace size is 0 past the cap and non-decreasing below it; and the per-lane
phases the kernels call, run on the CPU in the kernels' order by
csrc/build_check.cpp, give the host builder's seven arrays and pack_device's
buffers and maps bit for bit, also under the sanitizers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_helpers as bh
from ptmi import (_lib, build, guide, material, motion, post, scene_data as sd, temporal, tree, update, validate,
                  wf_tiles)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h', 'ptmi_tree.h', 'ptmi_validate.h', 'ptmi_material.h')
NAMES = {'ptmi_build_workspace_bytes', 'ptmi_build_sah_device', 'ptmi_build_pack'}


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbols_are_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_build.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error', 'ptmi_bvh_build_sah'}
    assert syms == NAMES == set(build.EXPORTS) == set(build.SIGNATURES)
    lib = build.load()
    assert all(hasattr(lib, s) for s in NAMES)

    def macro(name):
        return int(re.search(rf'#define {name} (\d+)', txt).group(1))

    assert macro('PTMI_BUILD_VERSION') == build.BUILD_VERSION == 1
    assert macro('PTMI_BUILD_MAX_PRIMS') == build.MAX_PRIMS >= 4096
    assert macro('PTMI_BUILD_LANES') == build.LANES and macro('PTMI_BUILD_SORT_MAX') == build.SORT_MAX
    assert macro('PTMI_BUILD_STATUS_WORDS') == build.STATUS_WORDS and macro('PTMI_BUILD_INFO_WORDS') == build.INFO_WORDS
    assert macro('PTMI_BUILD_NEEDS_HOST') == build.NEEDS_HOST
    others = (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES, wf_tiles.SIGNATURES,
              update.SIGNATURES, motion.SIGNATURES, tree.SIGNATURES, validate.SIGNATURES, material.SIGNATURES)
    assert len(others) == 10 and not any(NAMES & set(o) for o in others)
    for other in OTHER_HEADERS:
        assert not any(word in header(other) for word in ('ptmi_build_', 'PTMI_BUILD'))
    assert [len(build.SIGNATURES[s][1]) for s in ('ptmi_build_workspace_bytes', 'ptmi_build_sah_device',
                                                  'ptmi_build_pack')] == [1, 11, 10]
    assert C.sizeof(build.BuildArrays) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(build.BuildMaps) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in build.BuildMaps._fields_] == ['spheres', 'triangles', 'quads']  # type-code order


def test_workspace_bytes_is_zero_past_the_cap_and_non_decreasing_below():
    sizes = [build.workspace_bytes(n) for n in range(0, build.MAX_PRIMS + 1, 7)] + [build.workspace_bytes(build.MAX_PRIMS)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0 and sizes[-1] % 16 == 0
    assert build.workspace_bytes(build.MAX_PRIMS + 1) == 0 and build.workspace_bytes(-1) == 0
    assert build.workspace_bytes(1 << 30) == 0


def arrays(**bad):
    vals = {k: 4096 * (j + 1) for j, (k, _) in enumerate(build.BuildArrays._fields_)}
    vals.update(bad)
    return build.BuildArrays(**vals)


def test_builder_rejects_bad_arguments_before_touching_device():
    lib = build.load()
    E, CAP = _lib.PTMI_EINVAL, _lib.PTMI_ECAPACITY
    big = build.workspace_bytes(build.MAX_PRIMS)

    def call(sph=1 << 20, ns=5, quads=2 << 20, nq=3, tris=3 << 20, nt=2, out=None, status=64, ws=1 << 24, ws_bytes=big,
             null_out=False):
        out = arrays() if out is None else out
        return lib.ptmi_build_sah_device(sph, ns, quads, nq, tris, nt, None if null_out else C.byref(out), status, ws,
                                         ws_bytes, None)

    for neg in ({'ns': -1}, {'nq': -2}, {'nt': -3}):
        assert call(**neg) == E and 'build_sah_device: a count is negative' in err()
    assert call(sph=None) == E and 'spheres NULL/misaligned' in err()
    assert call(sph=(1 << 20) + 2) == E and 'spheres NULL/misaligned' in err()
    assert call(quads=None) == E and 'quads NULL/misaligned' in err()
    assert call(tris=None) == E and 'tris NULL/misaligned' in err()
    assert call(tris=(3 << 20) + 1) == E and 'tris NULL/misaligned' in err()
    assert call(status=None) == E and 'status NULL/misaligned' in err()
    assert call(status=66) == E and 'status NULL/misaligned' in err()
    assert call(ns=build.MAX_PRIMS - 4) == CAP and f'at most {build.MAX_PRIMS}' in err()  # MAX_PRIMS + 1 with nq, nt
    assert call(ns=build.MAX_PRIMS + 1, nq=0, nt=0) == CAP and f'{build.MAX_PRIMS + 1} primitives' in err()
    assert call(ns=1 << 30, nq=1 << 30, nt=1 << 30) == CAP  # the sum does not wrap
    assert call(null_out=True) == E and 'out is NULL' in err()
    for k, _ in build.BuildArrays._fields_:
        assert call(out=arrays(**{k: None})) == E and f'{k} NULL/misaligned' in err()
        assert call(out=arrays(**{k: 4098})) == E and f'{k} NULL/misaligned' in err()
    assert call(ws=None) == E and 'workspace NULL/misaligned' in err()
    assert call(ws=(1 << 24) + 8) == E and 'workspace NULL/misaligned' in err()
    assert call(ws_bytes=build.workspace_bytes(10) - 1) == E and 'bytes' in err() and 'needed' in err()
    # null record arrays with non-zero counts, one type at a time
    assert call(sph=None, nq=0, nt=0) == E and call(quads=None, ns=0, nt=0) == E and call(tris=None, ns=0, nq=0) == E


def test_pack_rejects_bad_arguments_before_touching_device():
    lib = build.load()
    E, CAP = _lib.PTMI_EINVAL, _lib.PTMI_ECAPACITY
    big = build.workspace_bytes(build.MAX_PRIMS)

    def scene(ns=5, nq=3, nt=2, **ptrs):
        v = _lib.SceneView()
        v.num_spheres, v.num_quads, v.num_triangles = ns, nq, nt
        v.num_bvh_nodes, v.n_inner = max(0, 2 * (ns + nq + nt) - 1), max(0, ns + nq + nt - 1)
        vals = dict(nodes=1 << 16, ref_nodes=2 << 16, mats=3 << 16, spheres=4 << 16, quads=5 << 16, tris=6 << 16)
        vals.update(ptrs)
        for k, p in vals.items():
            setattr(v, k, p)
        return v

    def maps(**bad):
        vals = dict(spheres=1 << 12, triangles=2 << 12, quads=3 << 12)
        vals.update(bad)
        return build.BuildMaps(**vals)

    def call(v=None, built=None, status=64, old=None, new=None, perm=None, info=128, ws=1 << 24, ws_bytes=big,
             null=()):
        v, built = scene() if v is None else v, arrays() if built is None else built
        old, new, perm = (maps() if m is None else m for m in (old, new, perm))

        def ref(name, x):
            return None if name in null else C.byref(x)
        return lib.ptmi_build_pack(ref('scene', v), ref('built', built), status, ref('old', old), ref('new', new),
                                   ref('perm', perm), info, ws, ws_bytes, None)

    assert call(null=('scene',)) == E and 'build_pack: scene is NULL' in err()
    assert call(null=('built',)) == E and 'built is NULL' in err()
    for name in ('old', 'new', 'perm'):
        assert call(null=(name,)) == E and 'a map struct is NULL' in err()
    assert call(v=scene(ns=-1)) == E and 'a count is negative' in err()
    assert call(status=None) == E and 'status NULL/misaligned' in err()
    assert call(info=None) == E and 'info NULL/misaligned' in err()
    assert call(info=130) == E and 'info NULL/misaligned' in err()
    assert call(v=scene(ns=build.MAX_PRIMS - 4)) == CAP and f'at most {build.MAX_PRIMS}' in err()
    short = scene()
    short.num_bvh_nodes -= 2
    assert call(v=short) == E and "the view's node counts" in err()
    for k in ('nodes', 'ref_nodes', 'mats'):
        assert call(v=scene(**{k: None})) == E and f'{k} NULL/misaligned' in err()
    for k, kind in (('spheres', 'spheres'), ('quads', 'quads'), ('tris', 'triangles')):
        assert call(v=scene(**{k: None})) == E and f'{kind} rows NULL/misaligned' in err()
    for kind in ('spheres', 'triangles', 'quads'):
        assert call(old=maps(**{kind: None})) == E and f'old_row {kind} NULL/misaligned' in err()
        assert call(new=maps(**{kind: 4098})) == E and f'new_row {kind} NULL/misaligned' in err()
        assert call(perm=maps(**{kind: None})) == E and f'perm {kind} NULL/misaligned' in err()
    for k, _ in build.BuildArrays._fields_:
        assert call(built=arrays(**{k: None})) == E and f'{k} NULL/misaligned' in err()
    assert call(ws=None) == E and 'workspace NULL/misaligned' in err()
    assert call(ws_bytes=16) == E and 'needed' in err()
    # nothing to pack: no launch, nothing but the counts, status and info is looked at
    assert call(v=scene(ns=0, nq=0, nt=0, nodes=None, ref_nodes=None, mats=None), ws=None) == _lib.PTMI_OK


# ------------------------------------------------------------------ build_check
def test_inputs_reach_what_they_are_for():
    """The host builder's own view of the inputs: node counts, and depth where the issue names it."""
    ins = bh.inputs()
    assert {k for k, v in ins.items() if v[3] != 'plain'} == {'sah_coincident', 'clusters', 'zeros', 'zeros_reversed',
                                                              'fallback_a', 'fallback_b'}
    for name, (s, q, t, _) in ins.items():
        n = len(s) + len(q) + len(t)
        assert bh.host_tree(name)['num_bvh_nodes'] == 2 * n - 1, name
    assert int(sd.leaf_depths(bh.host_tree('chain70')).max()) == 20  # 21 levels of nodes, the root's among them
    assert len(ins[f'random{build.MAX_PRIMS}'][0]) == build.MAX_PRIMS
    assert len(bh.needs_host_spheres()) > build.SORT_MAX


def _run_all(exe, tmp_path):
    for name, (s, q, t, _) in bh.inputs().items():
        got, status, printed, _ = bh.run_check(exe, str(tmp_path / name), (s, q, t))
        assert list(status[:6]) == [printed[k] for k in ('status', 'n_nodes', 'levels', 'max_leaf_depth', 'fallback_a',
                                                         'fallback_b')]
        bh.check_builder_result(name, got, status, (printed['fallback_a'], printed['fallback_b']))
    # the all-equal and the short distinct-key fallbacks are reproduced, not handed back
    for name in ('sah_coincident', 'clusters', 'zeros', 'zeros_reversed', 'fallback_a', 'fallback_b'):
        assert bh.run_check(exe, str(tmp_path / name), bh.inputs()[name][:3])[1][0] == 0, name
    # a long fallback segment with distinct keys is handed back, and a pack after it writes nothing
    _, status, printed, _ = bh.run_check(exe, str(tmp_path / 'needs'), (bh.needs_host_spheres(), bh.NONE9, bh.NONE9))
    assert status[0] == build.NEEDS_HOST and status[1] == 0 and printed['fallback_a'] == 1
    for name, mirror in bh.pack_scenes().items():
        old, want = sd.pack_device(mirror), bh.rebuilt_layout(mirror)
        _, status, _, pack = bh.run_check(exe, str(tmp_path / ('pack_' + name)), bh.th.builder_records(mirror),
                                          (old, bh.old_rows(old)))
        assert status[0] == 0 and bh.pack_differences(pack, old, want) == [], name
    # an empty input: the status block and nothing else
    _, status, _, _ = bh.run_check(exe, str(tmp_path / 'empty'), (bh.NONE4, bh.NONE9, bh.NONE9))
    assert status.tolist() == [0] * build.STATUS_WORDS


def test_check_program_equals_the_host_builder_and_pack_device(tmp_path):
    _run_all(bh.make_check(tmp_path), tmp_path)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same inputs."""
    _run_all(bh.make_check(tmp_path, sanitized=True), tmp_path)


def test_pack_carries_a_material_edit_into_the_leaf_codes(tmp_path):
    """A material class changed before the rebuild arrives in the permuted mats and in the leaf codes."""
    exe = bh.make_check(tmp_path)
    mirror = bh.with_material_edit(bh.pack_scenes()['vol2'], kind=0, index=7, material_type=2)
    old, want = sd.pack_device(mirror), bh.rebuilt_layout(mirror)
    _, _, _, pack = bh.run_check(exe, str(tmp_path / 'mat'), bh.th.builder_records(mirror), (old, bh.old_rows(old)))
    assert bh.pack_differences(pack, old, want) == []
    row = int(np.argsort(want.prim_perm[0])[7])
    codes = pack['ref_nodes'].view(np.int32).reshape(-1, 12)[:, 9]
    mine = codes[(codes < 0) & ((codes >> 28) & 7 == 0) & ((codes & 0x1ffffff) == row)]
    assert mine.size == 1 and (int(mine[0]) >> 25) & 7 == sd.CLASS_DIELECTRIC


def test_pack_rejects_a_tree_that_is_none_of_the_scene_and_writes_nothing(tmp_path):
    """Every rule of the pack's own check, one broken at a time: info says REJECTED and the tensors and maps
    are as they were (the nodes and ref_nodes the program starts from are zeros, the maps -1)."""
    exe = bh.make_check(tmp_path)
    mirror = bh.pack_scenes()['coverage']
    old = sd.pack_device(mirror)
    records = bh.th.builder_records(mirror)
    tree = bh.th.rebuilt(mirror).bvh
    cases = bh.rejections(old, tree)
    assert len(cases) == 11
    for k, (name, (poke, old_row)) in enumerate(cases.items()):
        _, status, printed, pack = bh.run_check(exe, str(tmp_path / f'reject{k}'), records, (old, old_row), poke)
        assert status[0] == 0 and printed['pack'] == build.PACK_REJECTED, name
        assert pack['info'].tolist() == [0] * 10 + [build.PACK_REJECTED, 0], name
        assert not pack['nodes'].any() and not pack['ref_nodes'].any(), name
        for key in ('spheres', 'tris', 'quads', 'mats'):
            assert pack[key].tobytes() == np.ascontiguousarray(getattr(old, key), np.float32).tobytes(), (name, key)
        assert all((m == -1).all() for m in tuple(pack['new_row']) + tuple(pack['perm'])), name


def test_auto_threshold_of_the_device_builder_is_its_own():
    from ptmi.renderer import MI355XRenderer as R
    assert R._rebuild_threshold('auto', None) == tree.REBUILD_GROWTH == R._rebuild_threshold('auto', None, 'host')
    assert R._rebuild_threshold('auto', 2.5, 'device') == 2.5
    if build.REBUILD_GROWTH_DEVICE is None:
        with pytest.raises(ValueError, match='REBUILD_GROWTH_DEVICE'):
            R._rebuild_threshold('auto', None, 'device')
    else:
        assert R._rebuild_threshold('auto', None, 'device') == build.REBUILD_GROWTH_DEVICE >= 1.0
    with pytest.raises(ValueError, match='builder'):
        R._rebuild_threshold(True, None, 'gpu')
