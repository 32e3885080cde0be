"""GPU tests of the device-build ABI (include/ptmi_build.h):
ptmi_build_sah_device gives the host builder's seven arrays bit for bit on the
inputs of test_build_abi (or PTMI_BUILD_NEEDS_HOST where the issue allows it);
build and pack leave in the tensors a scene already has, at the same addresses,
what pack_device of the rebuilt mirror holds, with the maps of
tree.device_maps; a status other than 0 leaves every tensor untouched and the
wrapper finishes on the host; renders of the rebuilt scene equal the CPU
oracle; and a renderer or viewer rebuilt with builder='device' is byte for byte
the one rebuilt with builder='host'."""
import copy
import ctypes as C

import numpy as np
import pytest

import build_helpers as bh
import parity_helpers as ph
import test_gpu_tree as tg
import tree_helpers as th
import update_helpers as uh
from ptmi import scene_data as sd

pytestmark = pytest.mark.gpu
f32 = np.float32
host = tg.host


# ------------------------------------------------------------------ the builder
def device_build(records, stream=None):
    """ptmi_build_sah_device on builder-form records: (tree dict, status words)."""
    import torch
    from ptmi import build
    s, q, t = (np.ascontiguousarray(a, f32) for a in records)
    counts = sd.ByCode(len(s), len(t), len(q))
    dev = torch.device('cuda', torch.cuda.current_device())
    b = build.DeviceBuilder(counts, dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        b.upload((s, q, t), [np.zeros(c, np.int64) for c in counts])
        b.build(C.c_void_p(st.cuda_stream))
        return b.read_bvh()


@pytest.mark.parametrize('name', list(bh.inputs()))
def test_device_builder_equals_the_host_builder(name):
    got, status = device_build(bh.inputs()[name][:3])
    bh.check_builder_result(name, got, status, (int(status[4]), int(status[5])))
    if bh.inputs()[name][3] != 'plain':  # this builder reproduces every degenerate input of the list
        assert status[0] == 0


def test_device_builder_on_a_side_stream_and_twice_in_one_workspace():
    """Three inputs of the same counts through one DeviceBuilder, so the second and third build find the first's
    workspace and arrays as they were left, on a side stream."""
    import torch
    from ptmi import build
    side = torch.cuda.Stream()
    names = ('vol2_scatter25', 'vol2_scatter100', 'vol2_final_scene')
    s, q, t, _ = bh.inputs()[names[0]]
    b = build.DeviceBuilder(sd.ByCode(len(s), len(t), len(q)), torch.device('cuda', torch.cuda.current_device()))
    with torch.cuda.stream(side):
        for name in names:
            b.upload(bh.inputs()[name][:3], [np.zeros(c, np.int64) for c in b.counts])
            b.build(C.c_void_p(side.cuda_stream))
            got, status = b.read_bvh()
            bh.check_builder_result(name, got, status, (int(status[4]), int(status[5])))
    assert bh.bits_equal(bh.host_tree(names[0]), bh.host_tree(names[1])) != []  # the builds did differ


def test_a_long_fallback_segment_is_handed_back_and_an_empty_input_writes_its_status_only():
    import torch
    from ptmi import _lib, build
    got, status = device_build((bh.needs_host_spheres(), bh.NONE9, bh.NONE9))
    assert status[0] == build.NEEDS_HOST and status[1] == 0 and status[4] == 1
    whole, st = tg.bordered(build.STATUS_WORDS, torch.int32, 777, torch.device('cuda', torch.cuda.current_device()))
    _lib.check(build.load().ptmi_build_sah_device(None, 0, None, 0, None, 0, None, st.data_ptr(), None, 0, None),
               'ptmi_build_sah_device')
    torch.cuda.synchronize()
    assert host(st).tolist() == [0] * build.STATUS_WORDS and tg.borders_intact(whole, build.STATUS_WORDS, 777)


# ------------------------------------------------------------------ build and pack in place
def scene_case(name):
    """(arrays before the edit, update_primitives' edit, the mirror after it) of a pack scene."""
    if name == 'vol2':
        sa = ph.fixture('vol2_final_scene')
        edit = {'spheres': th.scatter(sa, *th.DEPTH_CASE)}
    elif name == 'two':
        sa = th.sphere_arrays(bh.random_spheres(2))
        edit = {'spheres': uh.sphere_edit([0], sa.sphere_data[[1], 0:3] + f32(40.0), [1.5])}
    else:
        sa = ph.fixture(name, 64)
        edit = th.mixed_edit(sa)
    return sa, edit, uh.refit(sa, edit)


@pytest.mark.parametrize('name', ['vol2', 'coverage', 'cornell_mesh_fog', 'two'])
def test_device_rebuild_leaves_the_host_rebuilds_bytes_in_the_same_tensors(name):
    import torch
    from ptmi import tree
    sa, edit, mirror = scene_case(name)
    ds = tg.new_scene(sa)
    ptr0 = tg.pointers(ds)
    ds.update_primitives(**edit)
    # a material edit before the rebuild: it arrives in the permuted mats and, as its class, in the leaf codes
    kind = next(k for k in sd.STORAGE if getattr(sa, k.count))  # a kind the scene has
    lay = sd.pack_device(mirror)
    row = lay.mats[sd.mat_bases(sd.counts_by_code(sa))[kind.code] + np.argsort(lay.prim_perm[kind.code])[0]].copy()
    row.view(np.uint32)[19] = (row.view(np.uint32)[19] & ~np.uint32(0x1ff)) | np.uint32(2)  # a plain dielectric
    ds.update_materials(**{kind.name: (np.array([0]), row[None])})
    mirror = copy.deepcopy(ds.arrays)  # the scene's own mirror is edited in place by the updates below
    old = sd.pack_device(mirror)
    side = torch.cuda.Stream(ds.device) if name == 'coverage' else None  # one case on a side stream
    maps = ds.rebuild(stream=side, builder='device')
    assert ds.last_rebuild == {'builder': 'device', 'reason': 'asked for'}
    want_sa = th.rebuilt(mirror)
    want = tg.assert_scene_is(ds, want_sa)
    assert tg.pointers(ds) == ptr0 and ptr0[0] == ptr0[1]
    assert ds.tree_growth() == (1.0, 1.0)
    for m, w in zip(maps, tree.device_maps(old.prim_perm, want.prim_perm)):
        assert host(m).tobytes() == w.tobytes() and host(m).dtype == np.int32
    if name == 'vol2':
        assert (old.max_leaf_depth, ds.view.max_leaf_depth) == (15, 16)
    new_row = int(np.argsort(want.prim_perm[kind.code])[0])
    codes = want.ref_nodes.view(np.int32)[:, 9]
    mine = codes[(codes < 0) & ((codes >> 28) & 7 == kind.code) & ((codes & 0x1ffffff) == new_row)]
    assert mine.size == 1 and (int(mine[0]) >> 25) & 7 == sd.CLASS_DIELECTRIC
    # a second update through the new maps, and its inverse
    e2 = th.mixed_edit(want_sa, seed=5) if name != 'two' else \
        {'spheres': uh.sphere_edit([1], want_sa.sphere_data[[1], 0:3] + f32(3.0), [2.0])}
    ds.update_primitives(**e2)
    tg.assert_scene_is(ds, uh.refit(want_sa, e2))
    ds.update_primitives(**{k: uh.current(want_sa, k, e[0]) for k, e in e2.items()})
    tg.assert_scene_is(ds, want_sa)
    assert ds.tree_growth() == (1.0, 1.0) and tg.pointers(ds) == ptr0
    # and the host rebuild of the same scene changes nothing
    ds.rebuild()
    assert ds.last_rebuild['builder'] == 'host'
    tg.assert_scene_is(ds, want_sa)


def test_needs_host_leaves_every_tensor_untouched_and_the_wrapper_finishes_on_the_host():
    import torch
    from ptmi import _lib, build
    sa = th.sphere_arrays(bh.needs_host_spheres())
    ds = tg.new_scene(sa)
    ds._update_state()
    n = sa.num_spheres
    # the ABI itself, on bordered copies of the scene's tensors: the pack writes its info and nothing else
    b = build.DeviceBuilder(sd.counts_by_code(ds.layout), ds.device)
    view = _lib.SceneView.from_buffer_copy(ds.view)
    kept = {}
    for field, t in (('nodes', ds.t_nodes), ('ref_nodes', ds.t_ref_nodes), ('spheres', ds.t_spheres),
                     ('mats', ds.t_mats)):
        whole, mid = tg.bordered(t.numel(), t.dtype, 777, ds.device)
        mid.copy_(t)
        kept[field] = (whole, host(whole).copy())
        setattr(view, field, mid.data_ptr())
    b.upload(build.builder_records(sa), ds._upd['dev_of'])
    b.ti[int(b.i_off[10]):].fill_(-5)  # new_row and perm: untouched too
    b.build(None)
    b.pack(view, None)
    _, status, info, new_row, perm = b.read_ints()
    assert status[0] == build.NEEDS_HOST and info[10] == build.PACK_SKIPPED and not info[:10].any()
    assert (new_row[0] == -5).all() and (perm[0] == -5).all()
    for field, (whole, before) in kept.items():
        assert host(whole).tobytes() == before.tobytes(), field
    # the wrapper: the host path, saying so
    ds.rebuild(builder='device')
    assert ds.last_rebuild['builder'] == 'host' and 'NEEDS_HOST' in ds.last_rebuild['reason']
    tg.assert_scene_is(ds, th.rebuilt(sa))
    assert n > build.SORT_MAX


def test_pack_rejects_a_tree_that_is_none_of_the_scene_and_writes_nothing():
    """ptmi_build_pack through the ABI on bordered copies of a scene's tensors, one rule of its check broken at a
    time (build_helpers.rejections): info says REJECTED, every tensor, both maps and all borders are as they were.
    The good tree, packed last into the same copies, is pack_device's."""
    import torch
    from ptmi import _lib, build
    mirror = bh.pack_scenes()['coverage']
    ds = tg.new_scene(mirror)
    ds._update_state()
    old, want = sd.pack_device(mirror), bh.rebuilt_layout(mirror)
    b = build.DeviceBuilder(sd.counts_by_code(ds.layout), ds.device)
    view = _lib.SceneView.from_buffer_copy(ds.view)
    kept = {}
    for field, t in (('nodes', ds.t_nodes), ('ref_nodes', ds.t_ref_nodes), ('spheres', ds.t_spheres),
                     ('quads', ds.t_quads), ('tris', ds.t_tris), ('mats', ds.t_mats)):
        whole, mid = tg.bordered(t.numel(), t.dtype, 777, ds.device)
        mid.copy_(t)
        kept[field] = (whole, mid, host(whole).copy())
        setattr(view, field, mid.data_ptr())
    records = build.builder_records(mirror)
    arrays = dict(left=0, right=1, parent=2, prim_type=3, prim_idx=4)  # DeviceBuilder's int words, in this order
    tree = th.rebuilt(mirror).bvh
    a = int(b.i_off[10])
    for name, (poke, old_row) in bh.rejections(old, tree).items():
        b.upload(records, old_row)
        b.ti[a:].fill_(-5)  # new_row and perm
        b.build(None)
        for array, node, value in poke:
            b.ti[int(b.i_off[arrays[array]]) + node] = value
        b.pack(view, None)
        _, status, info, new_row, perm = b.read_ints()
        assert status[0] == 0 and info.tolist() == [0] * 10 + [build.PACK_REJECTED, 0], name
        assert all((m == -5).all() for m in tuple(new_row) + tuple(perm)), name
        for field, (whole, _, before) in kept.items():
            assert host(whole).tobytes() == before.tobytes(), (name, field)
    b.upload(records, bh.old_rows(old))
    b.build(None)
    b.pack(view, None)
    _, status, info, new_row, perm = b.read_ints()
    got = {field: host(mid) for field, (_, mid, _) in kept.items()}
    got.update(info=info, new_row=new_row, perm=perm)
    assert bh.pack_differences(got, old, want) == []
    for field, (whole, mid, _) in kept.items():
        assert tg.borders_intact(whole, mid.numel(), 777), field


def test_one_primitive_more_than_the_cap_takes_the_host_path_without_a_launch(monkeypatch):
    from ptmi import build
    sa = th.sphere_arrays(bh.random_spheres(build.MAX_PRIMS + 1))
    ds = tg.new_scene(sa)

    def no_build_call():
        raise AssertionError('a scene above the cap reached the device builder')

    monkeypatch.setattr(build, 'load', no_build_call)
    ds.rebuild(builder='device')
    monkeypatch.undo()
    assert ds.last_rebuild['builder'] == 'host' and str(build.MAX_PRIMS) in ds.last_rebuild['reason']
    assert ds._builder is None
    tg.assert_scene_is(ds, sa)


# ------------------------------------------------------------------ rendering
@pytest.mark.parametrize('name', ['vol2_final_scene', 'coverage'])
def test_render_parity_after_the_device_rebuild(name):
    sa, cam, bg = ph.scene_inputs(name, 64)
    edit = {'spheres': th.scatter(sa, *th.DEPTH_CASE)}
    ds = tg.new_scene(sa)
    ds.update_primitives(**edit)
    ds.rebuild(builder='device')
    assert ds.last_rebuild['builder'] == 'device'
    want_sa = th.rebuilt(uh.refit(sa, edit))
    tg.assert_scene_is(ds, want_sa)
    tg.assert_parity(ds, want_sa, cam, bg, tg.COMBOS)


# ------------------------------------------------------------------ the renderer and the viewer
def test_renderers_rebuilt_on_the_host_and_on_the_device_are_byte_equal(tmp_path):
    a, b = tg._renderer(tmp_path, 'a'), tg._renderer(tmp_path, 'b')
    for r in (a, b):
        r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    fa = a.update_primitives(**tg._move(a), keep_history=True, rebuild=True, builder='host', max_history=16)
    fb = b.update_primitives(**tg._move(b), keep_history=True, rebuild=True, builder='device', max_history=16)
    assert a.dscene.last_rebuild['builder'] == 'host' and b.dscene.last_rebuild['builder'] == 'device'
    assert (a.bvh_rebuilds, a.scene_revision) == (b.bvh_rebuilds, b.scene_revision) == (1, 2)
    assert fa == fb and 0.5 < fa <= 1.0
    for x, y in zip(a.guides_ids(), b.guides_ids()):
        assert host(x).tobytes() == host(y).tobytes()
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    assert uh.layouts_equal(a.dscene.layout, b.dscene.layout) == [] and uh.arrays_equal(a.arrays, b.arrays)
    # the next frames of the loop: the primitives go back, new samples, rebuild_bvh on its own
    for r, builder in ((a, 'host'), (b, 'device')):
        r.integrator.render_mk_stats(r.frame, r.accum, r.stats, r.current_sample, 2)
        r.current_sample += 2
        r.rebuild_bvh(keep_history=True, builder=builder, max_history=16)
    assert b.dscene.last_rebuild['builder'] == 'device' and a.bvh_rebuilds == b.bvh_rebuilds == 2
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    assert ph.compare(tg._render_image(b), tg._oracle_image(b), 8) == (0.0, 1.0)
    with pytest.raises(ValueError, match='builder'):
        b.rebuild_bvh(builder='gpu')


def test_motion_viewers_rebuilt_on_the_host_and_on_the_device_are_byte_equal(tmp_path):
    kw = dict(temporal=True, motion=True, max_history=8)
    a, b = tg._renderer(tmp_path, 'va', **kw), tg._renderer(tmp_path, 'vb', **kw)
    for v in (a, b):
        v.render_interactive()
    a.update_primitives(**tg._move(a), rebuild=True)
    b.update_primitives(**tg._move(b), rebuild=True, builder='device')
    assert b.dscene.last_rebuild['builder'] == 'device' and a.bvh_rebuilds == b.bvh_rebuilds == 1
    assert a.history_fraction == b.history_fraction > 0.5
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    a.rebuild_bvh()
    b.rebuild_bvh(builder='device')
    assert a.history_fraction == b.history_fraction
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    for x, y in zip(a.guides_ids(), b.guides_ids()):
        assert host(x).tobytes() == host(y).tobytes()


def test_default_arguments_make_no_build_call(tmp_path, monkeypatch):
    from ptmi import build
    r = tg._renderer(tmp_path, 'd')

    def no_build_call():
        raise AssertionError('a default rebuild made a ptmi_build_* call')

    monkeypatch.setattr(build, 'load', no_build_call)
    r.update_primitives(**tg._move(r), rebuild=True)
    r.rebuild_bvh()
    r.dscene.rebuild()
    monkeypatch.undo()
    assert r.dscene.last_rebuild == {'builder': 'host', 'reason': 'asked for'} and r.dscene._builder is None
    assert r.bvh_rebuilds == 2
