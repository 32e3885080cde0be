"""GPU tests of the tree-quality ABI and the in-place rebuild (include/ptmi_tree.h,
DESIGN.md §20): the three kernels equal their numpy reference (tree_helpers)
byte for byte; DeviceScene.rebuild leaves in the tensors the scene already had,
at the same addresses, what pack_device of a compile of the edited arrays
holds, and renders from it equal the CPU oracle, counters included; a history
carried across a rebuild equals the one carried across the update alone; and
update_primitives without ``rebuild`` does what it did."""
import ctypes as C
import random

import numpy as np
import pytest

import parity_helpers as ph
import tree_helpers as th
import update_helpers as uh
from ptmi import scene_data as sd

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 12345.0
COMBOS = [('mk', 'stack'), ('mk', 'stackless'), ('wf', 'stack'), ('wf', 'stackless')]
TENSORS = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris', 'mats')


# ------------------------------------------------------------------ helpers
def arrays_of(name):
    if name.startswith('synthetic'):
        return th.synthetic(int(name[len('synthetic'):]))
    return ph.scene_inputs(name, 64)[0]


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def host(t):
    return t.cpu().numpy()


def device_bytes(ds):
    """What the device holds of the six tensors a rebuild writes, in the layout's shapes."""
    lay = ds.layout
    return {k: host(getattr(ds, 't_' + k)).view(f32)[:getattr(lay, k).size].reshape(getattr(lay, k).shape).copy()
            for k in TENSORS}


def pointers(ds):
    v = ds.view
    return ([getattr(ds, 't_' + k).data_ptr() for k in TENSORS + ('texels', 'pvec', 'perm')],
            [v.nodes, v.ref_nodes, v.spheres, v.quads, v.tris, v.mats, v.texels, v.perlin_vec, v.perlin_perm])


def assert_scene_is(ds, expected_sa):
    """Device tensors, view fields, shell hint, layout and mirror all are pack_device(expected_sa)'s."""
    want = sd.pack_device(expected_sa)
    got = device_bytes(ds)
    for k in TENSORS:
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    v = ds.view
    assert (v.root_ref, v.max_leaf_depth, v.shell, v.n_inner, v.num_bvh_nodes) == \
        (want.root_ref, want.max_leaf_depth, want.shell, want.n_inner, want.num_bvh_nodes)
    assert np.array(list(v.root_min) + list(v.root_max), f32).tobytes() == \
        np.concatenate([want.root_min, want.root_max]).astype(f32).tobytes()
    assert uh.layouts_equal(ds.layout, want) == []
    assert all(np.array_equal(a, b) for a, b in zip(ds.layout.prim_perm, want.prim_perm))
    assert uh.arrays_equal(ds.arrays, expected_sa)
    return want


def bordered(n, dtype, fill, dev):
    """A tensor of n elements between two 16-element borders of ``fill``: (whole, the middle)."""
    import torch
    whole = torch.full((n + 32,), fill, dtype=dtype, device=dev)
    return whole, whole[16:16 + n]


def borders_intact(whole, n, fill):
    h = host(whole)
    return (h[:16] == fill).all() and (h[16 + n:] == fill).all()


def render_pair(ds, ref_sa, cam, bg, variant, traversal, spp=8):
    """(gpu accum, gpu counters, oracle accum, oracle counters) of a whole 64-px frame."""
    import oracle
    import torch
    from ptmi import device
    W, H = cam['width'], cam['height']
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, bg, 50, 0, W, H, traversal=traversal)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    (integ.render_mk if variant == 'mk' else integ.render_wf)(fr, acc, 0, spp)
    torch.cuda.synchronize()
    o = np.zeros((H, W, 3), f32)
    ost = oracle.render(oracle.OracleScene(ref_sa), oracle.make_frame(cam, bg, 50, 0, W, H, traversal), variant, o,
                        (0, 0, W, H), 0, spp)
    return host(acc), integ.read_counters(), o, {k: int(v) for k, v in ost.items()}


def assert_parity(ds, ref_sa, cam, bg, combos, spp=8):
    images = {}
    for variant, traversal in combos:
        g, cnt, o, ost = render_pair(ds, ref_sa, cam, bg, variant, traversal, spp)
        linf, exact = ph.compare(g, o, spp)
        assert linf == 0.0 and exact == 1.0, (variant, traversal, linf, exact)
        assert cnt == ost, (variant, traversal)
        assert np.isfinite(g).all() and g.sum() > 0
        images[variant, traversal] = g
    return images


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('name', ['vol2_final_scene', 'coverage', 'cornell_mesh_fog', 'synthetic0', 'synthetic1',
                                  'synthetic1025'])
def test_areas_and_growth_equal_numpy(name):
    import torch
    from ptmi import _lib, tree
    sa = arrays_of(name)
    ds = new_scene(sa)
    lib, dev, n = tree.load(), ds.device, sa.num_bvh_nodes
    side = torch.cuda.Stream(dev)
    ref0 = sd.pack_device(sa).ref_nodes
    whole, areas = bordered(n, torch.float32, SENTINEL, dev)
    _lib.check(lib.ptmi_tree_areas(ds.view, areas.data_ptr(), None), 'ptmi_tree_areas')
    torch.cuda.synchronize()
    assert host(areas).tobytes() == th.areas(ref0).tobytes() and borders_intact(whole, n, SENTINEL)
    assert ds.tree_growth() == (1.0, 1.0)  # takes the baseline
    assert host(ds._tree['base'])[:n].tobytes() == th.areas(ref0).tobytes()
    edit = {'spheres': th.scatter(sa, 0.25)} if sa.num_spheres else {}
    ds.update_primitives(**edit)
    now = sd.pack_device(uh.refit(sa, edit)).ref_nodes
    want = th.growth(now, th.areas(ref0))
    assert want[2] == ds.view.n_inner and (want[0] > 1.0 or not edit or n == 1)
    wout, out = bordered(4, torch.float32, SENTINEL, dev)
    for stream in (None, side):
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        _lib.check(lib.ptmi_tree_growth(ds.view, ds._tree['base'].data_ptr(), out.data_ptr(),
                                        C.c_void_p(stream.cuda_stream) if stream else None), 'ptmi_tree_growth')
        torch.cuda.synchronize()
        assert host(out).tobytes() == want.tobytes() and borders_intact(wout, 4, SENTINEL)
    assert ds.tree_growth() == (float(want[0]), float(want[1])) == ds.tree_growth(stream=side)
    # the areas of the moved tree, on the side stream
    areas.fill_(SENTINEL)
    torch.cuda.synchronize()
    _lib.check(lib.ptmi_tree_areas(ds.view, areas.data_ptr(), C.c_void_p(side.cuda_stream)), 'ptmi_tree_areas')
    side.synchronize()
    assert host(areas).tobytes() == th.areas(now).tobytes() and borders_intact(whole, n, SENTINEL)


def test_growth_of_an_empty_tree_writes_ones():
    import torch
    from ptmi import _lib, tree
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device='cuda')
    _lib.check(tree.load().ptmi_tree_growth(_lib.SceneView(), None, out.data_ptr(), None), 'ptmi_tree_growth')
    torch.cuda.synchronize()
    assert host(out).tolist() == [1.0, 1.0, 0.0, 0.0]


def test_ids_remap_on_hostile_ids_in_place_and_on_a_side_stream():
    """Through ctypes, past the wrapper's checks: every id that names no row of
    its type, or whose map entry names none, becomes -1 and reads nothing beyond
    its map; the maps sit between sentinel borders that would give a valid-looking
    entry if read."""
    import torch
    from ptmi import _lib, tree
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = tree.load()
    rng = np.random.default_rng(9)
    side = torch.cuda.Stream(dev)
    for counts in ((7, 5, 3), (1000, 0, 2)):
        maps = [rng.permutation(c).astype(np.int32) for c in counts]
        maps[0][1], maps[0][2] = -1, counts[0]
        ids = th.hostile_ids(counts, rng)
        want = th.remap(ids, maps)
        assert (want == -1).sum() > 40 and (want >= 0).sum() > 1000
        tmaps = []
        for m in maps:  # a border of zeros: a read past the map would find the valid entry 0
            whole, mid = bordered(len(m), torch.int32, 0, dev)
            mid.copy_(torch.from_numpy(m))
            tmaps.append((whole, mid))
        ptr = [mid.data_ptr() if len(m) else None for (_, mid), m in zip(tmaps, maps)]
        tin = torch.from_numpy(ids).to(dev)
        wout, tout = bordered(ids.size, torch.int32, 777, dev)
        for stream in (None, side):
            tout.fill_(777)
            torch.cuda.synchronize()
            _lib.check(lib.ptmi_ids_remap(tin.data_ptr(), tout.data_ptr(), ids.size, *ptr, tree.IdsCounts(*counts),
                                          C.c_void_p(stream.cuda_stream) if stream else None), 'ptmi_ids_remap')
            torch.cuda.synchronize()
            assert host(tout).tobytes() == want.tobytes() and borders_intact(wout, ids.size, 777)
        assert host(tin).tobytes() == ids.tobytes()
        # in place
        tout.copy_(tin)
        _lib.check(lib.ptmi_ids_remap(tout.data_ptr(), tout.data_ptr(), ids.size, *ptr, tree.IdsCounts(*counts), None),
                   'ptmi_ids_remap')
        torch.cuda.synchronize()
        assert host(tout).tobytes() == want.tobytes() and borders_intact(wout, ids.size, 777)


@pytest.mark.parametrize('name', ['vol2_final_scene', 'coverage', 'cornell_mesh_fog'])
def test_ids_and_rows_of_a_fixture_cross_its_rebuild(name):
    """DeviceScene.remap_ids and permute_rows on a fixture's own id image, rows and
    maps: spheres, triangles and quads are all moved, so the rebuild reorders
    every type the scene has and a map or a count taken for another type's shows."""
    import torch
    from ptmi import device, tree
    sa, cam, bg = ph.scene_inputs(name, 64)
    edits = th.mixed_edit(sa)
    ds = new_scene(sa)
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, bg, 50, 0, cam['width'], cam['height'])
    ds.update_primitives(**edits)
    g0, i0 = integ.trace_guides_ids(fr)
    rows0 = ds.primitive_rows()
    old = sd.pack_device(uh.refit(sa, edits))
    maps = ds.rebuild()
    hm = [host(m) for m in maps]
    want = sd.pack_device(th.rebuilt(uh.refit(sa, edits)))
    counts = (sa.num_spheres, sa.num_triangles, sa.num_quads)
    for m, w, n in zip(hm, tree.device_maps(old.prim_perm, want.prim_perm), counts):
        assert m.tobytes() == w.tobytes() and len(m) == n
        assert n == 0 or not np.array_equal(m, np.arange(n))  # reordered
    ids0 = host(i0)
    seen = set(np.unique(ids0[ids0 >= 0] >> 28).tolist())
    assert seen == {t for t, n in enumerate(counts) if n}  # every type the scene has shows in the image
    got = ds.remap_ids(i0, maps)
    assert host(got).tobytes() == th.remap(ids0, hm).tobytes() and host(i0).tobytes() == ids0.tobytes()
    assert not np.array_equal(host(got), ids0)
    # the retraced ids of the rebuilt scene are those ids: same guides (asserted), same primitives, new rows
    g1, i1 = integ.trace_guides_ids(fr)
    assert host(g1).tobytes() == host(g0).tobytes() and host(i1).tobytes() == host(got).tobytes()
    side = torch.cuda.Stream(ds.device)
    side.wait_stream(torch.cuda.current_stream(ds.device))
    assert ds.remap_ids(i0, maps, out=i0, stream=side) is i0  # in place, on a side stream
    side.synchronize()
    assert host(i0).tobytes() == host(got).tobytes()
    # the rows taken before the rebuild, permuted, are the rows the scene holds now (the geometry did not change)
    new_rows = ds.permute_rows(rows0, maps)
    held = ((ds.t_spheres, want.spheres), (ds.t_quads, want.quads), (ds.t_tris, want.tris))
    for t, (mine, lay_rows) in zip(new_rows, held):
        assert host(t).tobytes() == host(mine).tobytes()
        assert host(t)[:lay_rows.size].tobytes() == lay_rows.tobytes()
    assert any(host(a).tobytes() != host(b).tobytes() for a, b in zip(rows0, new_rows))


# ------------------------------------------------------------------ rebuild in place
@pytest.mark.parametrize('name', ['vol2_final_scene', 'coverage', 'synthetic0'])
def test_rebuild_leaves_the_packed_compile_in_the_same_tensors(name):
    from ptmi import tree
    sa = arrays_of(name)
    edit = {'spheres': th.scatter(sa, 0.25)}
    ds = new_scene(sa)
    ptr0 = pointers(ds)
    ds.update_primitives(**edit)
    refit = uh.refit(sa, edit)
    old = sd.pack_device(refit)
    if name != 'synthetic0':
        assert ds.tree_growth()[0] > 1.0
    maps = ds.rebuild()
    want_sa = th.rebuilt(refit)
    want = assert_scene_is(ds, want_sa)
    assert pointers(ds) == ptr0 and ptr0[0] == ptr0[1]
    assert ds.tree_growth() == (1.0, 1.0)
    for m, w in zip(maps, tree.device_maps(old.prim_perm, want.prim_perm)):
        assert host(m).tobytes() == w.tobytes() and host(m).dtype == np.int32
    if name == 'vol2_final_scene':
        assert not np.array_equal(host(maps[0]), np.arange(sa.num_spheres)) and 'nodes' in uh.layouts_equal(want, old)
    # a second update through the new leaf_of / dev_of: an edit, then its inverse
    idx = np.arange(want_sa.num_spheres)[::2]
    e2 = {'spheres': uh.sphere_edit(idx, want_sa.sphere_data[idx, 0:3] + f32(3.0), want_sa.sphere_data[idx, 3])}
    ds.update_primitives(**e2)
    assert_scene_is(ds, uh.refit(want_sa, e2))
    if name != 'synthetic0':
        assert ds.tree_growth()[0] > 1.0
    ds.update_primitives(spheres=uh.current(want_sa, 'spheres', idx))
    assert_scene_is(ds, want_sa)
    assert ds.tree_growth() == (1.0, 1.0) and pointers(ds) == ptr0
    assert uh.arrays_equal(sa, arrays_of(name))  # the caller's arrays were never written


def test_rebuild_needs_the_arrays_and_a_stream_of_its_device():
    import torch
    from ptmi import _lib
    sa = arrays_of('coverage')
    with pytest.raises(_lib.PtmiError, match='SceneArrays'):
        new_scene(sd.pack_device(sa)).rebuild()
    ds = new_scene(sa)
    ds.rebuild(stream=torch.cuda.Stream(ds.device))  # an unmoved scene: the same tree again
    assert_scene_is(ds, sa)


# ------------------------------------------------------------------ rendering after the rebuild
def test_render_parity_after_the_rebuild_of_coverage():
    sa, cam, bg = ph.scene_inputs('coverage', 64)
    edit = {'spheres': th.scatter(sa, 0.25)}
    ds = new_scene(sa)
    ds.update_primitives(**edit)
    ds.rebuild()
    want_sa = th.rebuilt(uh.refit(sa, edit))
    images = assert_parity(ds, want_sa, cam, bg, COMBOS)
    fresh = new_scene(want_sa)  # a scene made anew from the edited arrays: the same image
    for combo in (('mk', 'stack'), ('wf', 'stackless')):
        assert render_pair(fresh, want_sa, cam, bg, *combo)[0].tobytes() == images[combo].tobytes()


def test_render_parity_when_the_rebuild_changes_the_leaf_depth():
    sa, cam, bg = ph.scene_inputs('vol2_final_scene', 64)
    edit = {'spheres': th.scatter(sa, *th.DEPTH_CASE)}
    ds = new_scene(sa)
    ds.update_primitives(**edit)
    assert ds.view.max_leaf_depth == 15
    ds.rebuild()
    assert ds.view.max_leaf_depth == 16 and ds.view.shell != 0
    want_sa = th.rebuilt(uh.refit(sa, edit))
    assert_scene_is(ds, want_sa)
    images = assert_parity(ds, want_sa, cam, bg, COMBOS)
    fresh = new_scene(want_sa)
    assert render_pair(fresh, want_sa, cam, bg, 'mk', 'stack')[0].tobytes() == images['mk', 'stack'].tobytes()


def test_shell_hint_is_cleared_by_update_and_rebuild_alike():
    """§17's shell case: a sphere moved beyond R / 2 of the shell's centre clears the hint, refit or rebuilt."""
    sa, cam, bg = ph.scene_inputs('vol2_final_scene', 64)
    lay0 = sd.pack_device(sa)
    shell = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, lay0.max_leaf_depth)])
    c, R = sa.sphere_data[shell, 0:3], sa.sphere_data[shell, 3]
    small = next(i for i in range(sa.num_spheres) if i != shell and sa.sphere_data[i, 3] <= 10)
    away = {'spheres': uh.sphere_edit([small], [c + f32(0.6) * R * np.array([0, 1, 0], f32)], [10.0])}
    ds = new_scene(sa)
    assert ds.view.shell == lay0.shell != 0
    ds.update_primitives(**away)
    assert ds.view.shell == 0
    ds.rebuild()
    want_sa = th.rebuilt(uh.refit(sa, away))
    assert ds.view.shell == 0 == sd.pack_device(want_sa).shell
    assert_parity(ds, want_sa, cam, bg, [('mk', 'stack')])
    ds.update_primitives(spheres=uh.current(sa, 'spheres', [small]))  # back inside: the claim holds again
    ds.rebuild()
    assert_scene_is(ds, sa)
    assert ds.view.shell == lay0.shell
    assert_parity(ds, sa, cam, bg, [('mk', 'stack')])


# ------------------------------------------------------------------ the renderer and the viewer
N_BALLS, N_PANELS, N_TRIS = 14, 6, 6


def _shapes(moved=False):
    """(sphere centres, panel quads (Q, u, v), triangles (v0, v1, v2)): three rows
    of small primitives; ``moved``: every other one of each row sent to the far
    end of its row, so that a rebuild reorders the leaves of every type."""
    c = [(-2.6 + 0.4 * k, -0.2 + 0.05 * (k % 3), -1.0 - 0.1 * (k % 4)) for k in range(N_BALLS)]
    q = [((-2.4 + 0.8 * k, 0.9, -2.0 - 0.05 * k), (0.5, 0.0, 0.0), (0.0, 0.4, 0.0)) for k in range(N_PANELS)]
    t = [(-2.4 + 0.8 * k, 1.5, -1.8 - 0.05 * k) for k in range(N_TRIS)]
    if moved:
        c = [(-x + 0.13, y + 0.3, z - 0.2) if k % 2 else (x, y, z) for k, (x, y, z) in enumerate(c)]
        q = [((-Q[0] - 0.43, Q[1] + 0.15, Q[2]), u, v) if k % 2 else (Q, u, v) for k, (Q, u, v) in enumerate(q)]
        t = [(-x - 0.45, y + 0.1, z) if k % 2 else (x, y, z) for k, (x, y, z) in enumerate(t)]
    t = [((x, y, z), (x + 0.5, y, z), (x + 0.25, y + 0.4, z)) for x, y, z in t]
    return c, q, t


def _world(moved=False):
    from ptmi import core
    w = core.hittable_list()
    grey = core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))
    centres, panels, tris = _shapes(moved)
    w.add(core.Sphere.stationary(core.vec3(0, -100.5, -1), 100, grey))
    for k, c in enumerate(centres):
        w.add(core.Sphere.stationary(core.vec3(*c), 0.18, core.lambertian(
            core.solid_color(core.vec3(.2 + .05 * k, .3, .9 - .05 * k)))))
    w.add(core.quad(core.vec3(-4, -0.5, -3), core.vec3(8, 0, 0), core.vec3(0, 4, 0), grey))
    for Q, u, v in panels:
        w.add(core.quad(core.vec3(*Q), core.vec3(*u), core.vec3(*v), grey))
    w.add(core.triangle(core.vec3(-2.5, -0.5, 0.5), core.vec3(-1.5, -0.5, 0.5), core.vec3(-2, 0.5, 0.5), grey))
    for v0, v1, v2 in tris:
        w.add(core.triangle(core.vec3(*v0), core.vec3(*v1), core.vec3(*v2), grey))
    return w


def _camera(width=64):
    from ptmi import core
    cam = core.camera()
    cam.aspect_ratio, cam.img_width, cam.samples_per_pixel, cam.vfov = 1.5, width, 4, 60
    cam.lookfrom, cam.lookat, cam.vup = core.vec3(0, 0.5, 3), core.vec3(0, 0, -1), core.vec3(0, 1, 0)
    cam.defocus_angle = 0.0
    return cam


def _renderer(tmp_path, tag, **kw):
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import MI355XRenderer
    random.seed(4321)
    r = (InteractiveViewer if kw else MI355XRenderer)(_world(), _camera(), str(tmp_path / f'{tag}.png'), **kw)
    r.background_color = (0.7, 0.8, 1.0)
    return r


def _move(r):
    """update_primitives' arguments that take the renderer's world from _world() to _world(moved=True)."""
    from ptmi import core
    P = r.primitives
    centres, panels, tris = _shapes(True)  # index 0 of each list is the ground, the wall, the lone triangle
    return {'spheres': {k + 1: core.Sphere.stationary(core.vec3(*c), 0.18, P['spheres'][k + 1].material)
                        for k, c in enumerate(centres) if k % 2},
            'quads': {k + 1: core.quad(*(core.vec3(*x) for x in q), P['quads'][k + 1].mat)
                      for k, q in enumerate(panels) if k % 2},
            'triangles': {k + 1: core.triangle(*(core.vec3(*x) for x in t), P['triangles'][k + 1].mat)
                          for k, t in enumerate(tris) if k % 2}}


def _current(r):
    """The objects _move replaces, as they are now: the arguments that undo it."""
    return {name: {k: r.primitives[name][k] for k in new} for name, new in _move(r).items()}


def _refit_of(sa, move):
    """update_helpers.refit of ``sa`` by _move's arguments."""
    from ptmi import scene_compiler
    order = {name: sorted(new) for name, new in move.items()}
    records = scene_compiler.update_records(*([move[name][i] for i in order[name]]
                                              for name in ('spheres', 'quads', 'triangles')))
    return uh.refit(sa, {name: (np.asarray(order[name], np.int64), rows, build)
                         for name, (rows, build) in zip(('spheres', 'quads', 'triangles'), records)})


def _oracle_image(r, spp=8):
    import oracle
    W, H = r.cam.img_width, r.cam.img_height
    o = np.zeros((H, W, 3), f32)
    fr = oracle.make_frame(sd.camera_upload(r.cam), r.background_color, 50, r.seed, W, H, 'stack')
    oracle.render(oracle.OracleScene(r.arrays), fr, 'mk', o, (0, 0, W, H), 0, spp)
    return o


def _render_image(r, spp=8):
    import torch
    acc = torch.zeros_like(r.accum)
    r.integrator.render_mk(r.frame, acc, 0, spp)
    torch.cuda.synchronize()
    return host(acc)


def test_history_across_a_rebuild_equals_history_across_the_update(tmp_path):
    from ptmi import tree
    a, b = _renderer(tmp_path, 'a'), _renderer(tmp_path, 'b')
    for r in (a, b):
        r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    ptr = pointers(b.dscene)
    ids0 = host(a.guides_ids()[1]).copy()
    fa = a.update_primitives(**_move(a), keep_history=True, max_history=16)
    fb = b.update_primitives(**_move(b), keep_history=True, rebuild=True, max_history=16)
    assert (a.scene_revision, a.bvh_rebuilds, b.scene_revision, b.bvh_rebuilds) == (1, 0, 2, 1)
    assert pointers(b.dscene) == ptr and b.arrays is b.dscene.arrays
    (ga, ia), (gb, ib) = a.guides_ids(), b.guides_ids()
    assert host(ga).tobytes() == host(gb).tobytes()  # the precondition: no equal-t ties in this view
    maps = tree.device_maps(a.dscene.layout.prim_perm, b.dscene.layout.prim_perm)
    for m in maps:  # the rebuild did reorder the spheres, the triangles and the quads
        assert len(m) > 6 and not np.array_equal(m, np.arange(len(m)))
    assert {0, 1, 2} <= set(np.unique(host(ia) >> 28).tolist())  # and every type shows in the image
    assert not np.array_equal(host(ia), host(ib)) and th.remap(host(ia), maps).tobytes() == host(ib).tobytes()
    assert not np.array_equal(host(ia), ids0)
    assert fa == fb and 0.5 < fa <= 1.0 and a.current_sample == b.current_sample == 4
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    # what the rebuilt renderer holds is a new renderer's scene, and renders as the oracle does
    assert uh.layouts_equal(b.dscene.layout, sd.pack_device(th.rebuilt(a.arrays))) == []
    assert uh.layouts_equal(b.dscene.layout, sd.pack_device(sd.compile_world(_world(True), b.arrays.perlin))) == []
    assert ph.compare(_render_image(b), _oracle_image(b), 8) == (0.0, 1.0)
    # rebuild_bvh on its own, of a scene unmoved since: the same tree and ids as the other renderer's
    fr = a.rebuild_bvh(keep_history=True, max_history=16)
    assert a.bvh_rebuilds == 1 and a.scene_revision == 2 and 0.5 < fr <= 1.0 and a.current_sample == 4
    assert all(host(x).tobytes() == host(y).tobytes() for x, y in zip(a.guides_ids(), (gb, ib)))
    assert a.rebuild_bvh() is None and a.current_sample == 0 and not host(a.accum).any()
    with pytest.raises(ValueError, match='need keep_history=True'):
        a.rebuild_bvh(max_history=8)


def test_motion_viewer_carries_its_history_across_a_rebuild(tmp_path):
    kw = dict(temporal=True, motion=True, max_history=8)
    a, b = _renderer(tmp_path, 'va', **kw), _renderer(tmp_path, 'vb', **kw)
    for v in (a, b):
        v.render_interactive()
    back = [_current(v) for v in (a, b)]
    a.update_primitives(**_move(a))
    b.update_primitives(**_move(b), rebuild=True)
    assert (a.bvh_rebuilds, b.bvh_rebuilds) == (0, 1) and a.history_fraction == b.history_fraction > 0.5
    assert host(a.guides_ids()[0]).tobytes() == host(b.guides_ids()[0]).tobytes()
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    # a second update with no sample in between reprojects the rendered history again, across the rebuild
    a.update_primitives(**back[0])
    b.update_primitives(**back[1], rebuild=True)
    assert (a.bvh_rebuilds, b.bvh_rebuilds) == (0, 2) and a.history_fraction == b.history_fraction
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    # rebuild_bvh with no sample in between: the rendered history again, to the same scene in a new device order
    b.rebuild_bvh()
    assert b.bvh_rebuilds == 3 and a.history_fraction == b.history_fraction and b.current_sample == 0
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()
    # a new render is the history; rebuild_bvh carries its ids and rows along, so the next update finds them
    for v in (a, b):
        v.render_interactive()
    assert b._history.rows is None
    b.rebuild_bvh()
    assert b._history.rows is not None and b._history_kept and b.bvh_rebuilds == 4
    assert host(b._history.ids).tobytes() == host(b.guides_ids()[1]).tobytes()  # the scene has not moved since
    for v in (a, b):
        v.update_primitives(**_move(v))
    assert a.history_fraction == b.history_fraction > 0.5
    assert host(a.accum).tobytes() == host(b.accum).tobytes() and host(a.stats).tobytes() == host(b.stats).tobytes()


def test_viewer_without_motion_drops_its_history_at_a_rebuild(tmp_path):
    c = _renderer(tmp_path, 'vc', temporal=True)
    c.render_interactive()
    c.update_primitives(**_move(c), rebuild=True)
    assert c.history_fraction is None and c._history is None and not host(c.accum).any() and c.bvh_rebuilds == 1
    c.render_interactive()
    c.restart_rendering()  # as after a camera move: the history is reprojected and kept
    assert c._history_kept and c.history_fraction > 0.5
    c.rebuild_bvh()
    assert c._history is None and not c._history_kept and c.history_fraction is None and c.bvh_rebuilds == 2
    assert not host(c.accum).any() and c.current_sample == 0
    c.restart_rendering()  # a plain restart: there is no history to reproject again
    c.render_interactive()
    assert c._history is not None and float(c.accum.sum()) > 0


def test_auto_rebuilds_above_the_threshold_only(tmp_path):
    probe = _renderer(tmp_path, 'p')
    assert probe.tree_growth() == (1.0, 1.0)
    sa0 = probe.arrays
    base = th.areas(sd.pack_device(sa0).ref_nodes)
    probe.update_primitives(**_move(probe))
    g = probe.tree_growth()
    assert g == tuple(float(x) for x in th.growth(sd.pack_device(probe.arrays).ref_nodes, base)[:2]) and g[0] > 1.0
    with pytest.raises(ValueError, match="False, True or 'auto'"):
        probe.update_primitives(rebuild='always')
    with pytest.raises(ValueError, match="threshold of rebuild='auto'"):
        probe.update_primitives(rebuild=True, rebuild_growth=2.0)
    with pytest.raises(ValueError, match='at least 1.0'):
        probe.update_primitives(rebuild='auto', rebuild_growth=0.5)
    assert probe.scene_revision == 1
    below, above = float(np.nextafter(f32(g[0]), f32(0))), g[0]
    for tag, threshold, rebuilt in (('lo', below, 1), ('hi', above, 0)):
        r = _renderer(tmp_path, tag)
        r.update_primitives(**_move(r), rebuild='auto', rebuild_growth=threshold)
        assert r.last_tree_growth == g and r.bvh_rebuilds == rebuilt and r.scene_revision == 1 + rebuilt
        assert r.tree_growth() == ((1.0, 1.0) if rebuilt else g)
        want = th.rebuilt(probe.arrays) if rebuilt else probe.arrays
        assert uh.layouts_equal(r.dscene.layout, sd.pack_device(want)) == []
        assert ph.compare(_render_image(r), _oracle_image(r), 8) == (0.0, 1.0)


def test_auto_without_a_threshold_follows_the_modules_constant(tmp_path):
    from ptmi import tree
    r = _renderer(tmp_path, 'n')
    if tree.REBUILD_GROWTH is None:
        with pytest.raises(ValueError, match='needs rebuild_growth='):
            r.update_primitives(**_move(r), rebuild='auto')
        assert r.scene_revision == 0
    else:
        assert tree.REBUILD_GROWTH > 1.0
        r.update_primitives(**_move(r), rebuild='auto')
        assert r.bvh_rebuilds == int(r.last_tree_growth[0] > tree.REBUILD_GROWTH)


def _history_inputs(r):
    """What a keep_history update reads, taken before it: accum, stats, guides, ids and the device rows, on the host."""
    import motion_helpers as mh
    rows = [host(t)[:n * k] for t, n, k in zip(r.dscene.primitive_rows(), (r.arrays.num_spheres, r.arrays.num_quads,
                                                                           r.arrays.num_triangles), (4, 16, 12))]
    g, i = r.guides_ids()
    return host(r.accum).copy(), host(r.stats).copy(), host(g).copy(), host(i).copy(), mh.rows_of(*rows)


def _assert_reprojected(r, before):
    """accum and stats are the numpy reference's reprojection (motion_helpers) of the inputs taken before the update."""
    import motion_helpers as mh
    import reproject_helpers as rh
    a0, s0, g0, i0, rows0 = before
    cam = sd.camera_upload(r.cam)
    _, _, g1, i1, rows1 = _history_inputs(r)
    want_a, want_s = mh.reproject_moved(cam, cam, g1, g0, a0, s0, i1, i0, rows1, rows0, **rh.DEFAULTS)
    assert np.array_equal(host(r.accum), want_a, equal_nan=True)
    assert np.array_equal(host(r.stats), want_s, equal_nan=True)
    assert (want_s[..., 0] > 0).mean() > 0.5


def test_default_update_launches_nothing_new_and_renders_what_it_did(tmp_path, monkeypatch):
    """The first two frames of the README's loop with update_primitives' defaults:
    no tree call after the baseline, the accumulator and the stats of both
    frames are the numpy reference's reprojection (the check of
    test_gpu_motion), and the image of the refit scene is the oracle's on the
    numpy refit of the same edit."""
    from ptmi import tree
    r = _renderer(tmp_path, 'd')
    sa0 = r.arrays
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)  # frame 0
    move, back = _move(r), _current(r)
    refit = _refit_of(sa0, move)
    before = _history_inputs(r)
    frac = r.update_primitives(**move, keep_history=True)  # frame 1: takes the baseline once, before the update
    _assert_reprojected(r, before)
    assert frac == float((host(r.stats)[..., 0] > 0).mean())
    base = host(r.dscene._tree['base'])[:sa0.num_bvh_nodes]
    assert base.tobytes() == th.areas(sd.pack_device(sa0).ref_nodes).tobytes()
    r.integrator.render_mk_stats(r.frame, r.accum, r.stats, r.current_sample, 2)  # new samples on the carried image
    r.current_sample += 2

    def no_tree_call():
        raise AssertionError('a default update made a tree call')

    monkeypatch.setattr(tree, 'load', no_tree_call)
    before = _history_inputs(r)
    r.update_primitives(spheres=back['spheres'], keep_history=True)  # frame 2: the spheres go back
    _assert_reprojected(r, before)
    r.update_primitives(spheres=move['spheres'])
    monkeypatch.undo()
    assert not host(r.accum).any() and r.current_sample == 0
    assert (r.bvh_rebuilds, r.last_tree_growth, r.scene_revision) == (0, None, 3)
    assert uh.layouts_equal(r.dscene.layout, sd.pack_device(refit)) == [] and uh.arrays_equal(r.arrays, refit)
    assert ph.compare(_render_image(r), _oracle_image(r), 8) == (0.0, 1.0)
    import oracle
    W, H = r.cam.img_width, r.cam.img_height
    o = np.zeros((H, W, 3), f32)
    fr = oracle.make_frame(sd.camera_upload(r.cam), r.background_color, 50, r.seed, W, H, 'stack')
    oracle.render(oracle.OracleScene(refit), fr, 'mk', o, (0, 0, W, H), 0, 8)
    assert _render_image(r).tobytes() == o.tobytes()
