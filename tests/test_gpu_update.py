"""GPU tests of the scene-update ABI (include/ptmi_update.h):
after DeviceScene.update_primitives the device buffers equal, byte for byte,
pack_device of the numpy reference (update_helpers.refit), and renders from
them equal the CPU oracle on the refit reference arrays, counters included."""
import random
import re

import numpy as np
import pytest

import guide_helpers as gh
import parity_helpers as ph
import update_helpers as uh
from ptmi import scene_data as sd

pytestmark = pytest.mark.gpu
f32 = np.float32
SHIFT = np.array([0.25, -0.5, 0.125], f32)


# ------------------------------------------------------------------ helpers
def device_image(ds):
    """What the device holds, as numpy arrays in the layout's shapes, and the view's host fields."""
    lay = ds.layout

    def host(t, like):
        return t.cpu().numpy().view(f32)[:like.size].reshape(like.shape).copy()

    img = {'nodes': host(ds.t_nodes, lay.nodes), 'ref_nodes': host(ds.t_ref_nodes, lay.ref_nodes),
           'spheres': host(ds.t_spheres, lay.spheres), 'quads': host(ds.t_quads, lay.quads),
           'tris': host(ds.t_tris, lay.tris), 'mats': host(ds.t_mats, lay.mats)}
    img['view_root'] = np.array(list(ds.view.root_min) + list(ds.view.root_max), f32)
    img['shell'] = int(ds.view.shell)
    return img


def assert_device_is(ds, expected_sa):
    """Device buffers, root box, shell hint, the layout and the mirror all equal pack_device(expected_sa)."""
    want = sd.pack_device(expected_sa)
    got = device_image(ds)
    for k in ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris', 'mats'):
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    root = np.concatenate([want.root_min, want.root_max]).astype(f32)
    assert got['view_root'].tobytes() == root.tobytes()
    assert ds._upd['root'].cpu().numpy().tobytes() == root.tobytes()  # what the call itself wrote
    assert got['shell'] == want.shell
    assert uh.layouts_equal(ds.layout, want) == []
    assert uh.arrays_equal(ds.arrays, expected_sa)
    return want


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def translate(sa, node, shift, into):
    """Add to ``into`` the edit that translates the primitive of leaf ``node`` by ``shift``."""
    t, i = int(sa.bvh['bvh_prim_type'][node]), int(sa.bvh['bvh_prim_idx'][node])
    if t == sd.PRIM_SPHERE:
        into['spheres'][i] = (sa.sphere_data[i, 0:3] + shift, sa.sphere_data[i, 3])
    elif t == sd.PRIM_QUAD:
        q = sa.quads
        into['quads'][i] = (q['quad_Q'][i] + shift, q['quad_u'][i], q['quad_v'][i])
    else:
        tr = sa.tris
        into['triangles'][i] = tuple(tr[k][i] + shift for k in ('triangle_v0', 'triangle_v1', 'triangle_v2'))


def as_edits(spec):
    out = {}
    if spec['spheres']:
        idx = sorted(spec['spheres'])
        out['spheres'] = uh.sphere_edit(idx, [spec['spheres'][i][0] for i in idx], [spec['spheres'][i][1] for i in idx])
    if spec['quads']:
        idx = sorted(spec['quads'])
        out['quads'] = uh.quad_edit(idx, [tuple(tuple(float(x) for x in v) for v in spec['quads'][i]) for i in idx])
    if spec['triangles']:
        idx = sorted(spec['triangles'])
        out['triangles'] = uh.tri_edit(idx, [tuple(tuple(float(x) for x in v) for v in spec['triangles'][i])
                                              for i in idx])
    return out


def edit_set(name, sa):
    """The edits of the moved-buffers tests, with the properties the tests rely
    on asserted from the reference: the first, the last and a deepest leaf in
    preorder, a sphere grown until the root box changes, a sphere shrunk so
    that the box above it shrinks, a quad thin along an axis, every type the
    scene has in one call."""
    b = sa.bvh
    pidx, ptype, parent = b['bvh_prim_idx'], b['bvh_prim_type'], b['bvh_parent']
    leaves = np.nonzero(pidx >= 0)[0]
    depth = sd.leaf_depths(b)
    deepest = int(leaves[np.argmax(depth[leaves])])
    assert depth[deepest] == depth.max() == {'coverage': 17, 'vol2_final_scene': 15}[name]
    spec = {'spheres': {}, 'quads': {}, 'triangles': {}}
    for node in (int(leaves[0]), int(leaves[-1]), deepest):
        translate(sa, node, SHIFT, spec)
    taken = set(spec['spheres'])
    lo, hi = b['bvh_bbox_min'][0], b['bvh_bbox_max'][0]
    if name == 'vol2_final_scene':  # the shell sphere is the root box: it grows; 20 of the box spheres move
        grow = int(pidx[sd.find_shell(sa, int(depth.max()))])
        rng = np.random.default_rng(3)
        free = [i for i in range(sa.num_spheres) if i not in taken and i != grow]
        for i in rng.choice(free, size=20, replace=False):
            spec['spheres'][int(i)] = (sa.sphere_data[i, 0:3] + rng.uniform(-30, 30, 3).astype(f32),
                                       sa.sphere_data[i, 3])
        spec['spheres'][grow] = (sa.sphere_data[grow, 0:3], sa.sphere_data[grow, 3] * f32(1.25))
    else:
        grow = next(i for i in range(sa.num_spheres) if i not in taken and sa.sphere_data[i, 3] < 10)
        # through the top of the root box
        spec['spheres'][grow] = (sa.sphere_data[grow, 0:3], f32(6.0) * sa.sphere_data[grow, 3])
    taken = set(spec['spheres'])
    leaf_s = uh.leaf_of(sa, sd.PRIM_SPHERE)
    # shrink: a sphere whose sibling is a leaf that no edit touches, so the parent's box must shrink
    edited = {int(leaf_s[i]) for i in taken} | {int(uh.leaf_of(sa, sd.PRIM_QUAD)[i]) for i in spec['quads']} | \
             {int(uh.leaf_of(sa, sd.PRIM_TRIANGLE)[i]) for i in spec['triangles']}

    def sibling(node):
        p = parent[node]
        return int(b['bvh_right_child'][p] if b['bvh_left_child'][p] == node else b['bvh_left_child'][p])

    shrink = next(i for i in range(sa.num_spheres) if i not in taken and sa.sphere_data[i, 3] > 0
                  and pidx[sibling(leaf_s[i])] >= 0 and sibling(leaf_s[i]) not in edited)
    spec['spheres'][shrink] = (sa.sphere_data[shrink, 0:3], sa.sphere_data[shrink, 3] * f32(0.25))
    thin = next(i for i in range(sa.num_quads) if i not in spec['quads'])
    Q = sa.quads['quad_Q'][thin]
    spec['quads'][thin] = (Q + SHIFT, np.array([2, 0, 0], f32), np.array([0, 0, 3], f32))  # in a plane y = const
    if sa.num_triangles and not spec['triangles']:
        translate(sa, int(uh.leaf_of(sa, sd.PRIM_TRIANGLE)[0]), SHIFT, spec)
    edits = as_edits(spec)
    ref = uh.refit(sa, edits)
    rb = ref.bvh
    # the properties, from the reference
    assert set(edits) == {k for k, n in (('spheres', sa.num_spheres), ('quads', sa.num_quads),
                                         ('triangles', sa.num_triangles)) if n}
    touched = {int(uh.leaf_of(sa, uh.BOXES[k][0])[i]) for k, e in edits.items() for i in e[0]}
    assert {int(leaves[0]), int(leaves[-1]), deepest} <= touched
    assert not (np.array_equal(rb['bvh_bbox_min'][0], lo) and np.array_equal(rb['bvh_bbox_max'][0], hi))
    p = parent[leaf_s[shrink]]
    assert np.all(rb['bvh_bbox_min'][p] >= b['bvh_bbox_min'][p])
    assert np.all(rb['bvh_bbox_max'][p] <= b['bvh_bbox_max'][p])
    assert not (np.array_equal(rb['bvh_bbox_min'][p], b['bvh_bbox_min'][p])
                and np.array_equal(rb['bvh_bbox_max'][p], b['bvh_bbox_max'][p]))
    tl = uh.leaf_of(sa, sd.PRIM_QUAD)[thin]
    ext = rb['bvh_bbox_max'][tl] - rb['bvh_bbox_min'][tl]
    assert 0 < ext[1] < 1.5e-4 and abs(ext[0] - 2) < 1e-3 and abs(ext[2] - 3) < 1e-3  # padded along y only
    return edits, ref


def tiny_scene(n):
    """A one-sphere world (no internal node) or a sphere and a quad (one internal node)."""
    from ptmi import core
    random.seed(7)
    w = core.hittable_list()
    w.add(core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))))
    if n == 2:
        w.add(core.quad(core.vec3(-2, -0.5, -3), core.vec3(4, 0, 0), core.vec3(0, 0, 4),
                        core.metal(core.vec3(.8, .8, .8), 0.1)))
    return sd.compile_world(w)


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
    return acc.cpu().numpy(), integ.read_counters(), o, {k: int(v) for k, v in ost.items()}


def assert_parity(ds, ref_sa, cam, bg, combos, spp=8):
    for variant, traversal in combos:
        g, cnt, o, ost = render_pair(ds, ref_sa, cam, bg, variant, traversal, spp)
        linf, exact = ph.compare(g, o, spp)
        assert linf == 0.0 and exact == 1.0, (variant, traversal, linf, exact)
        assert cnt == ost, (variant, traversal)
        assert np.isfinite(g).all() and g.sum() > 0


COMBOS = [('mk', 'stack'), ('mk', 'stackless'), ('wf', 'stack'), ('wf', 'stackless')]
MOVED = ['coverage', 'vol2_final_scene']


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize('name', ['vol2_final_scene', 'coverage', 'cornell_mesh_fog', 'one_sphere', 'two_primitives'])
def test_zero_edit_call_is_the_identity(name):
    sa = tiny_scene(1 if name == 'one_sphere' else 2) if name in ('one_sphere', 'two_primitives') \
        else ph.scene_inputs(name, 64)[0]
    ds = new_scene(sa)
    assert ds.view.n_inner == {'one_sphere': 0, 'two_primitives': 1}.get(name, ds.view.n_inner)
    before = device_image(ds)
    for flags in (0, 1, None):  # one launch per level, the single workgroup, the wrapper's choice
        ds.update_primitives(flags=flags)
        after = device_image(ds)
        for k in before:
            assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), (k, flags)
        assert_device_is(ds, sa)
    ds.update_primitives(spheres=(np.zeros(0, np.int64), np.zeros((0, 4), f32), np.zeros((0, 4), f32)))  # empty lists
    assert_device_is(ds, sa)


# ------------------------------------------------------------------ moved, and moved back
@pytest.mark.parametrize('form', ['per_level', 'one_group'])
@pytest.mark.parametrize('name', MOVED)
def test_moved_buffers_equal_the_packed_reference_and_the_inverse_restores_them(name, form):
    from ptmi import update
    flags = {'per_level': 0, 'one_group': update.ONE_GROUP}[form]
    sa = ph.scene_inputs(name, 64)[0]
    edits, ref = edit_set(name, sa)
    ds = new_scene(sa)
    ds.update_primitives(flags=flags, **edits)
    want = assert_device_is(ds, ref)
    assert uh.layouts_equal(want, sd.pack_device(sa))  # and that is not what was there before
    if name == 'vol2_final_scene':
        assert len(ds._upd['level_end']) == 15 and want.shell != 0  # the grown shell still encloses the scene
    ds.update_primitives(flags=flags, **{k: uh.current(sa, k, e[0]) for k, e in edits.items()})
    assert_device_is(ds, sa)
    assert uh.arrays_equal(sa, ph.scene_inputs(name, 64)[0])  # the caller's arrays were never written


def test_one_sphere_scene_moves_without_internal_nodes():
    sa = tiny_scene(1)
    ds = new_scene(sa)
    e = {'spheres': uh.sphere_edit([0], [(1.0, 2.0, -3.0)], [0.75])}
    ds.update_primitives(**e)
    assert_device_is(ds, uh.refit(sa, e))


# ------------------------------------------------------------------ render parity
@pytest.mark.parametrize('name', MOVED)
def test_render_parity_after_the_update(name):
    sa, cam, bg = ph.scene_inputs(name, 64)
    edits, ref = edit_set(name, sa)
    ds = new_scene(sa)
    ds.update_primitives(**edits)
    assert_parity(ds, ref, cam, bg, COMBOS)
    # the same image from a scene made anew from the mirror
    fresh = new_scene(sd.pack_device(ds.arrays))
    for variant, traversal in (('mk', 'stack'), ('wf', 'stackless')):
        a = render_pair(ds, ref, cam, bg, variant, traversal)[0]
        c = render_pair(fresh, ref, cam, bg, variant, traversal)[0]
        assert a.tobytes() == c.tobytes()


# ------------------------------------------------------------------ the shell hint
@pytest.mark.parametrize('case', ['small_sphere_inside', 'sphere_beyond_half_radius', 'shell_moved_a_little',
                                  'shell_moved_far'])
def test_shell_hint_follows_the_claim(case):
    sa, cam, bg = ph.scene_inputs('vol2_final_scene', 64)
    lay0 = sd.pack_device(sa)
    shell = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, lay0.max_leaf_depth)])
    c, R = sa.sphere_data[shell, 0:3], sa.sphere_data[shell, 3]
    small = next(i for i in range(sa.num_spheres) if i != shell and sa.sphere_data[i, 3] <= 10)
    e = {'small_sphere_inside': uh.sphere_edit([small], [c + f32(0.1) * R * np.array([0, 1, 0], f32)], [10.0]),
         'sphere_beyond_half_radius': uh.sphere_edit([small], [c + f32(0.6) * R * np.array([0, 1, 0], f32)], [10.0]),
         'shell_moved_a_little': uh.sphere_edit([shell], [c + f32(0.1) * R * np.array([1, 0, 0], f32)], [R]),
         'shell_moved_far': uh.sphere_edit([shell], [c + f32(0.4) * R * np.array([1, 0, 0], f32)], [R])}[case]
    ref = uh.refit(sa, {'spheres': e})
    want = sd.pack_device(ref).shell
    keeps = case in ('small_sphere_inside', 'shell_moved_a_little')
    assert lay0.shell != 0 and (want == lay0.shell if keeps else want == 0)
    ds = new_scene(sa)
    assert ds.view.shell == lay0.shell
    ds.update_primitives(spheres=e)
    assert ds.view.shell == want == ds.layout.shell
    assert_device_is(ds, ref)
    assert_parity(ds, ref, cam, bg, [('mk', 'stack')])  # the kernels that use the hint


# ------------------------------------------------------------------ the C level
def test_ids_out_of_range_are_skipped_on_the_device():
    """Through ctypes, past the wrapper's checks: edits whose primitive or leaf
    id is out of range, or whose leaf holds another primitive, touch nothing;
    the one valid edit among them is applied."""
    import torch
    sa = ph.scene_inputs('coverage', 64)[0]
    ds = new_scene(sa)
    ds.update_primitives()  # makes the topology
    st = ds._upd
    good = 2
    leaf_good, dev_good = int(st['leaf_of'][0][good]), int(st['dev_of'][0][good])
    other_leaf = int(st['leaf_of'][0][3])
    inner_node = int(st['inner'][1])
    nb, ns = sa.num_bvh_nodes, sa.num_spheres
    dev = ds.device
    valid = (0.5, 1.5, -2.5, 0.25)
    # two calls: a list may not be longer than the type's primitive count (6 spheres)
    for prim, leaf in (([-1, ns, 1 << 30, dev_good, 0, 1], [leaf_good, leaf_good, leaf_good, leaf_good, -1, nb]),
                       ([int(st['dev_of'][0][4]), int(st['dev_of'][0][5])], [other_leaf, inner_node])):
        rows = np.full((len(prim), 4), 777.0, f32)
        if dev_good in prim:
            rows[prim.index(dev_good)] = valid
        tp, tl = (torch.tensor(a, dtype=torch.int32, device=dev) for a in (prim, leaf))
        tr = torch.from_numpy(rows.reshape(-1)).to(dev)
        ds.update_call({sd.PRIM_SPHERE: (tp.data_ptr(), tl.data_ptr(), tr.data_ptr(), tr.data_ptr(), len(prim))})
        torch.cuda.synchronize()
    rows = np.array([valid], f32)
    want = sd.pack_device(uh.refit(sa, {'spheres': uh.sphere_edit([good], [rows[0, 0:3]], [rows[0, 3]])}))
    got = device_image(ds)
    for k in ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris'):
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
        assert not np.any(got[k] == f32(777.0)), k
    # quads and triangles: an id past the type's count
    for t, n, nrow in ((sd.PRIM_QUAD, sa.num_quads, 16), (sd.PRIM_TRIANGLE, sa.num_triangles, 12)):
        tp = torch.tensor([n, -5], dtype=torch.int32, device=dev)
        tl = torch.tensor([int(st['leaf_of'][t][0])] * 2, dtype=torch.int32, device=dev)
        tr = torch.full((2 * nrow,), 777.0, dtype=torch.float32, device=dev)
        ds.update_call({t: (tp.data_ptr(), tl.data_ptr(), tr.data_ptr(), tr.data_ptr(), 2)})
    torch.cuda.synchronize()
    again = device_image(ds)
    for k in ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris'):
        assert again[k].tobytes() == got[k].tobytes(), k


def test_wrapper_rejects_bad_edits_before_any_upload():
    sa = ph.scene_inputs('coverage', 64)[0]
    ds = new_scene(sa)
    before = device_image(ds)
    row = np.array([[0, 0, 0, 1]], f32)
    for bad, msg in (((np.array([sa.num_spheres]), row, row), 'outside'), ((np.array([-1]), row, row), 'outside'),
                     ((np.array([1, 1]), np.repeat(row, 2, 0), np.repeat(row, 2, 0)), 'repeated'),
                     ((np.array([1]), row, row + 1), 'different points'),
                     ((np.array([1]), np.array([[np.nan, 0, 0, 1]], f32), row), 'finite'),
                     ((np.array([1.5]), row, row), 'integer'), ((np.array([1]), row[:, :3], row), '(n, 4)')):
        with pytest.raises(ValueError, match=re.escape(msg)):
            ds.update_primitives(spheres=bad)
    after = device_image(ds)
    for k in before:
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    from ptmi import _lib
    with pytest.raises(_lib.PtmiError, match='SceneArrays'):
        new_scene(sd.pack_device(sa)).update_primitives()


def test_update_on_a_side_stream():
    import torch
    sa = ph.scene_inputs('coverage', 64)[0]
    edits, ref = edit_set('coverage', sa)
    ds = new_scene(sa)
    side = torch.cuda.Stream(ds.device)
    ds.update_primitives(stream=side, **edits)
    assert_device_is(ds, ref)


# ------------------------------------------------------------------ the renderer
def _world(centre, radius=0.5):
    from ptmi import core
    w = core.hittable_list()
    grey = core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))
    w.add(core.Sphere.stationary(core.vec3(0, -100.5, -1), 100, grey))
    w.add(core.Sphere.stationary(core.vec3(*centre), radius, core.lambertian(core.solid_color(core.vec3(.7, .3, .3)))))
    w.add(core.Sphere.stationary(core.vec3(1.2, 0, -1), 0.5, core.metal(core.vec3(.8, .6, .2), 0.2)))
    w.add(core.quad(core.vec3(-2, -0.5, -3), core.vec3(4, 0, 0), core.vec3(0, 2, 0), grey))
    w.add(core.triangle(core.vec3(-1.5, -0.5, 0), core.vec3(-0.5, -0.5, 0), core.vec3(-1, 0.5, 0),
                        core.dielectric(1.5)))
    return w


def _camera(width=48):
    from ptmi import core
    cam = core.camera()
    cam.aspect_ratio, cam.img_width, cam.samples_per_pixel, cam.vfov = 1.5, width, 4, 50
    cam.lookfrom, cam.lookat, cam.vup = core.vec3(0, 0.5, 3), core.vec3(0, 0, -1), core.vec3(0, 1, 0)
    cam.defocus_angle = 0.0
    return cam


def test_renderer_update_resets_the_image_and_keeps_the_mirror(tmp_path):
    import torch
    from ptmi import core
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import _History
    random.seed(99)
    r = InteractiveViewer(_world((0, 0, -1)), _camera(), str(tmp_path / 'u.png'), temporal=True)
    tables = r.arrays.perlin
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    g0 = r.guides().cpu().numpy().copy()
    r.denoise()
    r._history, r._history_kept = _History(r.frame.cam, r.guides()), True
    r._history_spare = (torch.empty_like(r.accum), torch.empty_like(r.stats))
    assert r.current_sample == 4 and float(r.accum.abs().sum()) > 0 and r._tiles['n'] == 0
    moved = core.Sphere.stationary(core.vec3(-0.6, 0.3, -0.4), 0.35, r.primitives['spheres'][1].material)
    r.update_primitives(spheres={1: moved})
    torch.cuda.synchronize()
    assert r.scene_revision == 1 and r.current_sample == 0 and r.adaptive_passes == []
    assert float(r.accum.abs().sum()) == 0 and float(r.stats.abs().sum()) == 0
    ntiles = r._tiles['grid'][0] * r._tiles['grid'][1]
    assert r._tiles['n'] == ntiles and int(r._tiles['state'].sum()) == ntiles
    assert r.denoised is None and r.denoised_var is None and r._history_spare is None
    assert r._history is None and not r._history_kept  # the viewer's history
    # the mirror: a full compile of the edited world has the same geometry arrays (its tree differs)
    full = sd.compile_world(_world((-0.6, 0.3, -0.4), 0.35), tables)
    assert r.arrays is r.dscene.arrays and r.arrays.sphere_data.tobytes() == full.sphere_data.tobytes()
    for k in sd.QUAD_KEYS:
        assert r.arrays.quads[k].tobytes() == full.quads[k].tobytes()
    for k in sd.TRI_KEYS:
        assert r.arrays.tris[k].tobytes() == full.tris[k].tobytes()
    # the guides are retraced, changed, and are those of the mirror
    g1 = r.guides().cpu().numpy()
    assert g1.tobytes() != g0.tobytes()
    want = gh.trace_guides(r.arrays, sd.camera_upload(r.cam))
    assert g1.tobytes() == want.tobytes()
    # quads and triangles through the same surface, then a render
    q = r.primitives['quads'][0]
    t = r.primitives['triangles'][0]
    r.update_primitives(quads={0: core.quad(q.Q + core.vec3(0, 0, -0.5), q.u, q.v, q.mat)},
                        triangles={0: core.triangle(t.v0, t.v1, t.v2 + core.vec3(0, 0.25, 0), t.mat)})
    assert r.scene_revision == 2
    r.render_adaptive(target_error=0.0, min_spp=2, max_spp=2)
    assert r.current_sample == 2 and np.isfinite(r.accum.cpu().numpy()).all() and float(r.accum.sum()) > 0
    # what an update cannot do names the rebuild path
    for bad in ({'spheres': {7: moved}}, {'spheres': {1: q}}, {'quads': {0: moved}},
                {'spheres': {1: core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, core.dielectric(1.5))}}):
        with pytest.raises(ValueError, match='build a new MI355XRenderer'):
            r.update_primitives(**bad)
    assert r.scene_revision == 2
