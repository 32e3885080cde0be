"""GPU tests of the material-edit ABI (include/ptmi_material.h):
after DeviceScene.update_materials the device buffers and the view equal, byte
for byte, pack_device of the numpy reference (material_helpers.apply) on the
same BVH; renders from them equal the CPU oracle on the edited arrays, counters
included, on the megakernel and the wavefront, stack and stackless walk; the
shell hint follows the medium bit; edits the kernel must skip touch nothing; and
the renderer and the viewer treat the image as they do for update_primitives."""
import random

import numpy as np
import pytest

import material_helpers as mh
import motion_helpers as mo
import parity_helpers as ph
import reproject_helpers as rh
import update_helpers as uh
from ptmi import scene_data as sd

pytestmark = pytest.mark.gpu
f32 = np.float32
PARTS = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris', 'mats')


# ------------------------------------------------------------------ helpers
def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def device_image(ds):
    """What the device holds, as numpy arrays in the layout's shapes, and the view's host fields."""
    lay = ds.layout
    img = {k: host(t).view(f32)[:getattr(lay, k).size].reshape(getattr(lay, k).shape).copy()
           for k, t in (('nodes', ds.t_nodes), ('ref_nodes', ds.t_ref_nodes), ('spheres', ds.t_spheres),
                        ('quads', ds.t_quads), ('tris', ds.t_tris), ('mats', ds.t_mats))}
    v = ds.view
    img['view'] = np.array([v.root_ref, v.shell, v.max_leaf_depth, v.n_inner, v.num_bvh_nodes, v.num_images], np.int64)
    img['view_root'] = np.array(list(v.root_min) + list(v.root_max), f32)
    return img


def same_image(a, b):
    return [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def assert_device_is(ds, expected_sa):
    """Device buffers, root ref, shell hint, the layout and the mirror all equal pack_device(expected_sa)."""
    want = sd.pack_device(expected_sa)
    got = device_image(ds)
    for k in PARTS:
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    assert (int(ds.view.root_ref), int(ds.view.shell)) == (want.root_ref, want.shell)
    assert uh.layouts_equal(ds.layout, want) == []
    assert uh.arrays_equal(ds.arrays, expected_sa) and mh.mats_equal(ds.arrays, expected_sa)
    return want


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def tiny_scene(n):
    """A one-sphere world (no internal node: the root is a leaf) or a sphere and a quad (one internal node)."""
    from ptmi import core
    random.seed(7)
    w = core.hittable_list()
    w.add(core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))))
    if n == 2:
        w.add(core.quad(core.vec3(-2, -0.5, -3), core.vec3(4, 0, 0), core.vec3(0, 0, 4),
                        core.metal(core.vec3(.8, .8, .8), 0.1)))
    return sd.compile_world(w)


def scene_of(name):
    if name in ('one_sphere', 'two_primitives'):
        return tiny_scene(1 if name == 'one_sphere' else 2)
    return ph.scene_inputs(name, 64)[0]


def inverse(sa, edits):
    return {k: mh.current(sa, k, e[0]) for k, e in edits.items()}


FIXTURES = ['vol2_final_scene', 'coverage', 'cornell_mesh_fog', 'one_sphere', 'two_primitives']


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize('name', FIXTURES)
def test_zero_edit_and_null_edit_calls_change_no_byte(name):
    sa = scene_of(name)
    ds = new_scene(sa)
    assert ds.view.n_inner == {'one_sphere': 0, 'two_primitives': 1}.get(name, ds.view.n_inner)
    before = device_image(ds)
    ds.update_materials()
    assert same_image(before, device_image(ds)) == []
    ds.update_materials(spheres=(np.zeros(0, np.int64), np.zeros((0, 20), f32)))  # empty lists
    assert same_image(before, device_image(ds)) == []
    counts = {'spheres': sa.num_spheres, 'quads': sa.num_quads, 'triangles': sa.num_triangles}
    ds.update_materials(**{k: mh.current(sa, k, np.arange(n)) for k, n in counts.items() if n})  # the rows they have
    assert same_image(before, device_image(ds)) == []
    assert_device_is(ds, sa)


# ------------------------------------------------------------------ edited, and edited back
@pytest.mark.parametrize('offset', [0, 5])
@pytest.mark.parametrize('name', FIXTURES)
def test_edited_buffers_equal_the_packed_reference_and_the_inverse_restores_them(name, offset):
    sa = scene_of(name)
    snapshot = mh.apply(sa, {})  # copies of the caller's material arrays
    edits = mh.walk_edits(sa, offset)
    if sa.num_spheres + sa.num_quads + sa.num_triangles >= 10:
        assert mh.classes_of(edits) == set(range(6))
    ref = mh.apply(sa, edits)
    ds = new_scene(sa)
    before = device_image(ds)
    ds.update_materials(**edits)
    want = assert_device_is(ds, ref)
    assert 'mats' in uh.layouts_equal(want, sd.pack_device(sa))  # and that is not what was there before
    if name == 'one_sphere' and offset == 5:  # Lambertian to emissive: the root's own code changes
        assert want.root_ref != sd.pack_device(sa).root_ref and ds.view.root_ref == want.root_ref
    ds.update_materials(**inverse(sa, edits))
    assert_device_is(ds, sa)
    assert same_image(before, device_image(ds)) == []
    assert mh.mats_equal(sa, snapshot)  # the caller's arrays were never written


def big_scene():
    """A generated scene of 749 primitives (300 spheres, 250 quads, 199 triangles), materials by random_scenes."""
    import random_scenes as rs
    from ptmi import core
    r = random.Random(11)
    earth = core.image_texture(sd.load_earthmap())
    w = core.hittable_list()
    for _ in range(300):
        w.add(core.Sphere.stationary(rs._p(r, 20.0), r.uniform(0.2, 1.0), rs._material(r, earth)))
    for _ in range(250):
        w.add(core.quad(rs._p(r, 20.0), core.vec3(r.uniform(-2, 2), r.uniform(-2, 2), 0), core.vec3(0, r.uniform(-2, 2), 1),
                        rs._material(r, earth)))
    for _ in range(199):
        a = rs._p(r, 20.0)
        w.add(core.triangle(a, a + core.vec3(1, r.uniform(0, 2), 0), a + core.vec3(0, 1, r.uniform(0.5, 2)),
                            rs._material(r, earth)))
    random.seed(1011)
    return sd.compile_world(w)


def test_every_primitive_of_a_generated_scene_edited_in_one_call():
    """749 edits: three blocks of 256 lanes, the last one partial, and all three lists in one launch."""
    sa = big_scene()
    n = sa.num_spheres + sa.num_quads + sa.num_triangles
    assert 600 <= n <= 1000 and n % 256 != 0 and n > 512 and len(sa.images) == 1
    edits = mh.walk_edits(sa, offset=2)
    assert sum(len(e[0]) for e in edits.values()) == n and mh.classes_of(edits) == set(range(6))
    ds = new_scene(sa)
    ds.update_materials(**edits)
    assert_device_is(ds, mh.apply(sa, edits))
    ds.update_materials(**inverse(sa, edits))
    assert_device_is(ds, sa)


# ------------------------------------------------------------------ render parity
def render_gpu(ds, cam, bg, variant, traversal, spp=8, stats=False, max_depth=50, seed=0):
    import torch
    from ptmi import device
    W, H = cam['width'], cam['height']
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, bg, max_depth, seed, W, H, traversal=traversal)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    st = None
    if stats:
        st = integ.new_stats(fr)
        (integ.render_mk_stats if variant == 'mk' else integ.render_wf_stats)(fr, acc, st, 0, spp)
    else:
        (integ.render_mk if variant == 'mk' else integ.render_wf)(fr, acc, 0, spp)
    torch.cuda.synchronize()
    return host(acc), integ.read_counters(), None if st is None else host(st)


def render_oracle(ref_sa, cam, bg, variant, traversal, spp=8, max_depth=50, seed=0):
    import oracle
    W, H = cam['width'], cam['height']
    o = np.zeros((H, W, 3), f32)
    ost = oracle.render(oracle.OracleScene(ref_sa), oracle.make_frame(cam, bg, max_depth, seed, W, H, traversal),
                        variant, o, (0, 0, W, H), 0, spp)
    return o, {k: int(v) for k, v in ost.items()}


def assert_parity(ds, ref_sa, cam, bg, variant, traversal, spp=8, stats=False, **kw):
    g, cnt, st = render_gpu(ds, cam, bg, variant, traversal, spp, stats, **kw)
    o, ost = render_oracle(ref_sa, cam, bg, variant, traversal, spp, **kw)
    linf, exact = ph.compare(g, o, spp)
    assert linf == 0.0 and exact == 1.0, (variant, traversal, linf, exact)
    assert cnt == ost, (variant, traversal)
    assert np.isfinite(g).all() and g.sum() > 0
    if stats:
        assert (st[..., 0] == spp).all()


_edited = {}


def edited_coverage():
    """(reference arrays, camera, background) of `coverage` with every primitive's material walked on: shared."""
    if not _edited:
        sa, cam, bg = ph.scene_inputs('coverage', 64)
        edits = mh.walk_edits(sa, offset=3)
        before = sd.material_class(mh.flags_of(np.concatenate([mh.rows_of(sa, k)[e[0]] for k, e in edits.items()])))
        after = sd.material_class(mh.flags_of(np.concatenate([e[1] for e in edits.values()])))
        assert (before != after).mean() > 0.5 and set(after.tolist()) == set(range(6))  # the classes do move
        _edited.update(sa=sa, edits=edits, ref=mh.apply(sa, edits), cam=cam, bg=bg)
    return _edited


@pytest.mark.parametrize('variant,traversal', [('mk', 'stack'), ('mk', 'stackless'), ('wf', 'stack'), ('wf', 'stackless')])
def test_render_parity_after_the_edit(variant, traversal):
    """The wavefront sorts by the class in the `nodes` leaf codes (stack walk) or the `ref_nodes` ones
    (stackless): a code that kept its old class shades a hit with the wrong kernel."""
    c = edited_coverage()
    ds = new_scene(c['sa'])
    ds.update_materials(**c['edits'])
    assert_parity(ds, c['ref'], c['cam'], c['bg'], variant, traversal)


def test_render_parity_after_the_edit_through_the_stats_path():
    c = edited_coverage()
    ds = new_scene(c['sa'])
    ds.update_materials(**c['edits'])
    assert_parity(ds, c['ref'], c['cam'], c['bg'], 'wf', 'stack', stats=True)
    # and the same image from a scene made anew from the mirror
    a = render_gpu(ds, c['cam'], c['bg'], 'wf', 'stackless')[0]
    b = render_gpu(new_scene(sd.pack_device(ds.arrays)), c['cam'], c['bg'], 'wf', 'stackless')[0]
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the shell hint
def test_shell_hint_follows_the_medium_bit():
    import shell_scenes as ss
    sa, cam = ss.shell_scene(5000.0)
    lay0 = sd.pack_device(sa)
    shell = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, lay0.max_leaf_depth)])
    assert lay0.shell != 0 and sa.sphere_mats['is_constant_medium'][shell] == 1
    ds = new_scene(sa)
    assert ds.view.shell == lay0.shell
    idx, rows = mh.current(sa, 'spheres', [shell])
    plain = rows.copy()
    plain[:, 19] = (mh.flags_of(rows) & ~np.uint32(0x100)).view(f32)  # the same record, no longer a medium
    ref = mh.apply(sa, {'spheres': (idx, plain)})
    assert sd.pack_device(ref).shell == 0
    ds.update_materials(spheres=(idx, plain))
    assert ds.view.shell == 0 == ds.layout.shell
    assert_device_is(ds, ref)
    assert_parity(ds, ref, cam, ss.BG, 'mk', 'stack', seed=7)  # the kernels that use the hint
    ds.update_materials(spheres=(idx, rows))
    assert ds.view.shell == lay0.shell != 0
    assert_device_is(ds, sa)
    assert_parity(ds, sa, cam, ss.BG, 'mk', 'stack', seed=7)


def test_fog_density_through_media_keeps_the_hint(tmp_path):
    import shell_scenes as ss
    from ptmi import core
    from ptmi.renderer import MI355XRenderer
    from ptmi.scenes import _wrap
    R = 5000.0
    cam = core.camera()
    cam.aspect_ratio, cam.img_width, cam.vfov = 1.0, ss.WIDTH, 50.0
    cam.lookfrom, cam.lookat, cam.vup = core.point3(4 * R / 100, 6 * R / 100, 30 * R / 100), core.point3(0, 0, 0), \
        core.vec3(0, 1, 0)
    random.seed(99)
    r = MI355XRenderer(_wrap(ss.shell_world(R).objects), cam, str(tmp_path / 's.png'))
    sa0 = r.arrays
    shell = int(np.nonzero(sa0.sphere_mats['is_constant_medium'])[0][0])
    hint = int(r.dscene.view.shell)
    assert hint != 0 and hint == sd.pack_device(sa0).shell
    density = float(sa0.sphere_mats['medium_density'][shell])
    r.update_materials(media={('spheres', shell): (8 * density, (0.5, 0.6, 0.7))})
    idx, rows = mh.current(sa0, 'spheres', [shell])
    rows[:, 15], rows[:, 16:19] = f32(8 * density), (0.5, 0.6, 0.7)
    ref = mh.apply(sa0, {'spheres': (idx, rows)})
    assert int(r.dscene.view.shell) == hint and r.scene_revision == 1
    assert_device_is(r.dscene, ref)
    assert not mh.mats_equal(ref, sa0) and mh.mats_equal(sa0, mh.apply(sa0, {}))
    cu = sd.camera_upload(r.cam)
    assert_parity(r.dscene, ref, cu, ss.BG, 'mk', 'stack', seed=7)
    assert_parity(r.dscene, ref, cu, ss.BG, 'wf', 'stackless', seed=7)
    other = (shell + 1) % sa0.num_spheres
    assert not sa0.sphere_mats['is_constant_medium'][other]
    for bad in ({('spheres', other): (1.0, (1, 1, 1))}, {('quads', 0): (1.0, (1, 1, 1))}):
        with pytest.raises(ValueError, match='not the boundary of a constant medium'):
            r.update_materials(media=bad)
    with pytest.raises(ValueError, match='is not \\(kind, index\\)'):
        r.update_materials(media={shell: (1.0, (1, 1, 1))})
    assert r.scene_revision == 1


# ------------------------------------------------------------------ the C level
def test_edits_the_kernel_must_skip_touch_nothing():
    """Through ctypes, past the wrapper's checks: an edit whose primitive or leaf id is out of range, whose
    leaf holds another primitive or one of another type, or whose flags name an image past num_images,
    touches nothing; the valid edits among them are applied."""
    import torch
    sa = ph.scene_inputs('coverage', 64)[0]
    ds = new_scene(sa)
    ds.update_materials()  # makes the topology
    st = ds._upd
    dev = ds.device
    ns, nb, n_img = sa.num_spheres, sa.num_bvh_nodes, len(sa.images)
    assert ns >= 4 and sa.num_quads >= 1
    dev_s, leaf_s = st['dev_of'][sd.PRIM_SPHERE], st['leaf_of'][sd.PRIM_SPHERE]
    # a quad whose device row is a valid sphere row: "a leaf of the wrong type" passes the range check
    quad = next(i for i in range(sa.num_quads) if st['dev_of'][sd.PRIM_QUAD][i] < ns)
    quad_leaf, quad_dev = int(st['leaf_of'][sd.PRIM_QUAD][quad]), int(st['dev_of'][sd.PRIM_QUAD][quad])
    inner = int(st['inner'][1])
    good = mh.row(mh.DIELECTRIC, albedo=(1, 1, 1), ir=1.25, color1=(1, 1, 1), color2=(1, 1, 1))
    bad = np.full(20, 777.0, f32)
    bad[19:20] = np.array([mh.flags_word(mh.METAL)], np.uint32).view(f32)
    past = bad.copy()
    past[19:20] = np.array([mh.flags_word(mh.LAMBERTIAN, mh.IMAGE, image=n_img)], np.uint32).view(f32)
    max_img = bad.copy()
    max_img[19:20] = np.array([0xffff0020], np.uint32).view(f32)
    calls = [
        # prim out of range (below, at the count, far above); the valid edit of sphere 2 among them
        ([-1, ns, 1 << 30, int(dev_s[2])], [int(leaf_s[0])] * 3 + [int(leaf_s[2])], [bad, bad, bad, good]),
        # leaf out of range; a leaf naming another primitive; an internal node; a leaf of the wrong type
        ([int(dev_s[0]), int(dev_s[0]), int(dev_s[1]), int(dev_s[1])], [-1, nb, int(leaf_s[3]), inner], [bad] * 4),
        ([quad_dev], [quad_leaf], [bad]),
        # an image index past num_images, and the largest one a flags word can hold; the valid edit of sphere 3
        ([int(dev_s[0]), int(dev_s[1]), int(dev_s[3])], [int(leaf_s[0]), int(leaf_s[1]), int(leaf_s[3])],
         [past, max_img, good]),
    ]
    for prim, leaf, rows in calls:
        assert len(prim) <= ns
        tp, tl = (torch.tensor(a, dtype=torch.int32, device=dev) for a in (prim, leaf))
        tr = torch.from_numpy(np.stack(rows).reshape(-1)).to(dev)
        ds.material_call({sd.PRIM_SPHERE: (tp.data_ptr(), tl.data_ptr(), tr.data_ptr(), len(prim))})
        torch.cuda.synchronize()
    want = sd.pack_device(mh.apply(sa, {'spheres': (np.array([2, 3]), np.stack([good, good]))}))
    got = device_image(ds)
    for k in PARTS:
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
        assert not np.any(got[k] == f32(777.0)), k
    assert 'mats' in uh.layouts_equal(want, sd.pack_device(sa))
    # quads and triangles: an id past the type's count, a sphere's leaf
    for t, n in ((sd.PRIM_QUAD, sa.num_quads), (sd.PRIM_TRIANGLE, sa.num_triangles)):
        if n < 2:
            continue
        tp = torch.tensor([n, 0], dtype=torch.int32, device=dev)
        tl = torch.tensor([int(st['leaf_of'][t][0]), int(leaf_s[0])], dtype=torch.int32, device=dev)
        tr = torch.from_numpy(np.stack([bad, bad]).reshape(-1)).to(dev)
        ds.material_call({t: (tp.data_ptr(), tl.data_ptr(), tr.data_ptr(), 2)})
    torch.cuda.synchronize()
    assert same_image(got, device_image(ds)) == []


def test_wrapper_rejects_bad_edits_before_any_upload():
    sa = ph.scene_inputs('coverage', 64)[0]
    ds = new_scene(sa)
    before = device_image(ds)
    good = mh.row(mh.METAL, albedo=(.5, .5, .5))
    for bad, msg in ((([sa.num_spheres], [good]), 'outside'), (([1, 1], [good, good]), 'repeated'),
                     (([1], [good[:12]]), '(n, 20)'),
                     (([1], [mh.row(mh.LAMBERTIAN, mh.IMAGE, image=len(sa.images))]), 'names image')):
        with pytest.raises(ValueError, match=msg.replace('(', '\\(').replace(')', '\\)')):
            ds.update_materials(spheres=bad)
    assert same_image(before, device_image(ds)) == []
    from ptmi import _lib
    with pytest.raises(_lib.PtmiError, match='SceneArrays'):
        new_scene(sd.pack_device(sa)).update_materials()


def test_update_on_a_side_stream():
    import torch
    c = edited_coverage()
    ds = new_scene(c['sa'])
    side = torch.cuda.Stream(ds.device)
    ds.update_materials(stream=side, **c['edits'])
    assert_device_is(ds, c['ref'])


# ------------------------------------------------------------------ the renderer
GREY, RED, BLUE = (.5, .5, .5), (.7, .3, .3), (.1, .2, .9)
WALL, LIGHT = 0, 1  # the quads


def _lamb(c):
    from ptmi import core
    return core.lambertian(core.solid_color(core.vec3(*c)))


def _light(e):
    from ptmi import core
    return core.diffuse_light.from_color(core.color(*e))


def _world(ball=None, wall=None, light=None, centre=(0, 0, -1)):
    """A ground sphere, a ball, a metal sphere, a back wall, a quad light above and a glass triangle."""
    from ptmi import core
    w = core.hittable_list()
    w.add(core.Sphere.stationary(core.vec3(0, -100.5, -1), 100, _lamb(GREY)))
    w.add(core.Sphere.stationary(core.vec3(*centre), 0.5, ball or _lamb(RED)))
    w.add(core.Sphere.stationary(core.vec3(1.2, 0, -1), 0.5, core.metal(core.vec3(.8, .6, .2), 0.2)))
    w.add(core.quad(core.vec3(-2, -0.5, -3), core.vec3(4, 0, 0), core.vec3(0, 2, 0), wall or _lamb(GREY)))
    w.add(core.quad(core.vec3(-1, 2.5, -2), core.vec3(2, 0, 0), core.vec3(0, 0, 2), light or _light((6, 6, 6))))
    w.add(core.triangle(core.vec3(-1.5, -0.5, 0), core.vec3(-0.5, -0.5, 0), core.vec3(-1, 0.5, 0),
                        core.dielectric(1.5)))
    return w


def _camera(spp=4):
    cam = mo.slide_camera_object()
    cam.samples_per_pixel = spp
    return cam


def _renderer(tmp_path, world=None, spp=4, **kw):
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import MI355XRenderer
    random.seed(99)
    r = (InteractiveViewer if kw else MI355XRenderer)(world or _world(), _camera(spp), str(tmp_path / 'm.png'), **kw)
    r.background_color = (0.05, 0.05, 0.08)
    r._upload_camera()
    return r


def test_renderer_update_restarts_the_image_and_equals_a_new_renderer(tmp_path):
    from ptmi import core
    r = _renderer(tmp_path)
    tables = r.arrays.perlin
    caller = r.arrays
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    g0 = host(r.guides()).copy()
    assert float(r.accum.abs().sum()) > 0
    glass, checker = core.dielectric(1.5), core.lambertian(
        core.checker_texture.from_colors(0.5, core.color(.2, .3, .1), core.color(.9, .9, .9)))
    assert r.update_materials(spheres={1: glass}, quads={WALL: checker}, triangles={0: _lamb(BLUE)}) is None
    assert r.scene_revision == 1 and r.current_sample == 0 and r.adaptive_passes == []
    assert not host(r.accum).any() and not host(r.stats).any() and r.denoised is None
    assert r.primitives['spheres'][1].material is glass and r.primitives['quads'][WALL].mat is checker
    assert not host(r.guides()).tobytes() == g0.tobytes()  # retraced: the albedo guides changed
    assert mh.mats_equal(caller, sd.compile_world(_world(), tables))  # the arrays the renderer was made from
    edited = _world(ball=glass, wall=checker)
    edited.objects[5].mat = _lamb(BLUE)
    full = sd.compile_world(edited, tables)
    assert r.arrays is r.dscene.arrays and mh.mats_equal(r.arrays, full) and uh.arrays_equal(r.arrays, full)
    assert uh.layouts_equal(r.dscene.layout, sd.pack_device(full)) == []
    fresh = _renderer(tmp_path, edited)
    for x in (r, fresh):
        x.integrator.render_mk(x.frame, x.accum, 0, 8)
    assert host(r.accum).tobytes() == host(fresh.accum).tobytes() and float(r.accum.sum()) > 0
    # what an edit cannot do
    earth = core.lambertian(core.image_texture(sd.load_earthmap()))
    for bad, msg in (({'spheres': {7: glass}}, 'no primitive 7'), ({'spheres': {1: core.vec3(0, 0, 0)}}, 'is not a material'),
                     ({'quads': {WALL: earth}}, 'texels are not resident; .*build a new MI355XRenderer')):
        with pytest.raises(ValueError, match=msg):
            r.update_materials(**bad)
    with pytest.raises(ValueError, match='need keep_history=True'):
        r.update_materials(spheres={1: glass}, max_history=8)
    assert r.scene_revision == 1


def test_rebuild_and_update_primitives_after_a_material_edit(tmp_path):
    from ptmi import core
    r = _renderer(tmp_path)
    tables = r.arrays.perlin
    blue = _lamb(BLUE)
    r.update_materials(spheres={1: blue})
    r.rebuild_bvh()
    full = sd.compile_world(_world(ball=blue), tables)
    assert uh.layouts_equal(r.dscene.layout, sd.pack_device(full)) == [] and mh.mats_equal(r.arrays, full)
    assert_device_is(r.dscene, full)
    # moving the recoloured sphere: the material check compares against the edited record
    r.update_primitives(spheres={1: core.Sphere.stationary(core.vec3(-0.6, 0.3, -0.4), 0.5, blue)})
    moved = sd.compile_world(_world(ball=blue, centre=(-0.6, 0.3, -0.4)), tables)
    assert mh.mats_equal(r.arrays, moved) and r.arrays.sphere_data.tobytes() == moved.sphere_data.tobytes()
    with pytest.raises(ValueError, match='changes material_albedo.*update_materials.*build a new MI355XRenderer'):
        r.update_primitives(spheres={1: core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, _lamb(RED))})
    r.integrator.render_wf(r.frame, r.accum, 0, 2)
    assert np.isfinite(host(r.accum)).all() and float(r.accum.sum()) > 0


def test_keep_history_null_edit_recolour_and_dimmed_light(tmp_path, capsys):
    import torch
    r = _renderer(tmp_path, spp=8)
    r.render_adaptive(target_error=0.0, min_spp=8, max_spp=8)
    cam = sd.camera_upload(r.cam)
    g0, i0 = (t.clone() for t in r.guides_ids())
    a0, s0, rows = r.accum.clone(), r.stats.clone(), r.dscene.primitive_rows()
    sample0 = r.current_sample

    def restore():
        r.accum.copy_(a0)
        r.stats.copy_(s0)
        r.current_sample = sample0

    # (a) a null edit: what reproject_history gives for the unchanged camera with the same guides and ids
    want_a, want_s = (host(t) for t in r.integrator.reproject_moved(cam, cam, g0, g0, i0, i0, rows, a0, s0))
    frac = r.update_materials(spheres={1: r.primitives['spheres'][1].material}, keep_history=True)
    null_a, null_s = host(r.accum).copy(), host(r.stats).copy()
    assert eq(null_a, want_a) and eq(null_s, want_s) and frac == float((want_s[..., 0] > 0).mean()) > 0.9
    assert r.current_sample == sample0 and r.scene_revision == 1
    kept_null = r.render_validated(4)
    # (b) the wall recoloured by an L1 albedo distance of 1.2, above sigma_a = 0.2
    restore()
    assert rh.DEFAULTS['sigma_a'] == 0.2 and float(np.abs(np.array(BLUE) - np.array(GREY)).sum()) > 0.2
    r.update_materials(quads={WALL: _lamb(BLUE)}, keep_history=True)
    g1, i1 = (host(t) for t in r.guides_ids())
    assert eq(i1, host(i0)) and not eq(g1, host(g0))  # the id image carries no class and no material
    rows_np = mo.rows_of(*(host(t)[:n * k.row_floats] for t, n, k in
                           zip(rows, (r.arrays.num_spheres, r.arrays.num_quads, r.arrays.num_triangles), sd.STORAGE)))
    ref_a, ref_s = mo.reproject_moved(cam, cam, g1, host(g0), host(a0), host(s0), i1, host(i0), rows_np, rows_np,
                                      **rh.DEFAULTS)
    a, s = host(r.accum), host(r.stats)
    assert eq(a, ref_a) and eq(s, ref_s)
    wall = i1 == mo.make_id(sd.PRIM_QUAD, mo.device_index(r.arrays)[sd.PRIM_QUAD][WALL])
    assert wall.sum() > 50 and not s[wall].any() and not a[wall].any()
    assert eq(a[~wall], null_a[~wall]) and eq(s[~wall], null_s[~wall]) and (s[~wall][:, 0] > 0).mean() > 0.9
    # (c) the light's emission halved: the validation drops more of the history than after the null edit
    r.update_materials(quads={WALL: _lamb(GREY)})
    restore()
    r.update_materials(quads={LIGHT: _light((3, 3, 3))}, keep_history=True)
    kept_dimmed = r.render_validated(4)
    with capsys.disabled():
        print(f'\nmaterial history kept: null edit {kept_null:.6f}, light halved {kept_dimmed:.6f}')
    assert kept_dimmed < kept_null


# ------------------------------------------------------------------ the viewer
def test_viewer_drops_its_history_and_a_motion_viewer_carries_it(tmp_path):
    v = _renderer(tmp_path, temporal=True)
    v.render_interactive()
    v.update_materials(spheres={1: _lamb(BLUE)})
    assert v.history_fraction is None and not host(v.accum).any() and v._history is None
    assert v.current_sample == 0 and v.scene_revision == 1
    m = _renderer(tmp_path, temporal=True, motion=True, max_history=8)
    m.render_interactive()
    cam = sd.camera_upload(m.cam)
    a0, s0 = m.accum.clone(), m.stats.clone()
    g0, i0 = m.guides_ids()
    rows0 = m.dscene.primitive_rows()
    m.update_materials(spheres={1: _lamb(BLUE)}, media=None)
    g1, i1 = m.guides_ids()
    want_a, want_s = m.integrator.reproject_moved(cam, cam, g1, g0, i1, i0, rows0, a0, s0, max_history=8)
    assert eq(host(m.accum), host(want_a)) and eq(host(m.stats), host(want_s))
    assert m.history_fraction == float((host(want_s)[..., 0] > 0).mean()) and 0.3 < m.history_fraction < 1.0
    ball = host(i1) == mo.make_id(sd.PRIM_SPHERE, mo.device_index(m.arrays)[sd.PRIM_SPHERE][1])
    assert ball.sum() > 20 and not host(m.stats)[ball].any()  # the recoloured ball starts over
    assert m.scene_revision == 1 and m.primitives['spheres'][1].material is not None
