"""GPU tests of the rigid-body pose ABI and of blur and animation by rigid bodies
(include/ptmi_rigid.h, ptmi/rigid.py): after DeviceScene.pose(t)
the device holds byte for byte what update_primitives of the posed objects'
records leaves, with linear tracks in the same scene too; unpose restores every
byte; the shell hint of a body that turns comes from the swept box; a blurred
render is, slice by slice, the CPU oracle's on the numpy-refit arrays; and the
renderer and the viewer go through the same sequence, checkpoint the bodies and
leave the device at the rest scene."""
import random

import numpy as np
import pytest

import parity_helpers as ph
import pose_helpers as psh
import rigid_helpers as rh
import update_helpers as uh
from ptmi import core, pose, rigid, scene_data as sd, update

pytestmark = pytest.mark.gpu
f32 = np.float32
WIDTH = 48
TENSORS = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris')
FORMS = {'per_level': 0, 'one_group': update.ONE_GROUP}
TIMES = [0.0, 1.0, 1.0 / 3.0, pose.vdc(5)]
BOX = range(6)  # the coverage scene's medium box: quads 0 .. 5, centre (-1.6, 0.4, 2.4)
NO_TRACKS = {'spheres': {}, 'quads': {}, 'triangles': {}}


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def install(ds, prims, bodies, tracks=None, t_range=(0.0, 1.0)):
    ds.set_tracks(*pose.track_records(tracks or NO_TRACKS), t_range=t_range,
                  rigid=(bodies, rigid.body_records(bodies, prims)))


def scene_and_bodies(case):
    """(SceneArrays, primitive lists, bodies) of a buffers case."""
    if case == 'coverage':  # two bodies: the quad box with a sphere, turning and moving; 59 triangles tumbling
        sa, prims = ph.fixture('coverage', WIDTH), psh.scene_prims('coverage', WIDTH)
        bodies = [rh.scene_body('coverage', WIDTH, spheres=[1], quads=BOX, turn=0.7, displacement=(0.1, 0.3, -0.2)),
                  rh.scene_body('coverage', WIDTH, triangles=range(3, 62), axis=(1.0, -2.0, 0.5), turn=-2.0)]
        return sa, prims, bodies
    if case == 'cornell_mesh_fog':  # one body: every mesh triangle, 3000 entries
        sa, prims = ph.fixture('cornell_mesh_fog', WIDTH), psh.scene_prims('cornell_mesh_fog', WIDTH)
        assert sa.num_triangles == 3000
        return sa, prims, [rh.scene_body('cornell_mesh_fog', WIDTH, triangles=range(3000), turn=1.2,
                                         displacement=(5.0, 10.0, -5.0), pivot=(278.0, 140.0, 278.0))]
    # vol2: 16 bodies of three small spheres each; the fog shell is in none
    sa, prims = ph.fixture('vol2_final_scene'), psh.scene_prims('vol2_final_scene')
    rng = np.random.default_rng(3)
    shell = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, int(sd.leaf_depths(sa.bvh).max()))])
    picked = [int(i) for i in rng.choice([i for i in range(sa.num_spheres) if i != shell], 48, replace=False)]
    bodies = [rh.scene_body('vol2_final_scene', spheres=picked[3 * b:3 * b + 3], axis=rng.uniform(-1, 1, 3),
                            turn=float(rng.uniform(-3, 3)), displacement=rng.uniform(-20, 20, 3)) for b in range(16)]
    return sa, prims, bodies


# ------------------------------------------------------------------ 1. buffers
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('case', ['coverage', 'cornell_mesh_fog', 'vol2_final_scene'])
def test_posed_buffers_equal_an_update_with_the_posed_records(case, form):
    sa, prims, bodies = scene_and_bodies(case)
    ds, other = new_scene(sa), new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, prims, bodies)
    assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None  # set_tracks leaves the rest scene
    for n, t in enumerate(TIMES):
        ds.pose(t, flags=FORMS[form])
        assert ds.posed == t
        records = rigid.posed_records(bodies, prims, t)
        other.update_primitives(*records, flags=FORMS[form])
        got, want = psh.device_image(ds), psh.device_image(other)
        assert psh.images_differ(got, want, TENSORS + ('view_root',)) == [], t
        assert psh.images_differ(got, rest, ('mats', 'texels')) == []
        assert ds._upd['root'].cpu().numpy().tobytes() == got['view_root'].tobytes()
        if n == 2:  # and that is pack_device of the numpy refit
            ref = sd.pack_device(uh.refit(sa, psh.as_edits(records)))
            for k in TENSORS:
                assert got[k].tobytes() == np.asarray(getattr(ref, k), f32).tobytes(), (k, t)
            assert psh.images_differ(got, rest, TENSORS)  # something did move
    # the mirror and the layout kept describing the rest scene
    assert uh.layouts_equal(ds.layout, sd.pack_device(sa)) == [] and uh.arrays_equal(ds.arrays, sa)
    ds.unpose()
    assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 255, 256, 257])
def test_entry_counts_around_a_wave_and_a_block(count):
    sa, prims = ph.fixture('coverage', WIDTH), psh.scene_prims('coverage', WIDTH)
    bodies = [rh.scene_body('coverage', WIDTH, triangles=range(100, 100 + count), axis=(0.3, 1.0, 0.2), turn=1.5,
                            pivot=(-0.2, 1.9, -0.5))]
    ds, other = new_scene(sa), new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, prims, bodies)
    ds.pose(1.0 / 3.0)
    other.update_primitives(*rigid.posed_records(bodies, prims, 1.0 / 3.0))
    got = psh.device_image(ds)
    assert psh.images_differ(got, psh.device_image(other), TENSORS + ('view_root',)) == []
    assert bool(psh.images_differ(got, rest, TENSORS)) == (count > 0)
    moved = np.flatnonzero((got['tris'] != rest['tris']).any(axis=1))
    assert moved.size == count  # and no row beyond the body's
    ds.unpose()
    assert psh.images_differ(psh.device_image(ds), rest) == []


# ------------------------------------------------------------------ 2. skips
def call_with_a_table_of(ds, t, n_bodies):
    """ptmi_pose_rigid on the scene's resident lists with a table said to hold ``n_bodies`` bodies."""
    import ctypes as C
    import torch
    from ptmi import _lib, device
    st, tr = ds._update_state(), ds._tracks
    arg = device._list_args(rigid.RigidList, tr['rigid'])
    topo = ds._topology(st, None)
    with torch.cuda.device(ds.device):
        _lib.check(rigid.load().ptmi_pose_rigid(ds.view, arg[0], arg[1], arg[2], rigid.body_table(tr['bodies'], t),
                                                n_bodies, C.byref(topo), st['root'].data_ptr(), None),
                   'ptmi_pose_rigid')
        torch.cuda.synchronize()


def test_entries_that_name_nothing_are_skipped_and_the_others_applied():
    import torch
    sa, prims = ph.fixture('coverage', WIDTH), psh.scene_prims('coverage', WIDTH)
    n = 10
    kw = dict(axis=(0.0, 0.0, 1.0), turn=0.9, pivot=(-0.2, 1.9, -0.5))
    bodies = [rh.scene_body('coverage', WIDTH, triangles=range(0, n, 2), **kw),
              rh.scene_body('coverage', WIDTH, triangles=range(1, n, 2), displacement=(0.0, 0.5, 0.0), **kw)]
    ds, other = new_scene(sa), new_scene(sa)
    install(ds, prims, bodies)
    ints, _, body = ds._tracks['rigid_keep']  # device rows then leaves; the rest records; the body of every entry
    assert ints.numel() == 2 * n and body.cpu().numpy().tolist() == [0, 1] * (n // 2)
    host, bhost = ints.cpu().numpy().copy(), body.cpu().numpy().copy()
    a_quad_leaf = int(uh.leaf_of(sa, sd.PRIM_QUAD)[0])
    host[0] = -1                      # prim below the range
    host[1] = sa.num_triangles        # prim past the range
    host[n + 2] = sa.num_bvh_nodes    # leaf past the range
    host[n + 3] = -5                  # leaf below the range
    host[n + 4] = host[n + 5]         # the leaf of another triangle
    host[n + 6] = a_quad_leaf         # the leaf of a primitive of another type
    bhost[7] = 2                      # a body past the table
    bhost[8] = -1                     # a body below it
    ints.copy_(torch.from_numpy(host))
    body.copy_(torch.from_numpy(bhost))
    kept = [rigid.Body(b.pivot, b.axis, b.turn, b.displacement, triangles=idx) for b, idx in zip(bodies, ([], [5, 9]))]
    ds.pose(0.75)
    other.update_primitives(*rigid.posed_records(kept, prims, 0.75))
    assert psh.images_differ(psh.device_image(ds), psh.device_image(other), TENSORS + ('view_root',)) == []
    assert psh.images_differ(psh.device_image(ds), psh.device_image(new_scene(sa)), TENSORS)
    ds.unpose()
    # a table said to hold one body: the entries of body 1 are skipped, those of body 0 applied
    fresh, third = new_scene(sa), new_scene(sa)
    install(fresh, prims, bodies)
    call_with_a_table_of(fresh, 0.75, 1)
    third.update_primitives(*rigid.posed_records(bodies[:1], prims, 0.75))
    assert psh.images_differ(psh.device_image(fresh), psh.device_image(third), TENSORS) == []
    call_with_a_table_of(fresh, 0.75, 0)  # nobody: a pure refit of what is there
    assert psh.images_differ(psh.device_image(fresh), psh.device_image(third), TENSORS) == []


# ------------------------------------------------------------------ 3. linear tracks and bodies in one scene
@pytest.mark.parametrize('form', list(FORMS))
def test_linear_tracks_and_bodies_in_one_scene(form):
    sa, prims, bodies = scene_and_bodies('coverage')
    moving = [i for i, s in enumerate(prims['spheres']) if not pose._is_zero(s.center.direction)]
    tracks = psh.scene_tracks('coverage', WIDTH, spheres=moving + [2], quads=[6, 8], triangles=range(200, 230), seed=9)
    ds, other = new_scene(sa), new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, prims, bodies, tracks)
    calls = []
    for name in ('pose_call', 'rigid_call'):
        real = getattr(ds, name)
        setattr(ds, name, (lambda name, real: lambda *a, **k: calls.append(name) or real(*a, **k))(name, real))
    for t in (0.0, 0.625, 1.0):
        ds.pose(t, flags=FORMS[form])
        other.update_primitives(*as_arguments(rh.merged_edits(prims, bodies, tracks, t)), flags=FORMS[form])
        got = psh.device_image(ds)
        assert psh.images_differ(got, psh.device_image(other), TENSORS + ('view_root',)) == [], t
    assert calls == ['pose_call', 'rigid_call'] * 3  # two calls per pose, in this order
    ds.unpose()
    assert psh.images_differ(psh.device_image(ds), rest) == []
    # a primitive with a linear track may not be in a body
    with pytest.raises(ValueError, match='a primitive is in a rigid body and has a linear track'):
        install(ds, prims, bodies, psh.scene_tracks('coverage', WIDTH, quads=[3], seed=1))


def as_arguments(edits):
    """update_helpers.refit's dict as update_primitives' three arguments."""
    return tuple(edits.get(k) for k in psh.KINDS)


# ------------------------------------------------------------------ 4. unpose
def test_unpose_restores_every_byte_and_the_view():
    sa, prims = psh.small_world('zero')  # a quad with Q.x = -0.0 among them
    assert np.signbit(sa.quads['quad_Q'][0, 0]) and sa.quads['quad_Q'][0, 0] == 0.0
    bodies = [rigid.Body(core.vec3(0, 0, 0), core.vec3(0, 1, 0), 0.0, quads=[0], triangles=[0]),
              rigid.Body(core.vec3(3, 0, -2), core.vec3(1, 1, 0), 2.0, core.vec3(0, 0.5, 0), spheres=[1, 2])]
    ds = new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, prims, bodies)
    for t in (0.0, 0.625, 1.0):
        ds.pose(t)
        posed = psh.device_image(ds)
        assert psh.images_differ(posed, rest, TENSORS), t
        # body 0 neither turns nor moves: every row float of its primitives compares == to the rest row ...
        assert np.array_equal(posed['quads'], rest['quads']) and np.array_equal(posed['tris'], rest['tris'])
        # ... though not every bit: the -0.0 became +0.0
        diff = posed['quads'].view(np.uint32) ^ rest['quads'].view(np.uint32)
        assert diff.ravel()[4] == 0x80000000 and set(np.unique(diff).tolist()) <= {0, 0x80000000}
        ds.unpose()
        assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None
        assert uh.layouts_equal(ds.layout, sd.pack_device(sa)) == []
    ds.unpose()  # a second unpose has nothing to do
    assert psh.images_differ(psh.device_image(ds), rest) == []


# ------------------------------------------------------------------ 5. the shell hint
def test_the_posed_shell_hint_on_vol2():
    sa, prims = ph.fixture('vol2_final_scene'), psh.scene_prims('vol2_final_scene')
    ds = new_scene(sa)
    hint = int(ds.view.shell)
    shell_sphere = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, ds.layout.max_leaf_depth)])
    radius = float(sa.sphere_data[shell_sphere, 3])
    assert hint != 0 and radius == 5000.0
    others = [i for i in range(sa.num_spheres) if i != shell_sphere]
    # a small body far from the shell, turning about its own middle: kept
    small = [rh.scene_body('vol2_final_scene', spheres=others[:10], turn=3.0, displacement=(10.0, 0.0, 5.0))]
    install(ds, prims, small)
    assert ds._tracks['shell'] == hint
    ds.pose(0.5)
    assert ds.view.shell == hint  # stays while posed
    ds.unpose()
    # the same spheres about a pivot 0.6 R away: the swept sphere reaches the shell, though at no single time
    # within this shutter does a sphere get anywhere near it: the bound is conservative
    wide = [rh.scene_body('vol2_final_scene', spheres=others[:10], turn=1e-3, pivot=(0.6 * radius, 0.0, 0.0))]
    install(ds, prims, wide)
    assert ds._tracks['shell'] == 0 and ds.view.shell == hint  # the rest scene keeps its own
    ds.pose(0.0)
    assert ds.view.shell == 0
    ds.unpose()
    assert ds.view.shell == hint
    # with turn == 0 the two-ends union is used, and the same pivot does no harm
    still = [rigid.Body(wide[0].pivot, wide[0].axis, 0.0, core.vec3(1.0, 0.0, 0.0), spheres=others[:10])]
    install(ds, prims, still)
    assert ds._tracks['shell'] == hint
    # the shell sphere itself in a body
    install(ds, prims, [rh.scene_body('vol2_final_scene', spheres=[shell_sphere], turn=0.1)])
    assert ds._tracks['shell'] == 0
    ds.pose(1.0)
    assert ds.view.shell == 0
    ds.unpose()
    assert ds.view.shell == hint and psh.images_differ(psh.device_image(ds), psh.device_image(new_scene(sa))) == []


# ------------------------------------------------------------------ 6. render parity
def parity_case(name):
    """(scene inputs, primitive lists, bodies, linear tracks, window)."""
    if name == 'coverage':  # the quad box turning 20 degrees, 600 triangles of the torus tumbling; the moving sphere
        scene = ph.scene_inputs('coverage', WIDTH)
        prims = psh.scene_prims('coverage', WIDTH)
        bodies = [rh.scene_body('coverage', WIDTH, quads=BOX, turn=np.radians(20.0), pivot=(-1.6, 0.4, 2.4)),
                  rh.scene_body('coverage', WIDTH, triangles=range(2, 602), axis=(0.2, 1.0, 0.1), turn=1.0,
                                displacement=(0.3, 0.0, 0.0), pivot=(-0.2, 1.9, -0.5))]
        return scene, prims, bodies, pose.tracks_of(prims), (0, 0, WIDTH, scene[1]['height'])
    # the captured camera; the 32 x 32 window of it that shows the front of the cluster of small spheres, and the
    # ten of them whose centres project nearest its middle
    scene = ph.scene_inputs('vol2_final_scene', 800)
    sa, prims = scene[0], psh.scene_prims('vol2_final_scene')
    small = [581, 612, 618, 614, 579, 680, 650, 580, 715, 615]
    assert all(sa.sphere_data[i, 3] == 10.0 for i in small)
    bodies = [rh.scene_body('vol2_final_scene', spheres=small, axis=(0.0, 1.0, 0.3), turn=2.0,
                            displacement=(15.0, 0.0, 0.0))]
    return scene, prims, bodies, None, (465, 333, 32, 32)


_oracle_cache = {}


def oracle_of(name, variant, traversal):
    """The oracle's blurred image and counters of a parity case: 8 spp, slice_spp 2, computed once."""
    key = (name, variant, traversal)
    if key not in _oracle_cache:
        scene, prims, bodies, tracks, window = parity_case(name)
        _oracle_cache[key] = rh.oracle_blurred(scene, variant, window, prims, bodies, tracks, (0.0, 1.0), 2, 0, 8,
                                               traversal)
    return _oracle_cache[key]


def gpu_blurred(name, variant, traversal, chunks=((0, 8),), overlap=False):
    import torch
    from ptmi import device
    (sa, cam, bg), prims, bodies, tracks, window = parity_case(name)
    W, H = cam['width'], cam['height']
    ds = new_scene(sa)
    install(ds, prims, bodies, tracks)
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, bg, 50, 0, W, H, window, traversal=traversal)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    fn = integ.render_mk if variant == 'mk' else integ.render_wf
    kw = {'overlap': True} if overlap else {}
    for b, c in chunks:
        integ.render_posed(fn, fr, b, c, 2, (0.0, 1.0), acc, **kw)
        assert ds.posed is not None
    integ.unpose()
    torch.cuda.synchronize()
    assert ds.posed is None
    return acc.cpu().numpy(), integ.read_counters()


@pytest.mark.parametrize('variant,traversal', [('mk', 'stack'), ('wf', 'stack'), ('mk', 'stackless')])
@pytest.mark.parametrize('name', ['coverage', 'vol2_final_scene'])
def test_blurred_render_equals_the_oracle_slice_by_slice(name, variant, traversal):
    o, ost = oracle_of(name, variant, traversal)
    g, cnt = gpu_blurred(name, variant, traversal)
    linf, exact = ph.compare(g, o, 8)
    assert linf == 0.0 and exact == 1.0, (linf, exact)
    assert cnt == {k: int(v) for k, v in ost.items()}
    assert np.isfinite(g).all() and g.sum() > 0
    # and it is a blur: the unposed render of the same samples differs
    scene = parity_case(name)[0]
    still, _, _ = ph.gpu_render(name, scene[1]['width'], variant, parity_case(name)[4], 0, 8, traversal=traversal)
    assert not np.array_equal(still, g)


@pytest.mark.parametrize('name', ['coverage', 'vol2_final_scene'])
def test_chunked_and_overlapped_blurred_renders_are_identical(name):
    o, ost = oracle_of(name, 'mk', 'stack')
    counters = {k: int(v) for k, v in ost.items()}
    for chunks, overlap in ((((0, 3), (3, 5)), False), (((0, 8),), True), (((0, 3), (3, 5)), True)):
        g, cnt = gpu_blurred(name, 'mk', 'stack', chunks, overlap)
        assert np.array_equal(g, o) and cnt == counters, (chunks, overlap)
    g, cnt = gpu_blurred(name, 'wf', 'stack', ((0, 3), (3, 5)))
    o, ost = oracle_of(name, 'wf', 'stack')
    assert np.array_equal(g, o) and cnt == {k: int(v) for k, v in ost.items()}


# ------------------------------------------------------------------ 7. the renderer
def coverage_renderer(tmp_path, spp=8, width=WIDTH, viewer=False, **kw):
    from coverage_scene import coverage_scene
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import MI355XRenderer
    random.seed(1234)
    sc = coverage_scene(width)
    sc.cam.samples_per_pixel = spp
    r = (InteractiveViewer if viewer else MI355XRenderer)(sc.world, sc.cam, str(tmp_path / 'out.png'), **kw)
    r.background_color = sc.background
    r.max_depth = sc.max_depth
    return r


def coverage_bodies(turn=np.radians(20.0)):
    """The box turning ``turn`` over unit time and 400 triangles of the torus tumbling."""
    return [rigid.Body(core.vec3(-1.6, 0.4, 2.4), core.vec3(0, 1, 0), turn, quads=BOX),
            rigid.Body(core.vec3(-0.2, 1.9, -0.5), core.vec3(0.2, 1.0, 0.1), 1.0, core.vec3(0.3, 0.0, 0.0),
                       triangles=range(2, 402))]


def renderer_oracle(r, variant, spp=8, slice_spp=2, shutter=(0.0, 1.0)):
    """The oracle's blurred image for a renderer's scene as it is now: its mirror, its camera, its tracks and bodies."""
    r._upload_camera()
    cam = dict(sd.camera_upload(r.cam), width=r.cam.img_width, height=r.cam.img_height)
    tracks = pose.tracks_of(r.primitives, r._motion)
    window = (0, 0, r.cam.img_width, r.cam.img_height)
    return rh.oracle_blurred((r.dscene.arrays, cam, r.background_color), variant, window, r.primitives, r._bodies,
                             tracks, shutter, slice_spp, 0, spp)[0]


def assert_device_is_the_mirror(r):
    ds = r.dscene
    assert ds.posed is None
    want = sd.pack_device(ds.arrays)
    got = psh.device_image(ds)
    for k in TENSORS + ('mats',):
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    assert got['shell'] == want.shell
    assert got['view_root'].tobytes() == np.concatenate([want.root_min, want.root_max]).astype(f32).tobytes()


def test_the_entry_points_render_with_bodies(tmp_path):
    r = coverage_renderer(tmp_path, shutter=(0, 1), slice_spp=2)
    r.render(enable_preview=False)
    no_bodies = r.accum.cpu().numpy().copy()
    r.set_bodies(coverage_bodies())
    r.render(enable_preview=False)
    mk = r.accum.cpu().numpy().copy()
    assert not np.array_equal(mk, no_bodies) and np.array_equal(mk, renderer_oracle(r, 'mk'))
    assert len(r.dscene._tracks['indices'][sd.PRIM_TRIANGLE]) == 400 and len(r.dscene._tracks['bodies']) == 2
    assert_device_is_the_mirror(r)
    r.render_wavefront(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), renderer_oracle(r, 'wf'))
    assert_device_is_the_mirror(r)
    # render_sample goes the same way: sample s at slice s // slice_spp
    r.clear_accumulation_buffer()
    for s in range(8):
        r.render_sample(s)
    assert np.array_equal(r.accum.cpu().numpy(), mk)
    # render_adaptive, both integrators (listed tiles included), and render_validated
    for integrator, variant in (('megakernel', 'mk'), ('wavefront', 'wf')):
        r.render_adaptive(integrator=integrator, target_error=0.0, pass_spp=3, min_spp=2, max_spp=8)
        assert np.array_equal(r.accum.cpu().numpy(), renderer_oracle(r, variant))
        assert_device_is_the_mirror(r)
    r.render_adaptive(target_error=0.05, pass_spp=3, min_spp=3, max_spp=12)
    assert_device_is_the_mirror(r)
    kept = r.render_validated(4)
    assert 0.0 <= kept <= 1.0
    assert_device_is_the_mirror(r)
    # set_bodies, then a rebuild between two blurred renders: the tracks are remade on the new tree
    r.render(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), mk)
    r.rebuild_bvh()
    assert r.dscene._tracks is None
    r.render(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), mk)
    assert_device_is_the_mirror(r)
    # an update of a body's primitive drops the tracks and the next render poses the new rest object
    r.dscene.update_primitives(quads=uh.current(r.dscene.arrays, 'quads', [0]))
    assert r.dscene._tracks is None
    # [] clears them
    r.set_bodies([])
    r.render(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), no_bodies)
    # a set_motion that names a body's primitive is refused when the tracks are made
    r.set_bodies(coverage_bodies())
    r.set_motion(quads={0: core.vec3(1, 0, 0)})
    with pytest.raises(ValueError, match=r'quads\[0\] is in a body and moves linearly'):
        r.render(enable_preview=False)


def test_adaptive_render_with_bodies_resumes_bit_identically_and_checkpoints_refuse_other_bodies(tmp_path):
    kw = dict(target_error=0.0, pass_spp=3, min_spp=2, max_spp=8)  # passes of 3 straddle the slices of 2

    def make(bodies, **more):
        r = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2, **more)
        r.set_bodies(bodies)
        return r

    for integrator in ('megakernel', 'wavefront'):
        full = make(coverage_bodies())
        full.render_adaptive(integrator=integrator, **kw)
        a, s = full.accum.cpu().numpy().copy(), full.stats.cpu().numpy().copy()
        ck = str(tmp_path / f'{integrator}.npz')
        part = make(coverage_bodies())
        part.checkpoint_path = ck
        part.render_adaptive(integrator=integrator, **kw)
        with np.load(ck) as z:
            assert int(z['next_sample']) == 6 and str(z['bodies']) == rigid.digest(coverage_bodies()) != ''
        res = make(coverage_bodies())
        res.load_checkpoint(ck)
        res.render_adaptive(integrator=integrator, resume=True, **kw)
        assert np.array_equal(res.accum.cpu().numpy(), a) and np.array_equal(res.stats.cpu().numpy(), s)
    # other bodies, or none, are another render
    r = make(coverage_bodies(), spp=2)
    r.render(enable_preview=False)
    ck = str(tmp_path / 'ck.npz')
    r.save_checkpoint(ck)
    for bodies in (coverage_bodies(turn=0.5), coverage_bodies()[:1], []):
        other = make(bodies, spp=4)
        other.load_checkpoint(ck)
        with pytest.raises(ValueError, match='another render: bodies differs'):
            other.render(resume=True)
    same = make(coverage_bodies(), spp=4)
    same.load_checkpoint(ck)
    same.render(resume=True)
    # a checkpoint without the key is one of a render without bodies
    with np.load(ck) as z:
        old = {k: z[k] for k in z.files if k != 'bodies'}
    np.savez(str(tmp_path / 'old.npz'), **old)
    with_bodies = make(coverage_bodies(), spp=4)
    with_bodies.load_checkpoint(str(tmp_path / 'old.npz'))
    with pytest.raises(ValueError, match='another render: bodies differs'):
        with_bodies.render(resume=True)
    none = make([], spp=4)
    none.load_checkpoint(str(tmp_path / 'old.npz'))
    none.render(resume=True)


def test_no_bodies_makes_no_rigid_call(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(rigid, 'load', lambda: calls.append('load') or pytest.fail('rigid.load() without bodies'))
    r = coverage_renderer(tmp_path, spp=2)
    r.render(enable_preview=False)
    r.shutter, r.slice_spp = (0.0, 1.0), 1  # the moving sphere's linear track alone
    r.render(enable_preview=False)
    r.render_wavefront(enable_preview=False)
    r.render_adaptive(target_error=0.0, pass_spp=2, min_spp=2, max_spp=2)
    r.render_sample(0)
    r.set_bodies([])
    r.render(enable_preview=False)
    assert calls == [] and r.dscene._tracks['rigid'] == {} and r.dscene._tracks['bodies'] == []
    assert r.dscene.posed is None
    # and bodies without a shutter make no call either
    r.shutter = None
    r.set_bodies(coverage_bodies())
    r.render(enable_preview=False)
    assert calls == []


def test_the_animation_loop_renders_each_frame_at_its_pose(tmp_path):
    """shutter = (t, t): frame k is the still image of update_primitives(the posed objects at t_k) on a fresh renderer."""
    r = coverage_renderer(tmp_path, spp=4, slice_spp=2)
    body = rigid.Body(core.vec3(-0.2, 1.9, -0.5), core.vec3(0, 1, 0), 2.0, core.vec3(0.0, 0.1, 0.0),
                      triangles=range(2, len(r.primitives['triangles'])))  # all triangles of the torus mesh
    r.set_bodies([body])
    dt, frames = 0.125, []
    for k in (0, 1, 3):
        r.shutter = (k * dt, k * dt)
        r.render(enable_preview=False)
        frames.append(r.accum.cpu().numpy().copy())
        assert_device_is_the_mirror(r)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    fresh = coverage_renderer(tmp_path, spp=4)
    at = rigid.body_at(body, 3 * dt)
    moving = {i: pose.posed_object('spheres', s, s.center.direction, 3 * dt)  # the scene's own moving sphere is posed too
              for i, s in enumerate(fresh.primitives['spheres']) if not pose._is_zero(s.center.direction)}
    assert len(moving) == 1
    fresh.update_primitives(spheres=moving,
                            triangles={i: rigid.posed_object('triangles', fresh.primitives['triangles'][i], at)
                                       for i in body.triangles})
    fresh.render(enable_preview=False)
    assert np.array_equal(fresh.accum.cpu().numpy(), frames[2])


# ------------------------------------------------------------------ 8. errors
def test_rigid_errors():
    from ptmi import _lib
    sa, prims = psh.small_world('zero')
    bodies = [rigid.Body(core.vec3(0, 0, 0), core.vec3(0, 1, 0), 1.0, spheres=[1], quads=[0])]
    ds = new_scene(sa)
    with pytest.raises(_lib.PtmiError, match='set_tracks'):
        ds.rigid_call(0.5)
    install(ds, prims, bodies, t_range=(0.25, 0.75))
    for t in (0.0, 0.8, float('nan')):
        with pytest.raises(ValueError, match='outside'):
            ds.pose(t)
    assert ds.posed is None
    ds.pose(0.5)
    rows = uh.current(sa, 'spheres', [1])
    for call in (lambda: ds.update_primitives(spheres=rows), ds.rebuild, ds.tree_growth, ds.primitive_rows,
                 lambda: install(ds, prims, bodies)):
        with pytest.raises(_lib.PtmiError, match=r'the scene is posed at t = 0\.5: unpose\(\) first'):
            call()
    ds.unpose()
    ds.update_primitives(spheres=rows)  # names a body's primitive: the tracks are dropped
    assert ds._tracks is None
    install(ds, prims, bodies)
    ds.update_primitives(spheres=uh.current(sa, 'spheres', [2]))  # in no body: they stay
    assert ds._tracks is not None and ds._tracks['bodies'] == bodies
    ds.rebuild()
    assert ds._tracks is None
    with pytest.raises(ValueError, match='spheres: an index is outside'):
        ds.set_tracks(rigid=([rigid.Body(core.vec3(0, 0, 0), core.vec3(0, 1, 0), 1.0, spheres=[7])],
                             ((np.array([7]), np.zeros(1, np.int32), np.zeros((1, 3))), None, None)))
    with pytest.raises(ValueError, match='at most 16 bodies'):
        ds.set_tracks(rigid=([bodies[0]] * 17, (None, None, None)))


# ------------------------------------------------------------------ 9. the viewer
def test_viewer_progressive_steps_equal_the_renderer(tmp_path):
    v = coverage_renderer(tmp_path, spp=2, width=32, viewer=True, shutter=(0.0, 1.0), slice_spp=1)
    v.set_bodies(coverage_bodies())
    v.render_interactive()  # two steps of one sample: slices 0 and 1, t = 0 and 1/2
    assert v.current_sample == 2 and len(v.sample_times) == 2
    r = coverage_renderer(tmp_path, spp=2, width=32, shutter=(0.0, 1.0), slice_spp=1)
    r.set_bodies(coverage_bodies())
    r.render(enable_preview=False)
    assert np.array_equal(v.accum.cpu().numpy(), r.accum.cpu().numpy())
    assert np.array_equal(r.accum.cpu().numpy(), renderer_oracle(r, 'mk', spp=2, slice_spp=1))
    assert_device_is_the_mirror(v)
