"""GPU tests of the pose ABI and of motion blur by poses (include/ptmi_pose.h,
ptmi/pose.py): after DeviceScene.pose(t) the device holds byte for
byte what update_primitives of the posed objects' records leaves; unpose
restores every byte; a blurred render is, slice by slice, the CPU oracle's on
the numpy-refit arrays; and the renderer and the viewer go through the same
sequence and leave the device at the rest scene."""
import random

import numpy as np
import pytest

import parity_helpers as ph
import pose_helpers as psh
import update_helpers as uh
from ptmi import core, pose, scene_data as sd, update

pytestmark = pytest.mark.gpu
f32 = np.float32
WIDTH = 48
TENSORS = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris')
FORMS = {'per_level': 0, 'one_group': update.ONE_GROUP}


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def install(ds, tracks, t_range=(0.0, 1.0)):
    ds.set_tracks(*pose.track_records(tracks), t_range=t_range)


def scene_and_tracks(case):
    """(SceneArrays, tracks) of a buffers case; the properties the case is there for are asserted here."""
    if case in ('one_sphere', 'two_primitives'):
        sa, prims = psh.small_world(case)
        tracks = {'spheres': {0: (prims['spheres'][0], core.vec3(0.75, -0.5, 0.25))}, 'quads': {}, 'triangles': {}}
        if case == 'two_primitives':
            tracks['quads'][0] = (prims['quads'][0], core.vec3(0.1, 0.3, -0.2))
        assert sd.pack_device(sa).n_inner == (0 if case == 'one_sphere' else 1)
        return sa, tracks
    if case == 'coverage':  # the moving sphere and two more, three quads, 59 triangles: 65 tracks of every kind
        sa = ph.fixture('coverage', WIDTH)
        prims = psh.scene_prims('coverage', WIDTH)
        moving = [i for i, s in enumerate(prims['spheres']) if not pose._is_zero(s.center.direction)]
        assert len(moving) == 1
        tracks = psh.scene_tracks('coverage', WIDTH, spheres=moving + [1, 2], quads=[0, 2, 5],
                                  triangles=range(3, 62), seed=1)
        assert sum(len(v) for v in tracks.values()) == 65
        return sa, tracks
    if case == 'cornell_mesh_fog':  # every mesh triangle: more than one 1024-lane block
        sa = ph.fixture('cornell_mesh_fog', WIDTH)
        tracks = psh.scene_tracks('cornell_mesh_fog', WIDTH, triangles=range(sa.num_triangles), seed=2, reach=20.0)
        assert sa.num_triangles > 1024
        return sa, tracks
    # vol2: the six large spheres (the image centre shows them) and 34 of the small ones; the fog shell is not tracked
    sa = ph.fixture('vol2_final_scene')
    rng = np.random.default_rng(3)
    shell = int(sa.bvh['bvh_prim_idx'][sd.find_shell(sa, int(sd.leaf_depths(sa.bvh).max()))])
    large = [i for i in range(sa.num_spheres) if i != shell and sa.sphere_data[i, 3] > 20]
    small = [i for i in range(sa.num_spheres) if i != shell and i not in large]
    assert len(large) == 6
    picked = large + [int(i) for i in rng.choice(small, 34, replace=False)]
    return sa, psh.scene_tracks('vol2_final_scene', spheres=picked, seed=3, reach=30.0)


# ------------------------------------------------------------------ 1. buffers
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('case', ['one_sphere', 'two_primitives', 'coverage', 'cornell_mesh_fog', 'vol2_final_scene'])
def test_posed_buffers_equal_an_update_with_the_posed_records(case, form):
    sa, tracks = scene_and_tracks(case)
    ds, other = new_scene(sa), new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, tracks)
    assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None  # set_tracks leaves the rest scene
    for n, t in enumerate(psh.TIMES):
        ds.pose(t, flags=FORMS[form])
        assert ds.posed == t
        records = pose.posed_records(tracks, t)
        other.update_primitives(*records, flags=FORMS[form])
        got, want = psh.device_image(ds), psh.device_image(other)
        assert psh.images_differ(got, want, TENSORS + ('view_root',)) == [], t
        assert psh.images_differ(got, rest, ('mats', 'texels')) == []
        assert ds._upd['root'].cpu().numpy().tobytes() == got['view_root'].tobytes()
        if n % 4 == 1:  # t = 1, vdc(1), vdc(5): and that is pack_device of the numpy refit
            ref = sd.pack_device(uh.refit(sa, psh.as_edits(records)))
            for k in TENSORS:
                assert got[k].tobytes() == np.asarray(getattr(ref, k), f32).tobytes(), (k, t)
            assert psh.images_differ(got, rest, TENSORS)  # something did move
    # the mirror and the layout kept describing the rest scene
    assert uh.layouts_equal(ds.layout, sd.pack_device(sa)) == [] and uh.arrays_equal(ds.arrays, sa)
    ds.unpose()
    assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65])
def test_track_counts_around_a_wave(count):
    sa = ph.fixture('coverage', WIDTH)
    tracks = psh.scene_tracks('coverage', WIDTH, triangles=range(100, 100 + count), seed=count, reach=0.5)
    ds, other = new_scene(sa), new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, tracks)
    ds.pose(1.0 / 3.0)
    other.update_primitives(*pose.posed_records(tracks, 1.0 / 3.0))
    got = psh.device_image(ds)
    assert psh.images_differ(got, psh.device_image(other), TENSORS + ('view_root',)) == []
    assert bool(psh.images_differ(got, rest, TENSORS)) == (count > 0)
    moved = np.flatnonzero((got['tris'] != rest['tris']).any(axis=1))
    assert moved.size == count  # and no row beyond the tracked ones
    ds.unpose()
    assert psh.images_differ(psh.device_image(ds), rest) == []


# ------------------------------------------------------------------ 2. skips
def test_entries_that_name_nothing_are_skipped_and_the_others_applied():
    import torch
    sa = ph.fixture('coverage', WIDTH)
    n = 8
    tracks = psh.scene_tracks('coverage', WIDTH, triangles=range(n), seed=5, reach=0.5)
    ds, other = new_scene(sa), new_scene(sa)
    install(ds, tracks)
    ints = ds._tracks['keep'][0]  # the triangles' device rows, then their leaves
    assert ints.numel() == 2 * n
    host = ints.cpu().numpy().copy()
    a_quad_leaf = int(uh.leaf_of(sa, sd.PRIM_QUAD)[0])
    host[0] = -1                      # prim below the range
    host[1] = sa.num_triangles        # prim past the range
    host[n + 2] = sa.num_bvh_nodes    # leaf past the range
    host[n + 3] = -5                  # leaf below the range
    host[n + 4] = host[n + 5]         # the leaf of another triangle
    host[n + 6] = a_quad_leaf         # the leaf of a primitive of another type
    ints.copy_(torch.from_numpy(host))
    kept = {'spheres': {}, 'quads': {}, 'triangles': {i: tracks['triangles'][i] for i in (5, 7)}}
    ds.pose(0.75)
    other.update_primitives(*pose.posed_records(kept, 0.75))
    assert psh.images_differ(psh.device_image(ds), psh.device_image(other), TENSORS + ('view_root',)) == []
    assert psh.images_differ(psh.device_image(ds), psh.device_image(new_scene(sa)), TENSORS)


# ------------------------------------------------------------------ 3. unpose
@pytest.mark.parametrize('name', ['zero', 'coverage'])
def test_unpose_restores_every_byte_and_the_view(name):
    if name == 'zero':
        sa, prims = psh.small_world('zero')
        tracks = pose.tracks_of(prims, {'quads': {0: core.vec3(1.0, 0.5, 0.25)},
                                        'triangles': {0: core.vec3(-0.5, 0.0, 0.5)}})
        assert np.signbit(sa.quads['quad_Q'][0, 0]) and sa.quads['quad_Q'][0, 0] == 0.0  # the -0.0 quad is tracked
    else:
        sa, tracks = scene_and_tracks('coverage')
    ds = new_scene(sa)
    rest = psh.device_image(ds)
    install(ds, tracks)
    for t in (0.0, 0.625, 1.0):
        ds.pose(t)
        posed = psh.device_image(ds)
        if t or name == 'zero':  # at t = 0 nothing but the sign bit of a -0.0 changes
            assert psh.images_differ(posed, rest, TENSORS), t
        ds.unpose()
        assert psh.images_differ(psh.device_image(ds), rest) == [] and ds.posed is None
        assert uh.layouts_equal(ds.layout, sd.pack_device(sa)) == []
    if name == 'zero':  # pose(0.0) alone would not have done it
        ds.pose(0.0)
        diff = psh.device_image(ds)['quads'].view(np.uint32) ^ rest['quads'].view(np.uint32)
        changed = np.flatnonzero(diff).tolist()  # sign bits alone: Q.x, and D = normal . Q, a sum of zeros here
        assert 4 in changed and set(changed) <= {3, 4} and set(diff.ravel()[changed].tolist()) == {0x80000000}
        ds.unpose()
    ds.unpose()  # a second unpose has nothing to do
    assert psh.images_differ(psh.device_image(ds), rest) == []


# ------------------------------------------------------------------ 4. the shell hint
def test_the_posed_shell_hint_on_vol2():
    sa = ph.fixture('vol2_final_scene')
    ds = new_scene(sa)
    hint = int(ds.view.shell)
    shell_leaf = sd.find_shell(sa, ds.layout.max_leaf_depth)
    shell_sphere = int(sa.bvh['bvh_prim_idx'][shell_leaf])
    radius = float(sa.sphere_data[shell_sphere, 3])
    assert hint != 0 and radius == 5000.0
    others = [i for i in range(sa.num_spheres) if i != shell_sphere]
    near = psh.scene_tracks('vol2_final_scene', spheres=others[:20], seed=4, reach=30.0)
    install(ds, near)
    assert ds._tracks['shell'] == hint
    ds.pose(0.5)
    assert ds.view.shell == hint  # stays while posed
    ds.unpose()
    # one sphere carried beyond R / 2 at t1: the claim fails somewhere in the shutter, so nowhere is it made
    prims = psh.scene_prims('vol2_final_scene')
    far = {'spheres': {others[0]: (prims['spheres'][others[0]], core.vec3(0.6 * radius, 0, 0))}, 'quads': {},
           'triangles': {}}
    install(ds, far)
    assert ds._tracks['shell'] == 0 and ds.view.shell == hint  # the rest scene keeps its own
    ds.pose(0.0)
    assert ds.view.shell == 0
    ds.unpose()
    assert ds.view.shell == hint
    install(ds, far, t_range=(0.0, 0.125))  # within this shutter it stays inside
    assert ds._tracks['shell'] == hint
    # the shell sphere itself tracked
    install(ds, {'spheres': {shell_sphere: (prims['spheres'][shell_sphere], core.vec3(1, 0, 0))}, 'quads': {},
                 'triangles': {}})
    assert ds._tracks['shell'] == 0
    ds.pose(1.0)
    assert ds.view.shell == 0
    ds.unpose()
    assert ds.view.shell == hint and psh.images_differ(psh.device_image(ds), psh.device_image(new_scene(sa))) == []


# ------------------------------------------------------------------ 5. render parity
def parity_case(name):
    if name == 'coverage':
        scene = ph.scene_inputs('coverage', WIDTH)
        _, tracks = scene_and_tracks('coverage')
        H = scene[1]['height']
        return scene, tracks, (0, 0, WIDTH, H)
    scene = ph.scene_inputs('vol2_final_scene', 800)  # the captured camera; a 32 x 32 window of it is rendered
    _, tracks = scene_and_tracks('vol2_final_scene')
    return scene, tracks, (368, 368, 32, 32)


_oracle_cache = {}


def oracle_of(name, variant, traversal):
    """The oracle's blurred image and counters of a parity case: 8 spp, slice_spp 2, computed once."""
    key = (name, variant, traversal)
    if key not in _oracle_cache:
        scene, tracks, window = parity_case(name)
        _oracle_cache[key] = psh.oracle_blurred(scene, variant, window, tracks, (0.0, 1.0), 2, 0, 8, traversal)
    return _oracle_cache[key]


def gpu_blurred(name, variant, traversal, chunks=((0, 8),), overlap=False):
    import torch
    from ptmi import device
    (sa, cam, bg), tracks, window = parity_case(name)
    W, H = cam['width'], cam['height']
    ds = new_scene(sa)
    install(ds, tracks)
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, bg, 50, 0, W, H, window, traversal=traversal)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    fn = integ.render_mk if variant == 'mk' else integ.render_wf
    kw = {'overlap': True} if overlap else {}
    for b, c in chunks:
        integ.render_posed(fn, fr, b, c, 2, (0.0, 1.0), acc, **kw)
        if name == 'vol2_final_scene':
            assert ds.posed is not None and ds.view.shell != 0  # the hint is kept while posed
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
    scene, _, window = parity_case(name)
    still, _, _ = ph.gpu_render(name, scene[1]['width'], variant, window, 0, 8, traversal=traversal)
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


# ------------------------------------------------------------------ 6. the renderer
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


def renderer_oracle(r, variant, spp=8, slice_spp=2, shutter=(0.0, 1.0)):
    """The oracle's blurred image for a renderer's scene as it is now: its mirror, its camera, its tracks."""
    r._upload_camera()
    cam = dict(sd.camera_upload(r.cam), width=r.cam.img_width, height=r.cam.img_height)
    tracks = pose.tracks_of(r.primitives, r._motion)
    window = (0, 0, r.cam.img_width, r.cam.img_height)
    return psh.oracle_blurred((r.dscene.arrays, cam, r.background_color), variant, window, tracks, shutter, slice_spp,
                              0, spp)[0]


def assert_device_is_the_mirror(r):
    ds = r.dscene
    assert ds.posed is None
    want = sd.pack_device(ds.arrays)
    got = psh.device_image(ds)
    for k in TENSORS + ('mats',):
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    assert got['shell'] == want.shell
    assert got['view_root'].tobytes() == np.concatenate([want.root_min, want.root_max]).astype(f32).tobytes()


def test_renderer_with_a_shutter_equals_the_oracle_sum(tmp_path):
    r = coverage_renderer(tmp_path, shutter=(0, 1), slice_spp=2)
    assert r.shutter == (0, 1) and r.slice_spp == 2
    r.render(enable_preview=False)
    mk = r.accum.cpu().numpy().copy()
    assert np.array_equal(mk, renderer_oracle(r, 'mk'))
    assert_device_is_the_mirror(r)
    r.render_wavefront(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), renderer_oracle(r, 'wf'))
    assert_device_is_the_mirror(r)
    # render_sample goes the same way: sample s at slice s // slice_spp
    r.clear_accumulation_buffer()
    for s in range(8):
        r.render_sample(s)
    assert np.array_equal(r.accum.cpu().numpy(), mk)
    # the unblurred renderer differs, and an attribute set later is read at render time
    still = coverage_renderer(tmp_path)
    still.render(enable_preview=False)
    frozen = still.accum.cpu().numpy().copy()
    assert not np.array_equal(frozen, mk)
    still.shutter, still.slice_spp = (0.0, 1.0), 2
    still.render(enable_preview=False)
    assert np.array_equal(still.accum.cpu().numpy(), mk)


def test_renderer_tracks_follow_the_scene(tmp_path):
    r = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2)
    r.render(enable_preview=False)
    base = r.accum.cpu().numpy().copy()
    # set_motion on the mesh changes the image, and the oracle agrees
    mesh = {i: core.vec3(0.0, 0.3, 0.1) for i in range(2, len(r.primitives['triangles']))}
    r.set_motion(triangles=mesh)
    r.render(enable_preview=False)
    moved = r.accum.cpu().numpy().copy()
    assert not np.array_equal(moved, base) and np.array_equal(moved, renderer_oracle(r, 'mk'))
    assert len(r.dscene._tracks['indices'][sd.PRIM_TRIANGLE]) == len(mesh)
    r.set_motion(triangles={i: None for i in mesh})
    r.render(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), base)
    # update_primitives replacing the moving sphere remakes its track
    i = next(i for i, s in enumerate(r.primitives['spheres']) if not pose._is_zero(s.center.direction))
    old = r.primitives['spheres'][i]
    r.update_primitives(spheres={i: core.Sphere.moving(core.vec3(0.3, 0.5, 2.2), core.vec3(-0.4, 0.5, 2.2), 0.4,
                                                       old.material)})
    r.render(enable_preview=False)
    sideways = r.accum.cpu().numpy().copy()
    assert not np.array_equal(sideways, base) and np.array_equal(sideways, renderer_oracle(r, 'mk'))
    rec = r.dscene._tracks['keep'][1].cpu().numpy()[:6]
    assert rec.tolist() == [0.3, 0.5, 2.2, -0.4 - 0.3, 0.0, 0.0]
    assert_device_is_the_mirror(r)
    # a rebuild drops the tracks; the next blurred render remakes them on the new tree: the same image
    r.rebuild_bvh()
    assert r.dscene._tracks is None
    r.render(enable_preview=False)
    assert np.array_equal(r.accum.cpu().numpy(), sideways)
    assert_device_is_the_mirror(r)
    # set_motion on a sphere replaces its direction; None stops it
    r.set_motion(spheres={i: None})
    assert pose.tracks_of(r.primitives, r._motion)['spheres'] == {}
    with pytest.raises(ValueError, match='no primitive 99'):
        r.set_motion(quads={99: core.vec3(1, 0, 0)})
    with pytest.raises(ValueError, match='finite vec3'):
        r.set_motion(quads={0: (1, 0, 0)})


def test_adaptive_render_with_a_shutter_resumes_bit_identically(tmp_path):
    kw = dict(target_error=0.0, pass_spp=3, min_spp=2, max_spp=8)  # passes of 3 straddle the slices of 2
    for integrator in ('megakernel', 'wavefront'):
        full = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2)
        full.render_adaptive(integrator=integrator, **kw)
        a, s = full.accum.cpu().numpy().copy(), full.stats.cpu().numpy().copy()
        assert np.array_equal(a, renderer_oracle(full, 'mk' if integrator == 'megakernel' else 'wf'))
        assert_device_is_the_mirror(full)
        ck = str(tmp_path / f'{integrator}.npz')
        part = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2)
        part.checkpoint_path = ck
        part.render_adaptive(integrator=integrator, **kw)
        with np.load(ck) as z:
            assert int(z['next_sample']) == 6 and z['shutter'].tolist() == [0.0, 1.0] and int(z['slice_spp']) == 2
        res = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2)
        res.load_checkpoint(ck)
        res.render_adaptive(integrator=integrator, resume=True, **kw)
        assert np.array_equal(res.accum.cpu().numpy(), a) and np.array_equal(res.stats.cpu().numpy(), s)
    # listed tiles: a target some tiles reach early; the device is at rest afterwards
    listed = coverage_renderer(tmp_path, shutter=(0.0, 1.0), slice_spp=2)
    listed.render_adaptive(target_error=0.05, pass_spp=3, min_spp=3, max_spp=12)
    assert any(p['active_tiles'] < listed._tiles['grid'][0] * listed._tiles['grid'][1] for p in listed.adaptive_passes)
    assert_device_is_the_mirror(listed)
    # render_validated goes through the poses too
    kept = listed.render_validated(4)
    assert 0.0 <= kept <= 1.0
    assert_device_is_the_mirror(listed)


def test_no_shutter_makes_no_pose_call(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(pose, 'load', lambda: calls.append('load') or pytest.fail('pose.load() without a shutter'))
    r = coverage_renderer(tmp_path, spp=2)
    assert r.shutter is None
    r.render(enable_preview=False)
    r.render_wavefront(enable_preview=False)
    r.render_adaptive(target_error=0.0, pass_spp=2, min_spp=2, max_spp=2)
    r.render_sample(0)
    assert calls == [] and r.dscene._tracks is None and r.dscene.posed is None


# ------------------------------------------------------------------ 7. errors
def test_pose_errors(tmp_path):
    from ptmi import _lib
    sa, tracks = scene_and_tracks('two_primitives')
    ds = new_scene(sa)
    with pytest.raises(_lib.PtmiError, match='set_tracks'):
        ds.pose(0.5)
    install(ds, tracks, t_range=(0.25, 0.75))
    for t in (0.0, 0.8, float('nan')):
        with pytest.raises(ValueError, match='outside'):
            ds.pose(t)
    assert ds.posed is None
    ds.pose(0.5)
    rows = uh.current(sa, 'spheres', [0])
    mat_rows = np.asarray(ds.layout.mats[:1], f32)
    for call in (lambda: ds.update_primitives(spheres=rows), lambda: ds.update_materials(spheres=([0], mat_rows)),
                 ds.rebuild, ds.tree_growth, ds.primitive_rows, lambda: install(ds, tracks)):
        with pytest.raises(_lib.PtmiError, match=r'the scene is posed at t = 0\.5: unpose\(\) first'):
            call()
    ds.unpose()
    ds.update_primitives(spheres=rows)  # names a tracked primitive: the tracks are dropped
    assert ds._tracks is None
    install(ds, tracks)
    ds.update_primitives(quads=uh.current(sa, 'quads', [0]), spheres=None)  # tracked too
    assert ds._tracks is None
    install(ds, {'spheres': tracks['spheres'], 'quads': {}, 'triangles': {}})
    ds.update_primitives(quads=uh.current(sa, 'quads', [0]))  # not tracked: the tracks stay
    assert ds._tracks is not None
    ds.rebuild()
    assert ds._tracks is None
    with pytest.raises(ValueError, match='spheres: an index is outside'):
        ds.set_tracks(spheres=(np.array([5]), np.zeros((1, 6))))
    # checkpoints carry the shutter
    r = coverage_renderer(tmp_path, spp=2, shutter=(0.0, 1.0), slice_spp=2)
    r.render(enable_preview=False)
    ck = str(tmp_path / 'ck.npz')
    r.save_checkpoint(ck)
    for kw, key in ((dict(shutter=(0.0, 0.5), slice_spp=2), 'shutter'), (dict(shutter=(0.0, 1.0), slice_spp=4), 'slice_spp'),
                    (dict(), 'shutter')):
        other = coverage_renderer(tmp_path, spp=4, **kw)
        other.load_checkpoint(ck)
        with pytest.raises(ValueError, match=f'another render: {key} differs'):
            other.render(resume=True)
    with pytest.raises(ValueError, match='shutter must be'):
        coverage_renderer(tmp_path, spp=2, shutter=(1.0, 0.0)).render(enable_preview=False)


# ------------------------------------------------------------------ 8. the viewer
def test_viewer_progressive_steps_equal_the_renderer(tmp_path):
    v = coverage_renderer(tmp_path, spp=2, width=32, viewer=True, shutter=(0.0, 1.0), slice_spp=1)
    v.render_interactive()  # two steps of one sample: slices 0 and 1, t = 0 and 1/2
    assert v.current_sample == 2 and len(v.sample_times) == 2
    r = coverage_renderer(tmp_path, spp=2, width=32, shutter=(0.0, 1.0), slice_spp=1)
    r.render(enable_preview=False)
    assert np.array_equal(v.accum.cpu().numpy(), r.accum.cpu().numpy())
    assert np.array_equal(r.accum.cpu().numpy(), renderer_oracle(r, 'mk', spp=2, slice_spp=1))
    assert_device_is_the_mirror(v)
