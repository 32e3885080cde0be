"""GPU: the motion ABI (include/ptmi_motion.h) bit for bit against its numpy f32
reference (motion_helpers). The id form of the guide trace on `coverage` and
`cornell_box`, 48 x 27 and a ragged 37 x 21 frame, stack and stackless walk;
ptmi_reproject_moved across one update of `coverage` and on the unmoved scene;
a sphere that slides across a fixed view and takes its history along; hostile
ids; NaN history; a side stream and a captured graph; the renderer's
keep_history and the viewer's motion option."""
import ctypes as C
import random

import numpy as np
import pytest

import motion_helpers as mh
import reproject_helpers as rh

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = mh.W, mh.H


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def frame_of(cam, bg=(0, 0, 0), traversal='stack'):
    from ptmi import device
    return device.make_frame(cam, bg, 50, 0, cam['width'], cam['height'], traversal=traversal)


def device_rows(ds):
    """motion_helpers.rows_of dict of what the device scene holds."""
    lay = ds.layout
    torch_rows = [t.cpu().numpy()[:n * k] for t, n, k in ((ds.t_spheres, lay.num_spheres, 4),
                                                         (ds.t_quads, lay.num_quads, 16),
                                                         (ds.t_tris, lay.num_triangles, 12))]
    return mh.rows_of(*torch_rows)


def rows_equal(a, b):
    return all(a[t].tobytes() == b[t].tobytes() for t in a)


_scenes = {}


def updated_scene(key):
    """(Integrator on the updated scene, previous rows) of a motion_helpers
    case ('coverage', 'coverage_still', 'slide'): the case's base scene on the
    device, its rows copied, then its edits applied. Made once per module."""
    from ptmi import device
    if key not in _scenes:
        case = {'coverage': lambda: mh.coverage_case(True), 'coverage_still': lambda: mh.coverage_case(False),
                'slide': mh.slide_case}[key]()
        ds = device.DeviceScene.from_arrays(case['sa_prev'])
        assert rows_equal(device_rows(ds), case['rows_prev'])
        prev_rows = ds.primitive_rows()
        if case['edits']:
            ds.update_primitives(**case['edits'])
        assert rows_equal(device_rows(ds), case['rows_cur'])
        assert all(eq(host(t), host(s)) for t, s in zip(ds.primitive_rows(), (ds.t_spheres, ds.t_quads, ds.t_tris)))
        _scenes[key] = (device.Integrator(ds), prev_rows, case)
    return _scenes[key]


def run(key, case=None, match_ids=True, **prm):
    integ, prev_rows, base = updated_scene(key)
    c = case or base
    a, s = integ.reproject_moved(c['cur'], c['prev'], dev(c['guides_cur']), dev(c['guides_prev']), dev(c['ids_cur']),
                                 dev(c['ids_prev']), prev_rows, dev(c['accum']), dev(c['stats']), match_ids=match_ids,
                                 **prm)
    return host(a), host(s)


# ---------------------------------------------------------------- the id trace
@pytest.mark.parametrize('traversal', ['stack', 'stackless'])
@pytest.mark.parametrize('size', [(W, H), mh.RAGGED])
@pytest.mark.parametrize('name', ['coverage', 'cornell_box'])
def test_trace_guides_ids_equals_reference(name, size, traversal):
    import torch
    from ptmi import device
    sa, _, bg = rh.scene(name, 48)
    cam = mh.camera(name, *size)
    w, h = size
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    fr = frame_of(cam, bg, traversal)
    plain = host(integ.trace_guides(fr))
    # a sentinel border: a row before and a row after the id image
    buf = torch.full(((h + 2) * w,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    guides = torch.full((h, w, 8), -1.0, dtype=torch.float32, device='cuda')
    ids = buf[w:w + h * w].view(h, w)
    out = integ.trace_guides_ids(fr, out=(guides, ids))
    assert out[0] is guides and out[1] is ids
    assert host(guides).tobytes() == plain.tobytes()  # byte for byte ptmi_guide_trace's
    want_g, want_i = mh.traced(name, sa, 'base', cam, traversal)
    assert eq(plain, want_g)
    got = host(buf)
    assert (got[:w] == 0x5a5a5a5a).all() and (got[-w:] == 0x5a5a5a5a).all()
    bad = np.argwhere(host(ids) != want_i)
    assert not len(bad), (len(bad), bad[:4].tolist())
    assert (want_i >= 0).any() and (name == 'cornell_box' or (want_i < 0).any())
    g2, i2 = integ.trace_guides_ids(fr)  # made by the call
    assert eq(host(g2), plain) and eq(host(i2), want_i) and i2.dtype == torch.int32


# ---------------------------------------------------------------- moved and unmoved scenes
@pytest.mark.parametrize('match_ids', [True, False])
def test_reproject_moved_equals_reference_after_an_update(match_ids):
    """`coverage`: a sphere, a quad and a triangle moved in one update, the camera orbited one degree."""
    integ, prev_rows, case = updated_scene('coverage')
    ref_a, ref_s, det = mh.reference(case, match_ids=match_ids, details=True)
    a, s = run('coverage', match_ids=match_ids)
    assert eq(s, ref_s)
    assert eq(a, ref_a)
    rh.check_properties(a, s, det, 32.0)
    assert (s[..., 0] > 0).mean() > 0.9
    # the traces of the updated device scene are the case's: ids and guides of the oracle on the refit arrays
    g, i = integ.trace_guides_ids(frame_of(case['cur'], rh.scene('coverage', 48)[2]))
    assert eq(host(i), case['ids_cur']) and eq(host(g), case['guides_cur'])


def test_reproject_moved_on_the_unmoved_scene_is_reproject():
    integ, prev_rows, case = updated_scene('coverage_still')
    for match_ids in (True, False):
        ref_a, ref_s, det = mh.reference(case, match_ids=match_ids, details=True)
        a, s = run('coverage_still', match_ids=match_ids)
        assert eq(s, ref_s) and eq(a, ref_a)
        rh.check_properties(a, s, det, 32.0)
    pa, ps = integ.reproject(case['cur'], case['prev'], dev(case['guides_cur']), dev(case['guides_prev']),
                             dev(case['accum']), dev(case['stats']))
    assert host(pa).tobytes() == a.tobytes() and host(ps).tobytes() == s.tobytes()  # flags 0: byte for byte
    # what reproject_moved adds to reproject's arguments is checked like them, before the call
    import torch
    from ptmi import _lib
    t = {k: dev(case[k]) for k in ('guides_cur', 'guides_prev', 'ids_cur', 'ids_prev', 'accum', 'stats')}
    out = torch.full((H, W, 3), -1.0, device='cuda'), torch.full((H, W, 4), -1.0, device='cuda')

    def rejected(match, rows=prev_rows, **bad):
        v = dict(t, **bad)
        with pytest.raises(_lib.PtmiError, match=match):
            integ.reproject_moved(case['cur'], case['prev'], v['guides_cur'], v['guides_prev'], v['ids_cur'],
                                  v['ids_prev'], rows, v['accum'], v['stats'], out=out)

    rejected('ids must be', ids_cur=t['ids_cur'].float())
    rejected('ids must be', ids_prev=t['ids_prev'].cpu())
    rejected('ids must be', ids_cur=t['ids_cur'][:, :W - 1])
    rejected('guides must be', guides_prev=t['stats'])
    rejected(r'prev_rows must be \(spheres, quads, tris\)', rows=prev_rows[:2])
    rejected('prev_rows: spheres must be', rows=(prev_rows[0][:-4], prev_rows[1], prev_rows[2]))
    rejected('prev_rows: quads must be', rows=(prev_rows[0], prev_rows[1].double(), prev_rows[2]))
    rejected('prev_rows: tris must be', rows=(prev_rows[0], prev_rows[1], prev_rows[2].cpu()))
    assert (host(out[0]) == -1).all() and (host(out[1]) == -1).all()


def test_a_sliding_sphere_takes_its_history_along_on_the_device():
    """tests/test_motion_abi.py's property, with the same asserted counts: the
    guides and ids are the device's own traces before and after the update."""
    integ, prev_rows, case = updated_scene('slide')
    ds = integ.scene
    # the device's traces: after the update here, before it on a scene of its own
    from ptmi import device
    before = device.Integrator(device.DeviceScene.from_arrays(case['sa_prev']))
    fr = frame_of(case['cur'])
    g0, i0 = before.trace_guides_ids(fr)
    g1, i1 = integ.trace_guides_ids(fr)
    assert eq(host(i0), case['ids_prev']) and eq(host(i1), case['ids_cur'])
    assert eq(host(g0), case['guides_prev']) and eq(host(g1), case['guides_cur'])
    a0, s0 = dev(case['accum']), dev(case['stats'])
    a, s = integ.reproject_moved(case['cur'], case['prev'], g1, g0, i1, i0, prev_rows, a0, s0)
    pa, ps = integ.reproject(case['cur'], case['prev'], g1, g0, a0, s0)
    ref_a, ref_s, det = mh.reference(case, details=True)
    a, s = host(a), host(s)
    assert eq(a, ref_a) and eq(s, ref_s)
    counts = mh.check_slide(case, a, s, host(pa), host(ps), det)
    assert counts == (mh.SLIDE_SPHERE_PIXELS, mh.SLIDE_INTERIOR_PIXELS) == (113, 75)
    assert ds.layout.num_spheres == 2


# ---------------------------------------------------------------- hostile ids, NaN history
def test_hostile_ids_read_no_row():
    """Ids that name no row, in the current and in the previous id image,
    through ctypes on valid buffers: a prim equal to its type's count, type
    nibble 7, INT32_MIN and -1. Those pixels are zeros, those taps are
    skipped, everything else is the reference's; the range check comes before
    the row address is formed, so the run ends clean."""
    import torch
    from ptmi import _lib, motion, temporal
    integ, prev_rows, base = updated_scene('coverage')
    counts = {t: len(r) for t, r in base['rows_cur'].items()}
    hostile = [mh.make_id(t, counts[t]) for t in (mh.SPHERE, mh.QUAD, mh.TRIANGLE)] + \
        [np.int32(7 << 28 | 1), np.int32(-2 ** 31), np.int32(-1), np.int32(3 << 28), np.int32(0x0fffffff)]
    ids_cur, ids_prev = base['ids_cur'].copy(), base['ids_prev'].copy()
    hit = base['guides_cur'][..., 7] != 0
    spots = np.argwhere(hit)[::max(1, int(hit.sum()) // 40)][:40]
    for k, (y, x) in enumerate(spots):
        ids_cur[y, x] = hostile[k % len(hostile)]
    for k, (y, x) in enumerate(np.argwhere(base['guides_prev'][..., 7] != 0)[7::29]):
        ids_prev[y, x] = hostile[k % len(hostile)]
    case = dict(base, ids_cur=ids_cur, ids_prev=ids_prev)
    lib = motion.load()
    t = {k: dev(case[k]) for k in ('guides_cur', 'guides_prev', 'accum', 'stats', 'ids_cur', 'ids_prev')}
    for match_ids in (True, False):
        ref_a, ref_s = mh.reference(case, match_ids=match_ids)
        out_a, out_s = torch.full((H, W, 3), -1.0, device='cuda'), torch.full((H, W, 4), -1.0, device='cuda')
        prm = motion.params(match_ids=match_ids)
        cur, prev = temporal.camera(case['cur']), temporal.camera(case['prev'])
        rc = lib.ptmi_reproject_moved(C.byref(cur), C.byref(prev), t['guides_cur'].data_ptr(),
                                      t['guides_prev'].data_ptr(), t['accum'].data_ptr(), t['stats'].data_ptr(),
                                      t['ids_cur'].data_ptr(), t['ids_prev'].data_ptr(), integ.scene.view,
                                      prev_rows[0].data_ptr(), prev_rows[1].data_ptr(), prev_rows[2].data_ptr(), W, H,
                                      C.byref(prm), out_a.data_ptr(), out_s.data_ptr(), None)
        assert rc == _lib.PTMI_OK, lib.ptmi_last_error()
        a, s = host(out_a), host(out_s)
        for y, x in spots:
            assert not a[y, x].any() and not s[y, x].any()
        assert eq(a, ref_a) and eq(s, ref_s)


def test_nan_history_does_not_spread():
    integ, prev_rows, base = updated_scene('coverage')
    accum = base['accum'].copy()
    accum[::3, 1::4, 0] = np.nan
    accum[1::5, ::7, 2] = np.inf
    case = dict(base, accum=accum)
    ref_a, ref_s, det = mh.reference(case, details=True)
    a, s = run('coverage', case)
    assert eq(a, ref_a) and eq(s, ref_s)
    rh.check_properties(a, s, det, 32.0)
    assert np.isfinite(a).all() and np.isfinite(s).all() and (s[..., 0] > 0).mean() > 0.5


# ---------------------------------------------------------------- a side stream, a captured graph
def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the capture calls."""
    with open('/proc/self/maps') as f:
        paths = {line.split()[-1] for line in f if 'libamdhip64' in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_side_stream_and_graph_capture_give_the_same_bytes():
    import torch
    integ, prev_rows, case = updated_scene('coverage')
    t = {k: dev(case[k]) for k in ('guides_cur', 'guides_prev', 'accum', 'stats', 'ids_cur', 'ids_prev')}

    def launch(out, stream=None):
        return integ.reproject_moved(case['cur'], case['prev'], t['guides_cur'], t['guides_prev'], t['ids_cur'],
                                     t['ids_prev'], prev_rows, t['accum'], t['stats'], out=out, stream=stream)

    def fresh():
        return torch.full((H, W, 3), -1.0, device='cuda'), torch.full((H, W, 4), -1.0, device='cuda')

    want = launch(fresh())
    want = host(want[0]), host(want[1])
    assert eq(want[0], mh.reference(case)[0])
    side = torch.cuda.Stream()
    out = fresh()
    torch.cuda.synchronize()
    r = launch(out, side)
    side.synchronize()
    assert r[0] is out[0] and r[1] is out[1]
    assert out[0].cpu().numpy().tobytes() == want[0].tobytes() and out[1].cpu().numpy().tobytes() == want[1].tobytes()
    # one call captured into a graph: a single kernel node, so no parallel branches; its replay writes the same bytes
    hip = _hip_runtime()
    out = fresh()
    torch.cuda.synchronize()
    stream = C.c_void_p(side.cuda_stream)
    graph, graph_exec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
    try:
        launch(out, side)
    finally:
        rc = hip.hipStreamEndCapture(stream, C.byref(graph))
    assert rc == 0 and graph.value
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1
    node, kind = (C.c_void_p * 1)(), C.c_int(-1)
    assert hip.hipGraphGetNodes(graph, node, C.byref(n)) == 0
    assert hip.hipGraphNodeGetType(C.c_void_p(node[0]), C.byref(kind)) == 0 and kind.value == 0  # a kernel node
    side.synchronize()
    assert (out[1].cpu().numpy() == -1).all()  # captured, not run
    assert hip.hipGraphInstantiate(C.byref(graph_exec), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(graph_exec, stream) == 0
    side.synchronize()
    assert out[0].cpu().numpy().tobytes() == want[0].tobytes() and out[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0


# ---------------------------------------------------------------- renderer and viewer
def _renderer(tmp_path, spp=4, **kw):
    """An MI355XRenderer of the sliding-sphere scene, 48 x 27; with viewer options, an InteractiveViewer."""
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import MI355XRenderer
    cls = InteractiveViewer if kw else MI355XRenderer
    random.seed(1234)
    cam = mh.slide_camera_object()
    cam.samples_per_pixel = spp
    r = cls(mh.slide_world(mh.SLIDE_FROM), cam, str(tmp_path / f'm{len(kw)}.png'), **kw)
    r.background_color = (0.7, 0.8, 1.0)
    return r


def _sphere_at(r, centre):
    from ptmi import core
    return core.Sphere.stationary(core.vec3(*centre), mh.SLIDE_RADIUS, r.primitives['spheres'][1].material)


def test_renderer_update_without_keep_history_clears_the_image(tmp_path):
    r = _renderer(tmp_path)
    with pytest.raises(ValueError, match='keep_history=True needs stats'):
        r.update_primitives(spheres={1: _sphere_at(r, mh.SLIDE_TO)}, keep_history=True)
    assert r.scene_revision == 0
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    assert float(r.accum.abs().sum()) > 0
    assert r.update_primitives(spheres={1: _sphere_at(r, mh.SLIDE_TO)}, keep_history=False) is None
    assert not host(r.accum).any() and not host(r.stats).any() and r.current_sample == 0 and r.scene_revision == 1
    with pytest.raises(ValueError, match='need keep_history=True'):
        r.update_primitives(spheres={1: _sphere_at(r, mh.SLIDE_FROM)}, max_history=8)


def test_renderer_update_with_keep_history_equals_reference(tmp_path):
    from ptmi import scene_data as sd
    r = _renderer(tmp_path)
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    r.denoise()
    cam = sd.camera_upload(r.cam)
    g0, i0 = (host(t).copy() for t in r.guides_ids())
    assert r.guides() is r.guides_ids()[0] and eq(g0, host(r.integrator.trace_guides(r.frame)))
    a0, s0, rows0 = host(r.accum).copy(), host(r.stats).copy(), device_rows(r.dscene)
    assert r._tiles['n'] == 0
    with pytest.raises(ValueError, match='go together'):
        r.reproject_history(cam, r.guides(), prev_ids=r.guides_ids()[1])
    frac = r.update_primitives(spheres={1: _sphere_at(r, (0.2, 0.3, -1.0))}, keep_history=True, max_history=16)
    assert 0.0 < frac <= 1.0 and r.scene_revision == 1 and r.denoised is None and r.current_sample == 4
    g1, i1 = (host(t) for t in r.guides_ids())
    assert not eq(i1, i0)
    ref_a, ref_s = mh.reproject_moved(cam, cam, g1, g0, a0, s0, i1, i0, device_rows(r.dscene), rows0,
                                      **dict(rh.DEFAULTS, max_history=16.0))
    a, s = host(r.accum), host(r.stats)
    assert eq(a, ref_a) and eq(s, ref_s)
    n = s[..., 0]
    assert eq(n, np.floor(n)) and n.max() <= 16 and frac == float((n > 0).mean())
    sid = mh.make_id(mh.SPHERE, mh.device_index(r.arrays)[mh.SPHERE][1])
    assert (n[i1 == sid] > 0).mean() > 0.5  # the moved sphere kept history
    ntiles = r._tiles['grid'][0] * r._tiles['grid'][1]
    assert r._tiles['n'] == ntiles and int(r._tiles['state'].sum()) == ntiles  # the tile states have restarted
    # a pass of the adaptive path on top of the carried history
    integ = r.integrator
    integ.render_mk_stats(r.frame, r.accum, r.stats, r.current_sample, 2)
    integ.tile_update(r.frame, r.stats, 0.05, 4, 64, r._tiles)
    n2 = host(r.stats)[..., 0]
    assert eq(n2, n + 2) and np.isfinite(host(r.accum)).all()


class _Event:
    def __init__(self, x, y):
        self.x, self.y = x, y


def test_motion_viewer_keeps_its_history_across_updates(tmp_path):
    from ptmi import scene_data as sd
    from ptmi.interactive_viewer import InteractiveViewer
    with pytest.raises(ValueError, match='needs temporal=True'):
        InteractiveViewer(mh.slide_world(mh.SLIDE_FROM), mh.slide_camera_object(), str(tmp_path / 'x.png'),
                          motion=True)
    spp = 4
    v = _renderer(tmp_path, spp=spp, temporal=True, motion=True, max_history=8)
    assert isinstance(v, InteractiveViewer) and v.motion
    v.render_interactive()
    assert v.next_sample_index == spp and (v.sample_count_map() == spp).all()
    cam = sd.camera_upload(v.cam)
    a0, s0 = v.accum.clone(), v.stats.clone()
    g0, i0 = v.guides_ids()
    rows0 = v.dscene.primitive_rows()
    v.update_primitives(spheres={1: _sphere_at(v, (-0.4, 0.3, -1.0))})
    assert v.history_fraction is not None and v.history_fraction > 0.5
    assert v.current_sample == 0 and v.next_sample_index == spp and v.scene_revision == 1
    # a second update with no sample in between: the rendered history again, not the reprojected one
    v.update_primitives(spheres={1: _sphere_at(v, (0.2, 0.3, -1.0))})
    g1, i1 = v.guides_ids()
    want_a, want_s = v.integrator.reproject_moved(cam, cam, g1, g0, i1, i0, rows0, a0, s0, max_history=8)
    assert eq(host(v.accum), host(want_a)) and eq(host(v.stats), host(want_s))
    assert v.history_fraction == float((host(want_s)[..., 0] > 0).mean()) > 0.5
    # a camera move, still with no sample in between: from the rendered history, across the updates
    v.camera_update_interval = 0.0
    v.on_mouse_down(_Event(10, 10))
    v.on_mouse_drag(_Event(13, 11))
    cam2 = sd.camera_upload(v.cam)
    g2, i2 = v.guides_ids()
    want_a, want_s = v.integrator.reproject_moved(cam2, cam, g2, g0, i2, i0, rows0, a0, s0, max_history=8)
    assert eq(host(v.accum), host(want_a)) and eq(host(v.stats), host(want_s))
    assert v.next_sample_index == spp
    v.render_interactive()  # continues from next_sample_index on top of the carried history
    for i in range(spp, 2 * spp):
        v.integrator.render_mk_stats(v.frame, want_a, want_s, i, 1)
    assert eq(host(v.accum), host(want_a)) and eq(host(v.stats), host(want_s))
    assert v.next_sample_index == 2 * spp
    counts = v.sample_count_map()
    assert counts.min() == spp and spp < counts.max() <= 8 + spp
    assert v._history.rows is None  # the new render is the history, of the scene as it is


def test_viewer_without_motion_drops_its_history(tmp_path):
    v = _renderer(tmp_path, spp=4, temporal=True)
    assert v.motion is False
    v.render_interactive()
    v.update_primitives(spheres={1: _sphere_at(v, mh.SLIDE_TO)})
    assert v.history_fraction is None and not host(v.accum).any() and v._history is None
    assert v.current_sample == 0
