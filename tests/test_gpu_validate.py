"""GPU: the history-validation ABI (include/ptmi_validate.h) bit for bit against
its numpy f32 reference (validate_helpers). The kernel on every frame, radius and
synthetic input of the CPU test; a side stream and a captured graph; with and
without the weight image; MI355XRenderer.render_validated on the sliding sphere
against the numpy composition of reproject_moved, oracle samples in Welford
order and the validation, with both integrators; the quality orderings of the
CPU test from that run; the viewer's validate option across an update and an
orbit step, and a viewer without it against today's path."""
import ctypes as C
import random

import numpy as np
import pytest

import adaptive_helpers as ah
import motion_helpers as mh
import reproject_helpers as rh
import validate_helpers as vh

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = mh.W, mh.H


def eq(a, b):
    return vh.same_bits(np.asarray(a), np.asarray(b))


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


_integ = []


def integrator():
    """An Integrator on some resident scene (the call reads none): made once per module."""
    from ptmi import device
    if not _integ:
        _integ.append(device.Integrator(device.DeviceScene.from_arrays(mh.slide_case()['sa_prev'])))
    return _integ[0]


def run(images, weight=True, **prm):
    import torch
    t = [dev(a) for a in images]
    wt = torch.full(t[1].shape[:2], -1.0, device='cuda') if weight else None
    a, s = integrator().validate_history(*t, weight=wt, **prm)
    return host(a), host(s), (host(wt) if weight else None)


# ---------------------------------------------------------------- the kernel against numpy
@pytest.mark.parametrize('radius', vh.RADII)
@pytest.mark.parametrize('size', vh.FRAMES)
def test_kernel_equals_reference(size, radius):
    images = vh.synthetic(*size)
    want = vh.validate(*images, radius=radius)
    got = run(images, radius=radius)
    for g, x, what in zip(got, want, ('accum', 'stats', 'weight')):
        assert eq(g, x), what
    # the same images without the weight image
    assert all(eq(g, x) for g, x in zip(run(images, weight=False, radius=radius)[:2], want[:2]))


def test_kernel_equals_reference_with_other_k_and_on_hostile_statistics():
    images = vh.synthetic(48, 27, seed=1)
    assert all(eq(g, x) for g, x in zip(run(images, radius=2, k_lo=0.0, k_hi=0.75),
                                        vh.validate(*images, radius=2, k_lo=0.0, k_hi=0.75)))
    rng = np.random.default_rng(11)
    w, h = 19, 7
    pool = np.array([0, -0.0, 1, 2, 3.5, -4, 32, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan], f32)
    images = [rng.choice(pool, (h, w, c)).astype(f32) for c in (3, 4, 3, 4)]
    assert all(eq(g, x) for g, x in zip(run(images, radius=1), vh.validate(*images, radius=1)))


def test_identities_on_the_device():
    ha, hs, fa, fs = vh.synthetic(37, 21)
    a, s, wt = run((np.zeros_like(ha), np.zeros_like(hs), fa, fs))
    assert a.tobytes() == fa.tobytes() and s.tobytes() == fs.tobytes() and not wt.any()
    clean = np.isfinite(ha).all(-1) & np.isfinite(hs).all(-1)
    ha, hs = np.where(clean[..., None], ha, 0).astype(f32), np.where(clean[..., None], hs, 0).astype(f32)
    a, s, wt = run((ha, hs, np.zeros_like(fa), np.zeros_like(fs)))
    assert a.tobytes() == ha.tobytes() and s.tobytes() == hs.tobytes()


def test_host_layer_rejects_what_the_contract_rejects():
    import torch
    from ptmi import _lib
    integ = integrator()
    t = [dev(a) for a in vh.synthetic(16, 16)]
    with pytest.raises(_lib.PtmiError, match='out_accum aliases hist_accum'):
        integ.validate_history(*t, out=(t[0], torch.empty_like(t[1])))
    with pytest.raises(_lib.PtmiError, match='radius must be in'):
        integ.validate_history(*t, radius=8)
    with pytest.raises(_lib.PtmiError, match='k_hi must be above k_lo'):
        integ.validate_history(*t, k_lo=3.0, k_hi=3.0)
    with pytest.raises(_lib.PtmiError, match='stats must be'):
        integ.validate_history(t[0], t[1], t[2], t[3][:8])
    with pytest.raises(_lib.PtmiError, match='var must be'):
        integ.validate_history(*t, weight=torch.empty((16, 16), dtype=torch.float64, device='cuda'))


# ---------------------------------------------------------------- a side stream, a captured graph
def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for the capture calls."""
    with open('/proc/self/maps') as f:
        paths = {line.split()[-1] for line in f if 'libamdhip64' in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_side_stream_and_graph_capture_give_the_same_bytes():
    import torch
    integ = integrator()
    images = vh.synthetic(W, H)
    t = [dev(a) for a in images]

    def launch(out, stream=None):
        return integ.validate_history(*t, out=out[:2], weight=out[2], stream=stream)

    def fresh():
        return (torch.full((H, W, 3), -1.0, device='cuda'), torch.full((H, W, 4), -1.0, device='cuda'),
                torch.full((H, W), -1.0, device='cuda'))

    def same(out, want):
        return all(eq(host(o), x) for o, x in zip(out, want))

    want = vh.validate(*images)
    out = fresh()
    launch(out)
    assert same(out, want)
    side = torch.cuda.Stream()
    out = fresh()
    torch.cuda.synchronize()
    r = launch(out, side)
    side.synchronize()
    assert r[0] is out[0] and r[1] is out[1] and same(out, want)
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
    assert same(out, want)
    assert hip.hipGraphExecDestroy(graph_exec) == 0 and hip.hipGraphDestroy(graph) == 0


# ---------------------------------------------------------------- renderer and viewer
def _renderer(tmp_path, spp=4, centre=mh.SLIDE_FROM, **kw):
    """An MI355XRenderer of the sliding-sphere scene, 48 x 27; with viewer options, an InteractiveViewer."""
    from ptmi.interactive_viewer import InteractiveViewer
    from ptmi.renderer import MI355XRenderer
    cls = InteractiveViewer if kw else MI355XRenderer
    random.seed(1234)
    cam = mh.slide_camera_object()
    cam.samples_per_pixel = spp
    r = cls(mh.slide_world(centre), cam, str(tmp_path / f'v{len(kw)}.png'), **kw)
    r.background_color = vh.BACKGROUND
    return r


def _sphere_at(r, centre):
    from ptmi import core
    return core.Sphere.stationary(core.vec3(*centre), mh.SLIDE_RADIUS, r.primitives['spheres'][1].material)


def _device_rows(ds):
    lay = ds.layout
    return mh.rows_of(*(t.cpu().numpy()[:n * k] for t, n, k in ((ds.t_spheres, lay.num_spheres, 4),
                                                                (ds.t_quads, lay.num_quads, 16),
                                                                (ds.t_tris, lay.num_triangles, 12))))


def test_render_validated_needs_stats_and_two_samples(tmp_path):
    r = _renderer(tmp_path)
    with pytest.raises(ValueError, match='needs stats'):
        r.render_validated(4)
    r.render_adaptive(target_error=0.0, min_spp=4, max_spp=4)
    for spp in (1, 0):
        with pytest.raises(ValueError, match='spp >= 2'):
            r.render_validated(spp)
    with pytest.raises(ValueError, match='unknown integrator'):
        r.render_validated(4, integrator='both')
    assert r.current_sample == 4 and r.last_history_kept is None
    # on an unmoved scene the fresh samples agree with the history: nearly all of it is kept, counts are whole
    spare = r._history_spare
    kept = r.render_validated(4)
    assert 0.9 < kept <= 1.0 and kept == r.last_history_kept and r.current_sample == 8
    n = host(r.stats)[..., 0]
    assert eq(n, np.floor(n)) and n.min() >= 4 and n.max() == 8 and r._history_spare is spare


@pytest.mark.parametrize('integrator_name,variant', [('megakernel', 'mk'), ('wavefront', 'wf')])
def test_render_validated_after_an_update_equals_the_numpy_composition(tmp_path, integrator_name, variant):
    from ptmi import scene_data as sd
    r = _renderer(tmp_path)
    r.render_adaptive(target_error=0.0, min_spp=8, max_spp=8, integrator=integrator_name)
    r.denoise()
    cam = sd.camera_upload(r.cam)
    g0, i0 = (host(t).copy() for t in r.guides_ids())
    a0, s0, rows0 = host(r.accum).copy(), host(r.stats).copy(), _device_rows(r.dscene)
    frac = r.update_primitives(spheres={1: _sphere_at(r, mh.SLIDE_TO)}, keep_history=True)
    g1, i1 = (host(t) for t in r.guides_ids())
    hist = mh.reproject_moved(cam, cam, g1, g0, a0, s0, i1, i0, _device_rows(r.dscene), rows0, **rh.DEFAULTS)
    assert eq(host(r.accum), hist[0]) and eq(host(r.stats), hist[1]) and 0.5 < frac < 1.0
    spare = r._history_spare
    kept = r.render_validated(4, integrator=integrator_name)
    fresh = vh.stats_render(vh.oracle_cols(r.arrays, cam, 8, 4, variant))
    want_a, want_s, _, det = vh.validate(*hist, *fresh, details=True)
    assert eq(host(r.accum), want_a) and eq(host(r.stats), want_s)
    assert kept == vh.kept_fraction(det['n_v'], det['n_h']) == r.last_history_kept and 0.3 < kept < 1.0
    assert r.current_sample == 12 and r.denoised is None and r._history_spare is spare
    ntiles = r._tiles['grid'][0] * r._tiles['grid'][1]
    assert r._tiles['n'] == ntiles and int(r._tiles['state'].sum()) == ntiles  # the tile states have restarted
    # other parameters reach the kernel; a second call reuses the scratch pairs and validates the merged state
    before = (host(r.accum).copy(), host(r.stats).copy())
    scratch = {id(t) for pair in (r._validate_scratch['fresh'], r._validate_scratch['out']) for t in pair} | \
        {id(r.accum), id(r.stats)}
    r.render_validated(2, integrator=integrator_name, radius=1, k_lo=1.0, k_hi=2.0)
    fresh = vh.stats_render(vh.oracle_cols(r.arrays, cam, 12, 2, variant))
    want = vh.validate(*before, *fresh, radius=1, k_lo=1.0, k_hi=2.0)
    assert eq(host(r.accum), want[0]) and eq(host(r.stats), want[1]) and r.current_sample == 14
    assert {id(t) for pair in (r._validate_scratch['fresh'], r._validate_scratch['out']) for t in pair} | \
        {id(r.accum), id(r.stats)} == scratch


def test_quality_orderings_on_the_device(tmp_path):
    """The CPU test's quality case run by the renderer: 64 samples, the move
    with keep_history (capped at 32), render_validated(4); the control moves
    nothing. The device state equals the numpy composition bit for bit, so the
    orderings are the CPU test's."""
    q = vh.quality_case()
    figures = {}
    for name, centre in (('moved', mh.SLIDE_TO), ('control', mh.SLIDE_FROM)):
        hist_ref, cols, truth, changed = q[name]
        r = _renderer(tmp_path)
        r.render_adaptive(target_error=0.0, min_spp=vh.HISTORY_SAMPLES, max_spp=vh.HISTORY_SAMPLES)
        r.update_primitives(spheres={1: _sphere_at(r, centre)}, keep_history=True, max_history=vh.MAX_HISTORY)
        hist = (host(r.accum).copy(), host(r.stats).copy())
        assert eq(hist[0], hist_ref[0]) and eq(hist[1], hist_ref[1])
        plain = (r.accum.clone(), r.stats.clone())  # today's path: the fresh samples on top of the history
        r.integrator.render_mk_stats(r.frame, plain[0], plain[1], vh.FRESH_BEGIN, vh.FRESH_SPP)
        kept = r.render_validated(vh.FRESH_SPP)
        fresh = tuple(host(t) for t in r._validate_scratch['fresh'])
        ref_fresh = vh.stats_render(cols)
        assert eq(fresh[0], ref_fresh[0]) and eq(fresh[1], ref_fresh[1])
        figures[name] = vh.orderings(hist, fresh, (host(plain[0]), host(plain[1])), (host(r.accum), host(r.stats)),
                                     kept, truth, changed)
        np.testing.assert_equal(figures[name], vh.reference_orderings(q[name]))  # (a NaN, of no pixels, equals a NaN)
    vh.check_orderings(figures['moved'], figures['control'])


class _Event:
    def __init__(self, x, y):
        self.x, self.y = x, y


def _drag(v):
    v.camera_update_interval = 0.0
    v.on_mouse_down(_Event(10, 10))
    v.on_mouse_drag(_Event(13, 11))
    v.on_mouse_up(_Event(13, 11))


def test_validating_viewer_across_an_update_and_an_orbit_step(tmp_path):
    import torch
    from ptmi.interactive_viewer import InteractiveViewer
    with pytest.raises(ValueError, match='needs temporal=True'):
        InteractiveViewer(mh.slide_world(mh.SLIDE_FROM), mh.slide_camera_object(), str(tmp_path / 'x.png'),
                          validate=True)
    with pytest.raises(ValueError, match='validate_spp must be at least 2'):
        InteractiveViewer(mh.slide_world(mh.SLIDE_FROM), mh.slide_camera_object(), str(tmp_path / 'x.png'),
                          temporal=True, validate=True, validate_spp=1)
    spp = 6
    v = _renderer(tmp_path, spp=spp, temporal=True, motion=True, validate=True, validate_spp=4, max_history=8)
    assert v.validate and v.validate_spp == 4
    v.render_interactive()  # no restart before it: nothing to validate
    assert v.last_history_kept is None and (v.sample_count_map() == spp).all()
    integ = v.integrator
    for step, move in enumerate((lambda: v.update_primitives(spheres={1: _sphere_at(v, mh.SLIDE_TO)}), lambda: _drag(v))):
        move()
        begin = v.next_sample_index
        assert v.current_sample == 0 and begin == spp * (step + 1) and v.history_fraction > 0.5
        hist = (v.accum.clone(), v.stats.clone())
        v.render_interactive()
        # the first four samples rendered apart and merged by the validation, the other two on top as ever
        fresh = (torch.zeros_like(hist[0]), torch.zeros_like(hist[1]))
        integ.render_mk_stats(v.frame, *fresh, begin, 4)
        want = integ.validate_history(*hist, *fresh)
        for i in range(begin + 4, begin + spp):
            integ.render_mk_stats(v.frame, *want, i, 1)
        assert eq(host(v.accum), host(want[0])) and eq(host(v.stats), host(want[1]))
        assert v.next_sample_index == begin + spp and v.current_sample == spp
        assert 0.0 < v.last_history_kept <= 1.0
        if step == 0:  # the sphere crossed the frame: its old and new shadow say so
            assert v.last_history_kept < 0.99
        counts = v.sample_count_map()
        assert spp <= counts.min() and spp < counts.max() <= 8 + spp  # the fresh samples, and at most the cap more


def test_viewer_without_validate_equals_todays_path(tmp_path):
    from ptmi import scene_data as sd
    spp = 4
    v = _renderer(tmp_path, spp=spp, temporal=True, motion=True, max_history=8)
    assert v.validate is False
    v.render_interactive()
    cam = sd.camera_upload(v.cam)
    a0, s0, rows0 = host(v.accum).copy(), host(v.stats).copy(), _device_rows(v.dscene)
    g0, i0 = (host(t).copy() for t in v.guides_ids())
    assert eq(a0, vh.stats_render(vh.oracle_cols(v.arrays, cam, 0, spp))[0])
    prm = dict(rh.DEFAULTS, max_history=8.0)
    # an update: reproject_moved, then the next samples on top in Welford order
    v.update_primitives(spheres={1: _sphere_at(v, mh.SLIDE_TO)})
    g1, i1 = (host(t).copy() for t in v.guides_ids())
    want = [a.copy() for a in mh.reproject_moved(cam, cam, g1, g0, a0, s0, i1, i0, _device_rows(v.dscene), rows0, **prm)]
    assert eq(host(v.accum), want[0]) and eq(host(v.stats), want[1])
    v.render_interactive()
    ah.accumulate(want[0], want[1], vh.oracle_cols(v.arrays, cam, spp, spp))
    assert eq(host(v.accum), want[0]) and eq(host(v.stats), want[1]) and v.last_history_kept is None
    # an orbit step: the static reprojection, then the next samples
    _drag(v)
    cam2 = sd.camera_upload(v.cam)
    g2 = host(v.guides())
    want = [a.copy() for a in rh.reproject(cam2, cam, g2, g1, want[0], want[1], **prm)]
    assert eq(host(v.accum), want[0]) and eq(host(v.stats), want[1])
    v.render_interactive()
    ah.accumulate(want[0], want[1], vh.oracle_cols(v.arrays, cam2, 2 * spp, spp))
    assert eq(host(v.accum), want[0]) and eq(host(v.stats), want[1]) and v.next_sample_index == 3 * spp
