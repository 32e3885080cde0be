"""GPU: the guide ABI (include/ptmi_guide.h) bit for bit against its numpy f32
reference (guide_helpers). The guide trace on scenes with an enclosing medium
shell, a fog sphere, medium boxes, every texture and material type, triangles
and a deeper stack rung, and with the stackless traversal; the guided filter on
ragged and tiny synthetic images in both tap forms and on a real 16-spp frame
with its traced guides; the optional arguments, a side stream, the renderer
surface, and the quality condition: at the default parameters the guided
filter is closer to a 4096-spp frame than the unguided one."""
import ctypes as C
import random

import numpy as np
import pytest

import denoise_helpers as dh
import guide_helpers as gh

pytestmark = pytest.mark.gpu

f32 = np.float32


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


# ---------------------------------------------------------------- the guide trace
# vol2: shell, fog sphere, image and Perlin textures, a 4-traversal chain;
# cornell_smoke: medium boxes in front of quads; coverage: every texture and
# material type; cornell_mesh_fog: triangles and the 20-slot stack rung.
TRACE_CASES = [('vol2_final_scene', 64, 'stack'), ('cornell_smoke', 64, 'stack'), ('coverage', 64, 'stack'),
               ('cornell_mesh_fog', 48, 'stack'), ('coverage', 64, 'stackless')]


@pytest.mark.parametrize('name,width,traversal', TRACE_CASES)
def test_trace_guides_equals_reference(name, width, traversal):
    from ptmi import device
    sa, cam, bg = gh.scene_inputs(name, width)
    W, H = cam['width'], cam['height']
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    fr = device.make_frame(cam, bg, 50, 0, W, H, traversal=traversal)
    g = host(integ.trace_guides(fr))
    ref = gh.trace_guides(sa, cam, traversal)
    assert g.shape == ref.shape == (H, W, 8)
    for ch, what in ((slice(7, 8), 'hit'), (slice(3, 4), 'depth'), (slice(0, 3), 'normal'), (slice(4, 7), 'albedo')):
        bad = np.argwhere((g[..., ch] != ref[..., ch]).any(-1))
        assert not len(bad), (what, len(bad), bad[:4].tolist())
    assert np.array_equal(g, ref)
    hit = ref[..., 7] != 0
    assert 0.5 < hit.mean() < 1.0  # hits and misses both occur
    if name == 'vol2_final_scene':  # seen through the shell (and the fog sphere): not one medium albedo
        assert len(np.unique(ref[..., 4:7][hit], axis=0)) > 100
    if name == 'cornell_mesh_fog':
        assert integ.scene.layout.max_leaf_depth + 1 > 16  # past the 16-slot rung


def test_trace_guides_into_a_given_tensor_on_a_side_stream():
    import torch
    from ptmi import _lib, device
    sa, cam, bg = gh.scene_inputs('coverage', 64)
    W, H = cam['width'], cam['height']
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    fr = device.make_frame(cam, bg, 50, 0, W, H)
    ref = host(integ.trace_guides(fr))
    out = torch.full((H, W, 8), -1.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert integ.trace_guides(fr, out=out, stream=side) is out
    side.synchronize()
    assert eq(out.cpu().numpy(), ref)
    with pytest.raises(_lib.PtmiError, match='windowed'):
        integ.trace_guides(device.make_frame(cam, bg, 50, 0, W, H, (0, 0, W, H - 1)))
    with pytest.raises(_lib.PtmiError, match='guides must be'):
        integ.trace_guides(fr, out=torch.zeros((H, W, 4), dtype=torch.float32, device='cuda'))
    # the id form: the same check of the guides, and the id image's own
    ids = torch.zeros((H, W), dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.PtmiError, match='guides must be'):
        integ.trace_guides_ids(fr, out=(torch.zeros((H, W, 4), dtype=torch.float32, device='cuda'), ids))
    for bad in (ids.float(), ids.cpu(), torch.zeros((H, W + 1), dtype=torch.int32, device='cuda')[:, :W],
                torch.zeros((H, W, 1), dtype=torch.int32, device='cuda'), None):
        with pytest.raises(_lib.PtmiError, match='ids must be'):
            integ.trace_guides_ids(fr, out=(out, bad))
    assert eq(out.cpu().numpy(), ref) and not ids.any()  # rejected before the call


# ---------------------------------------------------------------- the guided filter
@pytest.fixture(scope='module')
def integ():
    """One Integrator for the module; the filter reads no scene."""
    from ptmi import device
    return device.Integrator(device.DeviceScene.from_arrays(gh.scene_inputs('vol2_final_scene', 64)[0]))


DEFAULTS = dict(sigma=4.0, sigma_z=0.1, sigma_a=0.2, normal_power_log2=5, demodulate=True)
_cases = {}


def case(w, h, iterations, **kw):
    """Synthetic inputs and their reference, computed once per case."""
    prm = dict(DEFAULTS, **kw)
    key = (w, h, iterations) + tuple(sorted(prm.items()))
    if key not in _cases:
        accum, stats, invalid = dh.synthetic(w, h, seed=w * 1000 + h)
        guides = gh.synthetic_guides(w, h, seed=w * 1000 + h)
        rgb, var = gh.denoise_guided(accum, stats, guides, iterations, **prm)
        for a in (accum, stats, guides, rgb, var):
            a.setflags(write=False)
        _cases[key] = (accum, stats, guides, invalid, rgb, var, prm)
    return _cases[key]


def check_finite(invalid, rgb, var):
    bad = np.zeros(var.shape, bool)
    for p in invalid:
        bad[p] = True
    if var.size > 2:
        assert np.isfinite(rgb[~bad]).all() and np.isfinite(var[~bad]).all()


# 70x37 and 13x11: ragged, several blocks, steps past the image; 64x64: whole
# tiles; 1x1, 5x1: every tap but the centre outside; 8 iterations: step 128
@pytest.mark.parametrize('w,h,iterations,kw', [
    (13, 11, 5, {}), (70, 37, 5, {}), (64, 64, 5, {}), (70, 37, 8, dict(normal_power_log2=7)),
    (70, 37, 5, dict(demodulate=False)), (13, 11, 3, dict(demodulate=False, normal_power_log2=0)),
    (70, 37, 5, dict(sigma_z=0.0, sigma_a=0.0)), (70, 37, 3, dict(sigma=0.0, sigma_z=0.0, sigma_a=0.0)),
    (1, 1, 3, {}), (5, 1, 5, dict(demodulate=False)), (5, 1, 8, dict(normal_power_log2=7)),
])
def test_denoise_guided_equals_reference(integ, w, h, iterations, kw):
    accum, stats, guides, invalid, ref_rgb, ref_var, prm = case(w, h, iterations, **kw)
    rgb, var = integ.denoise_guided(dev(accum), dev(stats), dev(guides), iterations, **prm)
    rgb, var = host(rgb), host(var)
    assert eq(rgb, ref_rgb)
    assert eq(var, ref_var)
    check_finite(invalid, rgb, var)


@pytest.mark.parametrize('lds_max_step', [0, 1])
@pytest.mark.parametrize('w,h,iterations,kw', [(70, 37, 5, {}), (13, 11, 3, dict(demodulate=False,
                                                                                  normal_power_log2=0))])
def test_both_tap_forms_compute_the_same_bits(integ, lds_max_step, w, h, iterations, kw):
    """Steps 1 and 2 through global loads (0) and step 1 alone with its colour
    in LDS (1). The default (steps 1 and 2 in LDS, the rest global loads) is
    the other tests'."""
    from ptmi import guide
    accum, stats, guides, _, ref_rgb, ref_var, prm = case(w, h, iterations, **kw)
    prev = guide.set_lds_max_step(lds_max_step)
    try:
        rgb, var = integ.denoise_guided(dev(accum), dev(stats), dev(guides), iterations, **prm)
        rgb, var = host(rgb), host(var)
    finally:
        guide.set_lds_max_step(prev)
    assert prev == 2
    assert eq(rgb, ref_rgb) and eq(var, ref_var)


def test_zero_iterations_returns_the_remodulated_load(integ):
    accum, stats, guides, _, ref_rgb, ref_var, prm = case(70, 37, 0)
    rgb, var = integ.denoise_guided(dev(accum), dev(stats), dev(guides), 0, **prm)
    assert eq(host(rgb), ref_rgb) and eq(host(var), ref_var)
    c0, v0 = dh.load(accum, stats)
    m, lm2 = gh.modulation(guides)
    with np.errstate(all='ignore'):
        assert eq(ref_rgb, (c0 / m) * m) and eq(ref_var, (v0 / lm2) * lm2)
    # without the flag it is the load itself, as ptmi_denoise's
    accum, stats, guides, _, ref_rgb, ref_var, prm = case(70, 37, 0, demodulate=False)
    rgb, var = integ.denoise_guided(dev(accum), dev(stats), dev(guides), 0, **prm)
    assert eq(host(rgb), c0) and eq(host(var), v0)


def test_neutral_guides_give_the_unguided_filter(integ):
    """One flat surface everywhere and no demodulation: every guide factor is
    exactly 1, and ptmi_denoise_guided computes what ptmi_denoise computes."""
    import torch
    accum, stats, _ = dh.synthetic(70, 37, seed=70037)
    g = np.zeros((37, 70, 8), f32)
    g[...] = (0, 0, 1, 2.5, 0.5, 0.5, 0.5, 1)
    a, s = dev(accum), dev(stats)
    rgb, var = integ.denoise_guided(a, s, dev(g), 5, 4.0, demodulate=False)
    rgb, var = host(rgb).copy(), host(var).copy()
    rgb0, var0 = integ.denoise(a, s, 5, 4.0, out=torch.empty_like(a))
    assert eq(rgb, host(rgb0)) and eq(var, host(var0))


def test_out_var_may_be_null_and_outputs_may_be_given(integ):
    import torch
    from ptmi import guide, post
    accum, stats, guides, _, ref_rgb, ref_var, prm = case(13, 11, 5)
    a, s, g = dev(accum), dev(stats), dev(guides)
    out = torch.full((11, 13, 3), -1.0, dtype=torch.float32, device='cuda')
    var = torch.full((11, 13), -1.0, dtype=torch.float32, device='cuda')
    r = integ.denoise_guided(a, s, g, 5, out=out, var=var, **prm)
    assert r[0] is out and r[1] is var
    assert eq(host(out), ref_rgb) and eq(host(var), ref_var)
    assert eq(host(g), guides)  # read in place, left as they were
    # the C call with out_var = NULL, on the workspace of ptmi_denoise
    lib = guide.load()
    need = post.workspace_bytes(13, 11)
    ws = torch.empty(need // 4, dtype=torch.float32, device='cuda')
    out2 = torch.full((11, 13, 3), -1.0, dtype=torch.float32, device='cuda')
    p = guide.params(5, **prm)
    rc = lib.ptmi_denoise_guided(a.data_ptr(), s.data_ptr(), g.data_ptr(), 13, 11, C.byref(p), ws.data_ptr(), need,
                                 out2.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ptmi_last_error()
    assert eq(host(out2), ref_rgb)


def test_denoise_guided_on_a_side_stream(integ):
    import torch
    accum, stats, guides, _, ref_rgb, ref_var, prm = case(64, 64, 5)
    a, s, g = dev(accum), dev(stats), dev(guides)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    rgb, var = integ.denoise_guided(a, s, g, 5, stream=side, **prm)
    side.synchronize()
    assert eq(rgb.cpu().numpy(), ref_rgb) and eq(var.cpu().numpy(), ref_var)


# ---------------------------------------------------------------- renderer
def _renderer(tmp_path, scene='vol2_final_scene', spp=32):
    from coverage_scene import coverage_scene
    from ptmi import scenes
    from ptmi.renderer import MI355XRenderer
    random.seed(1234)
    if scene == 'vol2_final_scene':
        sc = scenes.vol2_final_scene(width=64)
    elif scene == 'coverage':
        sc = coverage_scene(64)
    else:
        sc = scenes.SCENES[scene]()
    sc.cam.img_width = 64
    sc.cam.samples_per_pixel = spp
    r = MI355XRenderer(sc.world, sc.cam, str(tmp_path / 'a.png'))
    r.background_color = sc.background
    r.max_depth = sc.max_depth
    return r


def test_renderer_guides_and_guided_denoise_on_a_real_frame(tmp_path, capsys):
    """The 16-spp cornell_smoke render with its traced guides: the renderer
    surface, and the filter against the numpy reference on real data."""
    from ptmi import scene_data as sd
    r = _renderer(tmp_path, 'cornell_smoke')
    with pytest.raises(ValueError, match='no stats: render through render_adaptive'):
        r.denoise(guided=True)
    r.render_adaptive(target_error=0, pass_spp=16, min_spp=16, max_spp=16)
    a, s = host(r.accum).copy(), host(r.stats).copy()
    # r.denoise() without `guided` is what it was
    plain = host(r.denoise()).copy()
    ref_rgb, ref_var = dh.denoise(a, s, 5, 4.0)
    assert eq(plain, ref_rgb) and eq(host(r.denoised_var), ref_var)
    assert r.guide_trace_seconds is None  # and traces nothing
    with pytest.raises(ValueError, match='guided=True'):
        r.denoise(sigma_z=0.5)
    # the guides: traced once, cached, equal to the reference
    g = r.guides()
    assert tuple(g.shape) == (64, 64, 8) and r.guides() is g and r.guide_trace_seconds is not None
    ref_g = gh.trace_guides(r.arrays, sd.camera_upload(r.cam))
    assert eq(host(g), ref_g)
    maps = r.guide_maps()
    assert eq(maps['normal'], ref_g[..., 0:3]) and eq(maps['depth'], ref_g[..., 3])
    assert eq(maps['albedo'], ref_g[..., 4:7]) and eq(maps['hit'], ref_g[..., 7] != 0) and maps['hit'].dtype == bool
    # the guided filter
    out = r.denoise(guided=True)
    assert out is r.denoised and tuple(out.shape) == (64, 64, 3) and tuple(r.denoised_var.shape) == (64, 64)
    ref_rgb, ref_var = gh.denoise_guided(a, s, ref_g)
    assert eq(host(r.denoised), ref_rgb) and eq(host(r.denoised_var), ref_var)
    assert not eq(ref_rgb, plain)
    assert eq(host(r.accum), a) and eq(host(r.stats), s) and eq(host(r.guides()), ref_g)
    assert eq(r.image_u8(denoised=True), dh.tonemap(ref_rgb))
    r.denoise(iterations=3, sigma=8.0, guided=True, sigma_z=0.3, sigma_a=0.1, normal_power_log2=2, demodulate=False)
    assert eq(host(r.denoised), gh.denoise_guided(a, s, ref_g, 3, 8.0, 0.3, 0.1, 2, False)[0])
    assert r.guides() is g
    r.sample_times = r.sample_times or [1.0]
    r.print_statistics()
    txt = capsys.readouterr().out
    assert 'Denoise Time' in txt and 'Guide Trace Time' in txt


def test_renderer_retraces_guides_for_a_new_camera(tmp_path):
    r = _renderer(tmp_path, 'cornell_box')
    g = r.guides()
    first = host(g).copy()
    r.max_depth = 7  # not a camera change: the guides stay
    r._upload_camera()
    assert r.guides() is g
    r.cam.vfov = r.cam.vfov * 0.5
    r.cam.initialize()
    r._upload_camera()
    g2 = r.guides()
    assert g2 is not g and not eq(host(g2), first)


# ---------------------------------------------------------------- quality
# The CPU prototype of the contract (numpy on the CPU oracle, 64 px, 16 spp
# against 4096 spp) gave unguided -> guided at the defaults: cornell_box 0.0331
# -> 0.0275 (17 %), coverage 0.00765 -> 0.00510 (33 %). vol2 is not in the
# condition: its margin is 1 %.
@pytest.mark.parametrize('scene', ['cornell_box', 'coverage'])
def test_guided_16spp_is_closer_to_4096spp_than_unguided(tmp_path, scene):
    """A condition, not a measurement: mse(guided, defaults) < mse(unguided,
    defaults) against a 4096-spp frame on a 64-px-wide frame, both rendered
    here as tests/test_gpu_denoise.py renders them; linear rgb over the pixels
    finite in both frames."""
    r = _renderer(tmp_path, scene)
    r.render_adaptive(target_error=0, pass_spp=16, min_spp=16, max_spp=16)
    noisy = host(r.accum) / f32(16)
    plain = host(r.denoise()).copy()
    guided = host(r.denoise(guided=True)).copy()
    r.render_adaptive(target_error=0, pass_spp=256, min_spp=4096, max_spp=4096)
    assert (r.sample_count_map() == 4096).all()
    ref = host(r.accum) / f32(4096)
    ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1)
    assert ok.mean() > 0.99

    def mse(img):
        return float(np.mean((img[ok].astype(np.float64) - ref[ok]) ** 2))

    print(f'{scene}: mse noisy {mse(noisy):.6g} unguided {mse(plain):.6g} guided {mse(guided):.6g} '
          f'over {int(ok.sum())} pixels')
    assert mse(guided) < mse(plain)
