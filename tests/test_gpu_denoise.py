"""GPU: the variance-guided a-trous denoiser (include/ptmi_post.h) bit for bit
against its numpy f32 reference (denoise_helpers): ragged and tiny images, steps
that cross tiles and borders, every special pixel of the contract, both tap
forms (LDS tile and global loads), the optional arguments, a side stream, the
renderer surface, and the quality condition: on a 16-spp frame the filter
lowers the error against a 4096-spp frame."""
import ctypes as C
import random

import numpy as np
import pytest

import denoise_helpers as dh

pytestmark = pytest.mark.gpu

f32 = np.float32


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope='module')
def integ():
    """One Integrator for the module; the denoiser reads no scene."""
    from parity_helpers import scene_inputs
    from ptmi import device
    return device.Integrator(device.DeviceScene.from_arrays(scene_inputs('vol2_final_scene', 64)[0]))


_cases = {}


def case(w, h, iterations, sigma=4.0):
    """Synthetic inputs and their reference, computed once per case."""
    key = (w, h, iterations, sigma)
    if key not in _cases:
        accum, stats, invalid = dh.synthetic(w, h, seed=w * 1000 + h)
        rgb, var = dh.denoise(accum, stats, iterations, sigma)
        for a in (accum, stats, rgb, var):
            a.setflags(write=False)
        _cases[key] = (accum, stats, invalid, rgb, var)
    return _cases[key]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def check_invalid(accum, stats, invalid, rgb, var):
    """The invalid pixels pass through bit-identically and poison no neighbour."""
    c0, v0 = dh.load(accum, stats)
    bad = np.zeros(var.shape, bool)
    for p in invalid:
        bad[p] = True
        assert eq(rgb[p], c0[p]) and eq(var[p], v0[p])
        assert not (np.isfinite(dh.lum(c0[p])) and np.isfinite(v0[p]))
    assert np.isfinite(rgb[~bad]).all() and np.isfinite(var[~bad]).all()


@pytest.mark.parametrize('w,h,iterations', [(13, 11, 5), (70, 37, 5), (64, 64, 5), (300, 200, 8)])
def test_denoise_equals_reference(integ, w, h, iterations):
    accum, stats, invalid, ref_rgb, ref_var = case(w, h, iterations)
    rgb, var = integ.denoise(dev(accum), dev(stats), iterations, 4.0)
    rgb, var = host(rgb), host(var)
    assert eq(rgb, ref_rgb)
    assert eq(var, ref_var)
    check_invalid(accum, stats, invalid, rgb, var)


@pytest.mark.parametrize('lds_max_step,w,h,iterations', [(0, 70, 37, 5), (1, 70, 37, 5), (0, 13, 11, 5)])
def test_both_tap_forms_compute_the_same_bits(integ, lds_max_step, w, h, iterations):
    """Steps 1 and 2 through global loads (0) and step 1 alone in LDS (1). The
    default (steps 1 and 2 in LDS, the rest global loads) is the other tests'."""
    from ptmi import post
    accum, stats, _, ref_rgb, ref_var = case(w, h, iterations)
    prev = post.set_lds_max_step(lds_max_step)
    try:
        rgb, var = integ.denoise(dev(accum), dev(stats), iterations, 4.0)
        rgb, var = host(rgb), host(var)
    finally:
        post.set_lds_max_step(prev)
    assert prev == 2
    assert eq(rgb, ref_rgb) and eq(var, ref_var)


def test_zero_iterations_returns_the_loaded_image(integ):
    accum, stats, _, ref_rgb, ref_var = case(70, 37, 0)
    rgb, var = integ.denoise(dev(accum), dev(stats), 0, 4.0)
    c0, v0 = dh.load(accum, stats)
    assert eq(host(rgb), c0) and eq(host(var), v0)
    assert eq(c0, ref_rgb) and eq(v0, ref_var)


def test_sigma_zero(integ):
    """den = 1e-4f everywhere: only taps of (nearly) the same luminance count."""
    accum, stats, invalid, ref_rgb, ref_var = case(70, 37, 3, 0.0)
    rgb, var = integ.denoise(dev(accum), dev(stats), 3, 0.0)
    rgb, var = host(rgb), host(var)
    assert eq(rgb, ref_rgb) and eq(var, ref_var)
    check_invalid(accum, stats, invalid, rgb, var)


def test_out_var_may_be_null_and_outputs_may_be_given(integ):
    import torch
    from ptmi import post
    accum, stats, _, ref_rgb, ref_var = case(13, 11, 5)
    a, s = dev(accum), dev(stats)
    out = torch.full((11, 13, 3), -1.0, dtype=torch.float32, device='cuda')
    var = torch.full((11, 13), -1.0, dtype=torch.float32, device='cuda')
    r = integ.denoise(a, s, 5, 4.0, out=out, var=var)
    assert r[0] is out and r[1] is var
    assert eq(host(out), ref_rgb) and eq(host(var), ref_var)
    # outputs of another shape, dtype, layout or device are rejected before the call
    from ptmi import _lib
    for bad in (torch.zeros((11, 13, 4), device='cuda'), out.double(), out.cpu(),
                torch.zeros((11, 13, 6), device='cuda')[..., ::2], host(out)):
        with pytest.raises(_lib.PtmiError, match='out must be'):
            integ.denoise(a, s, 5, 4.0, out=bad, var=var)
    for bad in (torch.zeros((13, 11), device='cuda'), var.int(), var.cpu(),
                torch.zeros((11, 26), device='cuda')[:, ::2]):
        with pytest.raises(_lib.PtmiError, match='var must be'):
            integ.denoise(a, s, 5, 4.0, out=out, var=bad)
    assert eq(host(out), ref_rgb) and eq(host(var), ref_var)
    # the C call with out_var = NULL
    lib = post.load()
    need = post.workspace_bytes(13, 11)
    ws = torch.empty(need // 4, dtype=torch.float32, device='cuda')
    out2 = torch.full((11, 13, 3), -1.0, dtype=torch.float32, device='cuda')
    rc = lib.ptmi_denoise(a.data_ptr(), s.data_ptr(), 13, 11, 5, 4.0, ws.data_ptr(), need, out2.data_ptr(), None,
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ptmi_last_error()
    assert eq(host(out2), ref_rgb)


def test_denoise_on_a_side_stream(integ):
    import torch
    accum, stats, _, ref_rgb, ref_var = case(64, 64, 5)
    a, s = dev(accum), dev(stats)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    rgb, var = integ.denoise(a, s, 5, 4.0, stream=side)
    side.synchronize()
    assert eq(rgb.cpu().numpy(), ref_rgb) and eq(var.cpu().numpy(), ref_var)


# ---------------------------------------------------------------- renderer
def _renderer(tmp_path, scene='vol2_final_scene', spp=32):
    from ptmi import scenes
    from ptmi.renderer import MI355XRenderer
    random.seed(1234)
    sc = scenes.vol2_final_scene(width=64) if scene == 'vol2_final_scene' else scenes.SCENES[scene]()
    sc.cam.img_width = 64
    sc.cam.samples_per_pixel = spp
    r = MI355XRenderer(sc.world, sc.cam, str(tmp_path / 'a.png'))
    r.background_color = sc.background
    r.max_depth = sc.max_depth
    return r


def test_renderer_denoise(tmp_path, capsys):
    from PIL import Image
    r = _renderer(tmp_path)
    with pytest.raises(ValueError, match='no stats: render through render_adaptive'):
        r.denoise()
    with pytest.raises(ValueError, match='denoise'):
        r.image_u8(denoised=True)
    r.render_adaptive(target_error=0.05, pass_spp=8, min_spp=8, max_spp=32)
    before = r.image_u8().copy()
    a, s = host(r.accum).copy(), host(r.stats).copy()
    out = r.denoise()
    assert out is r.denoised and tuple(out.shape) == (64, 64, 3) and tuple(r.denoised_var.shape) == (64, 64)
    ref_rgb, ref_var = dh.denoise(a, s, 5, 4.0)
    assert eq(host(r.denoised), ref_rgb) and eq(host(r.denoised_var), ref_var)
    assert eq(host(r.accum), a) and eq(host(r.stats), s)
    assert eq(r.image_u8(denoised=True), dh.tonemap(ref_rgb))
    assert eq(r.image_u8(), before)
    path = r.write_denoised_image()
    assert path.endswith('a_denoised.png') and eq(np.array(Image.open(path)), dh.tonemap(ref_rgb))
    r.denoise(iterations=2, sigma=1.0)
    assert eq(host(r.denoised), dh.denoise(a, s, 2, 1.0)[0])
    r.sample_times = r.sample_times or [1.0]
    r.print_statistics()
    assert 'Denoise Time' in capsys.readouterr().out


# ---------------------------------------------------------------- quality
# cornell_smoke is the scene the condition was first stated for; its 4096-spp
# frame has NaN pixels (2 of 4096 on the CPU oracle: samples lost in the
# medium), which leave an MSE over all pixels undefined. So the condition is
# asserted over all pixels on cornell_box, whose frames are finite, and on
# cornell_smoke over the pixels where both frames are finite. CPU oracle
# renders through the numpy reference (profiles/denoise/quality.json):
# cornell_box 0.0641 -> 0.0331, cornell_smoke 0.0620 -> 0.0264.
@pytest.mark.parametrize('scene,finite_only', [('cornell_box', False), ('cornell_smoke', True)])
def test_denoised_16spp_is_closer_to_4096spp_than_the_noisy_frame(tmp_path, scene, finite_only):
    """A cap, not a measurement: mse(denoised 16 spp, 4096 spp) < mse(noisy 16
    spp, 4096 spp) on a 64 x 64 frame, both frames rendered here (uniform
    stats renders: target_error = 0, min_spp = max_spp = N)."""
    r = _renderer(tmp_path, scene)
    r.render_adaptive(target_error=0, pass_spp=16, min_spp=16, max_spp=16)
    noisy = host(r.accum) / f32(16)
    den = host(r.denoise()).copy()
    r.render_adaptive(target_error=0, pass_spp=256, min_spp=4096, max_spp=4096)
    assert (r.sample_count_map() == 4096).all()
    ref = host(r.accum) / f32(4096)
    ok = np.ones(ref.shape[:2], bool)
    if finite_only:
        ok = np.isfinite(ref).all(-1) & np.isfinite(noisy).all(-1)
        assert ok.mean() > 0.99
    mse_noisy = float(np.mean((noisy[ok].astype(np.float64) - ref[ok]) ** 2))
    mse_den = float(np.mean((den[ok].astype(np.float64) - ref[ok]) ** 2))
    print(f'{scene}: mse noisy {mse_noisy:.6g} denoised {mse_den:.6g} over {int(ok.sum())} pixels')
    assert mse_den < mse_noisy
