"""GPU: the temporal ABI (include/ptmi_temporal.h) bit for bit against its numpy
f32 reference (reproject_helpers): the CPU check program's cases on the device
(oracle guides of cornell_box and cornell_smoke at 48 and 33 px, four camera
moves, a synthetic history with n = 0, n = 1, NaN and infinite pixels, tiny
frames, a previous camera without delta_u), coverage and vol2 at 64 px with
guides from ptmi_guide_trace, a side stream and given outputs; the contract's
properties on every output; the quality condition (a reprojected 64-spp
history plus 4 new spp is closer to 1024 spp than the 4 spp alone); and the
viewer surface."""
import os
import random

import numpy as np
import pytest

import reproject_helpers as rh

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
    return torch.from_numpy(np.array(a, f32)).cuda()


_integs = {}


def integrator(name='cornell_box', width=48):
    """One Integrator per scene for the module; the reprojection itself reads no scene."""
    from ptmi import device
    if (name, width) not in _integs:
        _integs[name, width] = device.Integrator(device.DeviceScene.from_arrays(rh.scene(name, width)[0]))
    return _integs[name, width]


def run(case, prm=rh.DEFAULTS):
    cur, prev, gc, gp, accum, stats = case
    a, s = integrator().reproject(cur, prev, dev(gc), dev(gp), dev(accum), dev(stats), **prm)
    return host(a), host(s)


def check(case, prm=rh.DEFAULTS):
    """The case on the device: bit for bit the reference, and the contract's properties."""
    ref_a, ref_s, det = rh.reproject(*case, details=True, **prm)
    a, s = run(case, prm)
    assert eq(s, ref_s)
    assert eq(a, ref_a)
    rh.check_properties(a, s, det, prm['max_history'])
    return a, s, det


# ---------------------------------------------------------------- bit for bit
@pytest.mark.parametrize('name,width,delta', rh.ORACLE_CASES)
def test_reproject_equals_reference_on_oracle_guides(name, width, delta):
    case = rh.oracle_case(name, width, delta)
    a, s, det = check(case)
    frac = float((s[..., 0] > 0).mean())
    print(f'{name} {width} px delta {delta}: history on {100 * frac:.1f} % of the pixels')
    if delta == (600, 0):  # from the other side: the points are in the old frame, but a wall shows its back
        assert det['valid'].any() and frac == 0.0
    if delta == (0, 0):  # the camera not moved: a pixel whose own previous pixel is a countable tap has history
        cur, prev, gc, gp, accum, stats = case
        own = rh.countable(accum, stats) & np.isfinite(gc[..., 3]) & np.isfinite(gp[..., 3])
        assert own.mean() > 0.95 and (s[..., 0][own] > 0).all()


@pytest.mark.parametrize('width,height', rh.FLAT_CASES)
def test_reproject_equals_reference_on_tiny_frames(width, height):
    a, s, _ = check(rh.flat_case(width, height))
    assert (s[..., 0] > 0).any()


@pytest.mark.parametrize('prm', [dict(max_history=1.0, sigma_z=0.0, normal_min=1.0, sigma_a=0.0),
                                 dict(max_history=8.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2),
                                 dict(max_history=float(1 << 24), sigma_z=10.0, normal_min=-1.0, sigma_a=10.0)])
def test_reproject_equals_reference_at_other_parameters(prm):
    check(rh.oracle_case('cornell_smoke', 33, (4, 2)), prm)


def test_degenerate_previous_cameras_leave_no_history():
    cur, prev, gc, gp, accum, stats = rh.oracle_case('cornell_box', 33, (4, 2))
    a, s, det = check((cur, dict(prev, delta_u=np.zeros(3, f32)), gc, gp, accum, stats))
    assert not det['valid'].any() and not a.any() and not s.any()
    # lam <= 0: the previous camera stood past the wall
    cur, prev, gc, gp, accum, stats = rh.flat_case(3, 2)
    a, s, det = check((cur, rh.flat_camera(3, 2, (0.0, 0.0, -5.0)), gc, gp, accum, stats))
    hit = gc[..., 7] != 0
    assert (det['lam'][hit] < 0).all() and not s[hit].any()


# coverage: every texture and material type; vol2: shell, fog sphere, glass, metal
@pytest.mark.parametrize('name', ['coverage', 'vol2_final_scene'])
@pytest.mark.parametrize('delta', [(4, 2), (40, 20)])
def test_reproject_equals_reference_on_traced_guides(name, delta):
    """Guides of both cameras from ptmi_guide_trace itself (pinned to its own
    reference by tests/test_gpu_guides.py), at 64 px."""
    from ptmi import device
    sa, cam_obj, bg = rh.scene(name, 64)
    integ = integrator(name, 64)
    prev, cur = rh.orbit(cam_obj, 0, 0), rh.orbit(cam_obj, *delta)
    W, H = prev['width'], prev['height']
    gp = integ.trace_guides(device.make_frame(prev, bg, 50, 0, W, H))
    gc = integ.trace_guides(device.make_frame(cur, bg, 50, 0, W, H))
    accum, stats = rh.history(W, H)
    a, s = integ.reproject(cur, prev, gc, gp, dev(accum), dev(stats))
    a, s, gc, gp = host(a), host(s), host(gc), host(gp)
    ref_a, ref_s, det = rh.reproject(cur, prev, gc, gp, accum, stats, details=True)
    assert eq(s, ref_s) and eq(a, ref_a)
    rh.check_properties(a, s, det, 32.0)
    frac = float((s[..., 0] > 0).mean())
    print(f'{name} 64 px delta {delta}: history on {100 * frac:.1f} % of the pixels')
    assert 0.0 < frac < 1.0  # part of the moved frame is new


def test_reproject_into_given_tensors_on_a_side_stream():
    import torch
    from ptmi import _lib
    case = rh.oracle_case('cornell_smoke', 33, (4, 2))
    cur, prev, gc, gp, accum, stats = case
    ref_a, ref_s = rh.reproject(*case)
    integ = integrator()
    g0, g1, a0, s0 = dev(gc), dev(gp), dev(accum), dev(stats)
    out = (torch.full((33, 33, 3), -1.0, dtype=torch.float32, device='cuda'),
           torch.full((33, 33, 4), -1.0, dtype=torch.float32, device='cuda'))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r = integ.reproject(cur, prev, g0, g1, a0, s0, out=out, stream=side)
    side.synchronize()
    assert r[0] is out[0] and r[1] is out[1]
    assert eq(out[0].cpu().numpy(), ref_a) and eq(out[1].cpu().numpy(), ref_s)
    assert eq(host(a0), accum) and eq(host(s0), stats) and eq(host(g0), gc) and eq(host(g1), gp)  # inputs untouched
    # ptmi_camera values instead of dicts
    from ptmi import temporal
    a, s = integ.reproject(temporal.camera(cur), temporal.camera(prev), g0, g1, a0, s0)
    assert eq(host(a), ref_a) and eq(host(s), ref_s)
    with pytest.raises(_lib.PtmiError, match='aliases'):
        integ.reproject(cur, prev, g0, g1, a0, s0, out=(a0, out[1]))
    with pytest.raises(_lib.PtmiError, match='max_history'):
        integ.reproject(cur, prev, g0, g1, a0, s0, max_history=0.0)
    with pytest.raises(_lib.PtmiError, match='guides must be'):
        integ.reproject(cur, prev, g0, s0, a0, s0)


# ---------------------------------------------------------------- quality
# Measured on an MI355X (profiles/temporal/quality.json; 48 px, a 64-spp history,
# orbit (4, 2), 4 new spp, against 1024 spp), 4 spp alone -> with history at the
# defaults: cornell_box 0.1935 -> 0.0695 (2.8x), cornell_smoke 0.2254 -> 0.0314
# (7.2x). vol2 is not in the condition: its margin is 8 %.
def _quality(name, caps=(32.0,), delta=(4, 2)):
    import torch
    from ptmi import device
    sa, cam_obj, bg = rh.scene(name, 48)
    integ = integrator(name, 48)
    prev, cur = rh.orbit(cam_obj, 0, 0), rh.orbit(cam_obj, *delta)
    W, H = prev['width'], prev['height']
    f0, f1 = device.make_frame(prev, bg, 50, 0, W, H), device.make_frame(cur, bg, 50, 0, W, H)
    zeros = lambda c: torch.zeros((H, W, c), dtype=torch.float32, device='cuda')  # noqa: E731
    a0, s0 = zeros(3), zeros(4)
    integ.render_mk_stats(f0, a0, s0, 0, 64)  # the history
    g0, g1 = integ.trace_guides(f0), integ.trace_guides(f1)
    ref = zeros(3)
    integ.render_mk(f1, ref, 10000, 1024)
    ref = host(ref) / f32(1024)
    alone_a, alone_s = zeros(3), zeros(4)
    integ.render_mk_stats(f1, alone_a, alone_s, 64, 4)
    alone = host(alone_a) / f32(4)
    assert (host(alone_s)[..., 0] == 4).all()
    out = {}
    for cap in caps:
        a, s = integ.reproject(cur, prev, g1, g0, a0, s0, max_history=cap)
        frac = float((host(s)[..., 0] > 0).mean())
        integ.render_mk_stats(f1, a, s, 64, 4)
        n = host(s)[..., 0]
        assert (n >= 4).all() and (n <= cap + 4).all() and eq(n, np.floor(n))
        out[cap] = (host(a) / n[..., None], frac)
    ok = np.isfinite(ref).all(-1) & np.isfinite(alone).all(-1)
    for img, _ in out.values():
        ok &= np.isfinite(img).all(-1)
    assert ok.mean() > 0.99

    def mse(img):
        return float(np.mean((img[ok].astype(np.float64) - ref[ok]) ** 2))

    return mse(alone), {cap: (mse(img), frac) for cap, (img, frac) in out.items()}


@pytest.mark.parametrize('name', ['cornell_box', 'cornell_smoke'])
def test_history_plus_4spp_is_closer_to_1024spp_than_4spp_alone(name):
    """A condition, not a measurement: mse(reprojected 64-spp history + samples
    64..67) < mse(samples 64..67 alone) against 1024 spp from sample 10000 at
    the moved camera, 48 px, defaults; linear rgb over the finite pixels. The
    caps 8 and 64 are printed, not asserted."""
    alone, with_history = _quality(name, (32.0, 8.0, 64.0))
    for cap, (m, frac) in with_history.items():
        print(f'{name}: mse 4 spp alone {alone:.6g}, + history cap {cap:g} {m:.6g} ({alone / m:.2f}x), '
              f'history on {100 * frac:.1f} % of the pixels')
    assert with_history[32.0][0] < alone


# ---------------------------------------------------------------- renderer and viewer
class _Event:
    def __init__(self, x, y):
        self.x, self.y = x, y


def _viewer(tmp_path, name, spp, **kw):
    from ptmi import scenes
    from ptmi.interactive_viewer import InteractiveViewer
    random.seed(1234)
    sc = scenes.SCENES[name]()
    sc.cam.img_width = 48
    sc.cam.samples_per_pixel = spp
    v = InteractiveViewer(sc.world, sc.cam, str(tmp_path / f'{name}{len(kw)}.png'), **kw)
    v.background_color = sc.background
    v.max_depth = sc.max_depth
    return v


def test_renderer_reproject_history(tmp_path):
    from ptmi import scene_data as sd
    v = _viewer(tmp_path, 'cornell_box', 16)
    with pytest.raises(ValueError, match='no stats'):
        v.reproject_history(sd.camera_upload(v.cam), None)
    v.render_adaptive(target_error=0, pass_spp=16, min_spp=16, max_spp=16)
    v.denoise()
    prev_cam, prev_guides = sd.camera_upload(v.cam), v.guides()
    a0, s0, g0 = host(v.accum).copy(), host(v.stats).copy(), host(prev_guides).copy()
    with pytest.raises(ValueError, match='again=True needs'):
        v.reproject_history(prev_cam, prev_guides, again=True)
    # the camera not moved: prev_guides is the cached tensor of the current camera, every countable pixel keeps history
    frac = v.reproject_history(prev_cam, prev_guides, max_history=64)
    ref_a, ref_s = rh.reproject(prev_cam, prev_cam, g0, g0, a0, s0, max_history=64.0)
    assert eq(host(v.accum), ref_a) and eq(host(v.stats), ref_s)
    own = rh.countable(a0, s0)
    assert frac == float((ref_s[..., 0] > 0).mean()) and own.mean() > 0.99 and (ref_s[..., 0][own] >= 15).all()
    assert v.guides() is prev_guides and v.denoised is None
    a0, s0 = ref_a, ref_s
    # a move
    v.rotate_camera(4, 2)
    frac = v.reproject_history(prev_cam, prev_guides, max_history=8)
    cur_cam = sd.camera_upload(v.cam)
    ref_a, ref_s = rh.reproject(cur_cam, prev_cam, host(v.guides()), g0, a0, s0, max_history=8.0)
    assert eq(host(v.accum), ref_a) and eq(host(v.stats), ref_s)
    assert frac == float((ref_s[..., 0] > 0).mean()) and 0.8 < frac < 1.0
    assert v._tiles['n'] == v._tiles['grid'][0] * v._tiles['grid'][1]
    assert (v.sample_count_map() <= 8).all()
    # the camera moves on with no sample in between: the same history again, not the reprojected one
    v.rotate_camera(3, 1)
    frac = v.reproject_history(prev_cam, prev_guides, again=True, max_history=8)
    ref_a, ref_s = rh.reproject(sd.camera_upload(v.cam), prev_cam, host(v.guides()), g0, a0, s0, max_history=8.0)
    assert eq(host(v.accum), ref_a) and eq(host(v.stats), ref_s) and frac == float((ref_s[..., 0] > 0).mean())


def test_temporal_viewer_keeps_its_history_across_a_drag(tmp_path, capsys):
    from ptmi import device, scene_data as sd
    spp = 6
    v = _viewer(tmp_path, 'cornell_box', spp, temporal=True, max_history=4)
    v.render_interactive()
    assert v.next_sample_index == spp and (v.sample_count_map() == spp).all()
    cam0 = sd.camera_upload(v.cam)
    # what the first run must have accumulated: samples 0 .. spp-1, one per launch
    integ = v.integrator
    f0 = device.make_frame(cam0, v.background_color, v.max_depth, v.seed, 48, 48)
    a, s = integ.new_stats(f0)[..., :3].contiguous(), integ.new_stats(f0)
    for i in range(spp):
        integ.render_mk_stats(f0, a, s, i, 1)
    assert eq(host(v.accum), host(a)) and eq(host(v.stats), host(s))
    g0 = v.guides()

    v.camera_update_interval = 0.0  # no throttle: every drag event moves the camera
    v.on_mouse_down(_Event(10, 10))
    v.on_mouse_drag(_Event(13, 11))
    v.on_mouse_drag(_Event(14, 12))  # a second step of the same drag: the rendered history once more, no chain
    out = capsys.readouterr().out
    assert out.count('history reprojected to') == 2
    counts = v.sample_count_map()
    frac = float((counts > 0).mean())
    print(f'viewer: history on {100 * frac:.1f} % of the pixels after the drag')
    assert frac == v.history_fraction and 0.8 < frac < 1.0
    assert counts.max() <= 4
    assert v.current_sample == 0 and v.next_sample_index == spp  # the progress count restarts, the index does not
    cam1 = sd.camera_upload(v.cam)
    assert not np.array_equal(cam0['center'], cam1['center'])
    f1 = device.make_frame(cam1, v.background_color, v.max_depth, v.seed, 48, 48)
    a1, s1 = integ.reproject(cam1, cam0, v.guides(), g0, a, s, max_history=4)
    assert eq(host(v.accum), host(a1)) and eq(host(v.stats), host(s1))

    v.render_interactive()  # keeps the history: its warm-up sample clears nothing
    for i in range(spp, 2 * spp):  # the second run's sample indices continue past the first run's
        integ.render_mk_stats(f1, a1, s1, i, 1)
    assert eq(host(v.accum), host(a1)) and eq(host(v.stats), host(s1))
    assert v.next_sample_index == 2 * spp
    counts = v.sample_count_map()
    assert counts.min() == spp and counts.max() <= 4 + spp
    assert os.path.exists(v.img_path)
    # the image divides each pixel by its own count
    assert eq(v.image_u8(), integ.tonemap(v.accum, stats=v.stats).cpu().numpy())


def test_temporal_viewer_drag_at_the_phi_clamp(tmp_path):
    """A vertical drag at the +-89 degree clamp uploads the camera it had: the
    reprojection then runs with one guide tensor for both frames, and, with no
    sample in between, once more from the same rendered history."""
    from ptmi import scene_data as sd
    spp = 3
    v = _viewer(tmp_path, 'cornell_box', spp, temporal=True, max_history=16)
    v.camera_update_interval = 0.0
    v.render_interactive()
    v.on_mouse_down(_Event(0, 0))
    v.on_mouse_drag(_Event(0, 400))  # 120 degrees up: clamped at 89
    assert v.history_fraction < 1.0  # seen from above: little or nothing of the old view
    v.render_interactive()
    cam = sd.camera_upload(v.cam)
    a0, s0, g = host(v.accum).copy(), host(v.stats).copy(), v.guides()
    assert (s0[..., 0] >= spp).all()
    v.on_mouse_drag(_Event(0, 800))  # further up: the same camera, bit for bit
    assert all(np.array_equal(cam[k], sd.camera_upload(v.cam)[k]) for k in cam) and v.guides() is g
    ref_a, ref_s = rh.reproject(cam, cam, host(g), host(g), a0, s0, max_history=16.0)
    assert eq(host(v.accum), ref_a) and eq(host(v.stats), ref_s)
    assert v.history_fraction == float((ref_s[..., 0] > 0).mean()) and v.history_fraction > 0.99
    assert v.current_sample == 0 and v.next_sample_index == 2 * spp
    v.on_mouse_drag(_Event(0, 1200))  # and again, with no sample in between
    assert eq(host(v.accum), ref_a) and eq(host(v.stats), ref_s) and v.next_sample_index == 2 * spp
    v.render_interactive()
    assert v.next_sample_index == 3 * spp and (v.sample_count_map() >= spp).all()


def test_a_viewer_without_temporal_is_what_it_was(tmp_path):
    """temporal=False (the default) given the same events: the drag clears, the
    second run renders samples 0 .. spp-1 of the new camera through render_mk,
    and no stats exist."""
    import torch
    from ptmi import device, scene_data as sd
    spp = 6
    v = _viewer(tmp_path, 'cornell_box', spp)
    assert v.temporal is False
    v.render_interactive()
    v.on_mouse_down(_Event(10, 10))
    v.on_mouse_drag(_Event(14, 12))
    assert not host(v.accum).any() and v.stats is None and v.next_sample_index == 0
    v.render_interactive()
    f1 = device.make_frame(sd.camera_upload(v.cam), v.background_color, v.max_depth, v.seed, 48, 48)
    a = torch.zeros((48, 48, 3), dtype=torch.float32, device='cuda')
    for i in range(spp):
        v.integrator.render_mk(f1, a, i, 1)
    assert eq(host(v.accum), host(a)) and v.stats is None and v.history_fraction is None
