"""GPU: per-pixel error estimates and adaptive tile sampling (ABI v8), bit for
bit against numpy f32 over the CPU oracle's per-sample colours
(adaptive_helpers): the stats resolve of both integrators, tile geometry on a
banded window, the tile update, the tile-listed megakernel trace, the adaptive
loop end to end, the per-pixel tone map and the renderer / viewer surface."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import adaptive_helpers as ah
from parity_helpers import scene_inputs

pytestmark = pytest.mark.gpu

SCENE = 'vol2_final_scene'
f32 = np.float32


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope='module')
def integs():
    """One Integrator for the module: the scene arrays do not depend on the camera width."""
    from ptmi import device
    sa = scene_inputs(SCENE, 64)[0]
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    return integ


def make(width, window=None, band=(1, 1, 0)):
    from ptmi import device
    _, cam, bg = scene_inputs(SCENE, width)
    return device.make_frame(cam, bg, 50, 0, cam['width'], cam['height'], window, band)


def zeros(fr, c):
    import torch
    return torch.zeros((fr.height, fr.width, c), dtype=torch.float32, device='cuda')


def pattern(fr, c, lo):
    """A non-zero pattern no render produces (for 'this pixel was not touched')."""
    import torch
    n = fr.height * fr.width * c
    v = (torch.arange(n, dtype=torch.float32, device='cuda') % 7.0) * 0.125 + lo
    return v.reshape(fr.height, fr.width, c).contiguous()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------- 1, 2: stats resolve
@pytest.mark.parametrize('calls', [[(0, 3), (3, 5)], [(s, 1) for s in range(8)]], ids=['3+5', 'single'])
def test_stats_resolve_megakernel(integs, calls):
    integ = integs
    fr = make(64)
    acc, stats, plain = zeros(fr, 3), zeros(fr, 4), zeros(fr, 3)
    for b, c in calls:
        integ.render_mk_stats(fr, acc, stats, b, c)
        integ.render_mk(fr, plain, b, c)
    cols, _ = ah.oracle_samples(SCENE, 64, 'mk', 0, 32)
    acc_ref, st_ref = np.zeros((64, 64, 3), f32), np.zeros((64, 64, 4), f32)
    ah.accumulate(acc_ref, st_ref, cols[:8])
    g, s = host(acc), host(stats)
    assert eq(g, host(plain))
    assert eq(g, acc_ref)
    assert eq(s, st_ref)
    assert (s[..., 0] == 8).all() and (s[..., 3] == 0).all() and (s[..., 2] >= 0).all()


def test_stats_resolve_wavefront(integs):
    integ = integs
    fr = make(64)
    acc, stats, plain = zeros(fr, 3), zeros(fr, 4), zeros(fr, 3)
    for b, c in [(0, 2), (2, 4)]:
        integ.render_wf_stats(fr, acc, stats, b, c)
        integ.render_wf(fr, plain, b, c)
    cols, _ = ah.oracle_samples(SCENE, 64, 'wf', 0, 6)
    acc_ref, st_ref = np.zeros((64, 64, 3), f32), np.zeros((64, 64, 4), f32)
    ah.accumulate(acc_ref, st_ref, cols)
    g, s = host(acc), host(stats)
    assert eq(g, host(plain))
    assert eq(g, acc_ref)
    assert eq(s, st_ref)


# ---------------------------------------------------------------- 3: tile geometry
def test_banded_window_tiles(integs):
    """16 x 4 tiles on a 2-rank band frame whose window width (80) is no
    multiple of 16: stats resolve on the owned rows only, then a listed trace
    of every second tile, then the tile update of that frame."""
    import torch
    from ptmi import device
    integ = integs
    win = (96, 200, 80, 40)
    fr = make(800, win, (4, 2, 1))
    assert integ.tile_grid(fr) == (16, 4, 5, 5)
    owned = device.frame_pixel_rows(fr)
    assert len(owned) == 20
    own = np.zeros((800, 800), bool)
    own[owned, 96:176] = True
    cols, _ = ah.oracle_samples(SCENE, 800, 'mk', 0, 8, mask=own)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    integ.clear(fr, acc)
    integ.clear_stats(fr, stats)
    acc_ref[own] = 0
    st_ref[own] = 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)  # the clears touch the owned pixels only
    integ.render_mk_stats(fr, acc, stats, 0, 4)
    ah.accumulate(acc_ref, st_ref, cols[:4], own)
    assert eq(host(acc), acc_ref)
    assert eq(host(stats), st_ref)
    # every second tile, samples 4..7
    ids = np.arange(0, 25, 2, dtype=np.int32)
    local = ah.tile_mask(80, 20, 16, 4, ids)
    listed = np.zeros((800, 800), bool)
    lr, lc = np.nonzero(local)
    listed[owned[lr], 96 + lc] = True
    tl = torch.from_numpy(ids).cuda()
    integ.render_mk_stats(fr, acc, stats, 4, 4, tiles=(tl, len(ids)))
    ah.accumulate(acc_ref, st_ref, cols[4:8], listed)
    assert eq(host(acc), acc_ref)
    assert eq(host(stats), st_ref)
    assert set(np.unique(st_ref[own][:, 0])) == {4.0, 8.0}
    # tile update on the band frame's local rows
    tiles = integ.new_tiles(fr)
    n = integ.tile_update(fr, stats, 0.5, 6, 64, tiles)
    new, E, act = ah.tile_update(np.ones(25, np.int32), st_ref[owned][:, 96:176], 16, 4, 0.5, 6, 64)
    assert eq(host(tiles['err']), E) and eq(host(tiles['state']), new)
    assert n == len(act) and eq(host(tiles['list'])[:n], act)


BANDS = [(4, 2, 1), (2, 2, 1), (1, 2, 0)]


@pytest.mark.parametrize('band', BANDS, ids=lambda b: '%dx%d' % (64 // b[0], b[0]))
def test_banded_window_tile_shapes(integs, band):
    """The megakernel stats render on a 2-rank band frame, every tile shape a banded frame can have
    (16 x 4, 32 x 2, 64 x 1): the 64 x 64 image, window x0 = 3, y0 = 2, 37 x 24
    (12 owned rows, a ragged right edge), 3 samples on the whole frame, then 3
    on a list of every second tile, an id outside the grid and the last (edge)
    tile, then the tile update; bit for bit against the oracle."""
    import torch
    from ptmi import device
    integ = integs
    x0, y0, w, h = 3, 2, 37, 24
    fr = make(64, (x0, y0, w, h), band)
    th, tw = band[0], 64 // band[0]
    tiles_x, tiles_y = -(-w // tw), 12 // th
    nt = tiles_x * tiles_y
    assert integ.tile_grid(fr) == (tw, th, tiles_x, tiles_y)
    owned = device.frame_pixel_rows(fr)
    assert len(owned) == 12
    own = np.zeros((fr.height, fr.width), bool)
    own[owned, x0:x0 + w] = True
    cols, _ = ah.oracle_samples(SCENE, 64, 'mk', 0, 6, mask=own)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    integ.clear(fr, acc)
    integ.clear_stats(fr, stats)
    acc_ref[own] = 0
    st_ref[own] = 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)  # the clears touch the owned pixels only
    integ.render_mk_stats(fr, acc, stats, 0, 3)
    ah.accumulate(acc_ref, st_ref, cols[:3], own)
    assert eq(host(acc), acc_ref)
    assert eq(host(stats), st_ref)
    ids = np.array(list(range(0, nt - 1, 2)) + [nt, nt - 1], np.int32)
    local = ah.tile_mask(w, 12, tw, th, ids[ids < nt])
    listed = np.zeros((fr.height, fr.width), bool)
    lr, lc = np.nonzero(local)
    listed[owned[lr], x0 + lc] = True
    tl = torch.from_numpy(ids).cuda()
    integ.render_mk_stats(fr, acc, stats, 3, 3, tiles=(tl, len(ids)))
    ah.accumulate(acc_ref, st_ref, cols[3:6], listed)
    assert eq(host(acc), acc_ref)
    assert eq(host(stats), st_ref)
    assert set(np.unique(st_ref[own][:, 0])) == {3.0, 6.0}
    tiles = integ.new_tiles(fr)
    n = integ.tile_update(fr, stats, 0.5, 6, 64, tiles)
    new, E, act = ah.tile_update(np.ones(nt, np.int32), st_ref[owned][:, x0:x0 + w], tw, th, 0.5, 6, 64)
    assert eq(host(tiles['err']), E) and eq(host(tiles['state']), new)
    assert n == len(act) and eq(host(tiles['list'])[:n], act)


# ---------------------------------------------------------------- 4: tile update
def test_tile_update_synthetic(integs):
    """53 x 37 frame of synthetic stats: n in {0, 1}, all-zero tiles, a NaN,
    n >= max_spp, partial edge tiles; then a second call after the stats got
    noisier: tiles that were done stay done."""
    import torch
    from ptmi import device
    integ = integs
    cam = {k: np.zeros(3, f32) for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = 0.0
    fr = device.make_frame(cam, (0, 0, 0), 50, 0, 53, 37)
    assert integ.tile_grid(fr) == (8, 8, 7, 5)
    rng = np.random.default_rng(5)
    lr, col, valid, _ = ah.tile_lanes(53, 37, 8, 8)
    n_tile = rng.choice([0, 1, 2, 5, 16, 31, 32, 40], size=35).astype(f32)
    n_tile[[0, 6, 34]] = [5, 16, 2]  # the corner tiles (6 and 34 are partial) get error values
    n_tile[[8, 19, 24]] = [0, 16, 16]  # the special tiles below
    st = np.zeros((37, 53, 4), f32)
    for t in range(35):
        st[lr[t][valid[t]], col[t][valid[t]], 0] = n_tile[t]
    st[..., 1] = rng.uniform(-1, 2, (37, 53)).astype(f32)
    st[..., 2] = (rng.uniform(0, 1, (37, 53)) ** 4 * st[..., 0] * 2).astype(f32)
    st[3, 12, 0], st[20, 20, 0] = 1, 0    # single pixels with n < 2 (not lane 0 of their tiles)
    st[8:16, 8:16] = 0                    # tile 8: all zero
    st[16:24, 40:48] = [16, 0, 0, 0]      # tile 19: sampled, black, no variance: E = 0
    st[30, 30, 1] = np.nan                # tile 24: a NaN mean
    st[24:32, 24:32, 0] = 16
    state0 = np.ones(35, np.int32)
    state0[[2, 11]] = 0                   # already done
    thr, lo, hi = 0.25, 4, 32
    stats = torch.from_numpy(st).cuda()
    tiles = integ.new_tiles(fr)
    tiles['state'].copy_(torch.from_numpy(state0))
    n = integ.tile_update(fr, stats, thr, lo, hi, tiles)
    new, E, act = ah.tile_update(state0, st, 8, 8, thr, lo, hi)
    assert np.isnan(E[24]) and new[24] == 0 and E[19] == 0 and np.isinf(E[8]) and new[8] == 1
    assert 4 < len(act) < 30 and (new[n_tile >= 32] == 0).all()
    assert eq(host(tiles['err']), E)
    assert eq(host(tiles['state']), new)
    assert n == len(act) and eq(host(tiles['list'])[:n], act)
    assert (np.diff(host(tiles['list'])[:n]) > 0).all()
    # noisier stats, fewer samples: done tiles stay done
    st2 = st.copy()
    st2[..., 2] *= f32(400)
    st2[..., 0] = np.minimum(st2[..., 0], f32(8))
    stats.copy_(torch.from_numpy(st2))
    n2 = integ.tile_update(fr, stats, thr, lo, hi, tiles)
    new2, E2, act2 = ah.tile_update(new, st2, 8, 8, thr, lo, hi)
    free = ah.tile_update(np.ones(35, np.int32), st2, 8, 8, thr, lo, hi)[0]
    assert (free > new2).any()  # some done tile would be active again without the monotone rule
    assert eq(host(tiles['err']), E2) and eq(host(tiles['state']), new2)
    assert n2 == len(act2) and eq(host(tiles['list'])[:n2], act2)


# ---------------------------------------------------------------- 5: listed trace
def test_listed_trace(integs):
    import torch
    integ = integs
    fr = make(64)
    ids = np.array(list(range(1, 64, 3)) + [63], np.int32)
    assert len(ids) == 22
    # ids outside the grid are ignored on the device
    dev_list = torch.from_numpy(np.concatenate([ids[:5], [-3, 64, 1 << 30], ids[5:]]).astype(np.int32)).cuda()
    listed = ah.tile_mask(64, 64, 8, 8, ids)
    cols, ost = ah.oracle_samples(SCENE, 64, 'mk', 0, 4, mask=listed)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    ws = integ.workspace(fr, 4, 'mk')
    ws.fill_(float('nan'))
    integ.reset_counters()
    # an empty list is a no-op
    integ.render_mk_stats(fr, acc, stats, 0, 4, tiles=(dev_list, 0))
    wp = C.c_void_p(ws.data_ptr())
    assert integ.lib.ptmi_mk_trace_tiles_ws(C.byref(integ.scene.view), C.byref(fr), wp, ws.numel() * 4,
                                            C.c_void_p(dev_list.data_ptr()), 0, 0, 4, integ._cnt(), None) == 0
    assert integ.lib.ptmi_mk_resolve_stats_ws(C.byref(fr), wp, ws.numel() * 4, C.c_void_p(acc.data_ptr()),
                                              C.c_void_p(stats.data_ptr()), C.c_void_p(dev_list.data_ptr()), 0, 4,
                                              None) == 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref) and integ.read_counters()['paths'] == 0
    # a list that is no contiguous 1-D int32 tensor on the device, and a count outside the list, are rejected
    from ptmi import _lib
    for bad in ((dev_list, dev_list.numel() + 1), (dev_list, -1), (dev_list.cpu(), 1), (dev_list.float(), 1),
                (dev_list[::2], 1), (dev_list.view(5, 5), 1), (dev_list.tolist(), 1)):
        with pytest.raises(_lib.PtmiError, match='^tiles'):
            integ.render_mk_stats(fr, acc, stats, 0, 4, tiles=bad)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref) and integ.read_counters()['paths'] == 0
    integ.render_mk_stats(fr, acc, stats, 0, 4, tiles=(dev_list, dev_list.numel()))
    ah.accumulate(acc_ref, st_ref, cols, listed)
    g, s = host(acc), host(stats)
    assert eq(g[listed], acc_ref[listed]) and eq(s[listed], st_ref[listed])
    assert eq(g[~listed], acc_ref[~listed]) and eq(s[~listed], st_ref[~listed])  # the pattern, untouched
    assert np.isfinite(g).all()
    cnt = integ.read_counters()
    assert cnt['paths'] == 64 * len(ids) * 4
    assert cnt == {k: int(v) for k, v in ost.items()}


def _rung(slots):
    """The staged megakernel's traversal kernel for max_leaf_depth + 1 stack slots."""
    return next((r for r in (16, 17, 18, 19, 20, 24, 32, 64) if slots <= r and slots <= 63), 'reference walk')


@pytest.mark.parametrize('name,traversal,rung', [
    ('chain17', 'stack', 17), ('chain18', 'stack', 18), ('chain19', 'stack', 19), ('chain20', 'stack', 20),
    ('chain22', 'stack', 24), ('chain29', 'stack', 32), ('chain52', 'stack', 64),
    ('chainx70', 'stack', 'reference walk'), ('chain22', 'stackless', 24)])
def test_listed_trace_on_every_traversal_rung(name, traversal, rung):
    """The listed trace of every rung of the traversal dispatch but the 16-slot
    one (test_listed_trace) against the unlisted trace, which test_gpu_edge
    ties to the oracle: bit-equal on the listed tiles, nothing else touched.
    32 x 18: 4 x 3 tiles of 8 x 8, the last row of tiles 2 pixels high."""
    import torch
    from edge_scenes import edge_scene
    from ptmi import device
    sa, cam, bg = edge_scene(name, 32)
    W, H, spp = cam['width'], cam['height'], 3
    assert (W, H) == (32, 18)
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    assert _rung(integ.scene.layout.max_leaf_depth + 1) == rung
    fr = device.make_frame(cam, bg, 50, 3, W, H, traversal=traversal)
    assert integ.tile_grid(fr) == (8, 8, 4, 3)
    ids = np.array([1, 4, 6, 9, 11], np.int32)
    dev_list = torch.from_numpy(np.array([1, -3, 4, 6, 12, 9, 1 << 30, 11], np.int32)).cuda()  # 3 ids outside the grid
    listed = ah.tile_mask(W, H, 8, 8, ids)
    assert listed.sum() == 64 * 3 + 16 * 2  # tiles 9 and 11 are 8 x 2
    whole = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    part = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    pat = [host(t).copy() for t in part]
    integ.render_mk_stats(fr, *whole, 0, spp)
    integ.reset_counters()
    integ.render_mk_stats(fr, *part, 0, spp, tiles=(dev_list, dev_list.numel()))
    for got, ref, untouched in zip(part, whole, pat):
        got, ref = host(got), host(ref)
        assert eq(got[listed], ref[listed])
        assert eq(got[~listed], untouched[~listed])
        assert not eq(ref[~listed], untouched[~listed])  # the unlisted trace did render there
    assert integ.read_counters()['paths'] == int(listed.sum()) * spp


# ---------------------------------------------------------------- 6: adaptive end to end
@pytest.mark.parametrize('always_listed', [False, True], ids=['plain-first-pass', 'listed-first-pass'])
def test_adaptive_end_to_end(integs, always_listed):
    """The adaptive loop (pass_spp 8, min_spp 8, max_spp 32, target 0.05) on
    the GPU and in numpy on the oracle's samples: per-pass active sets, tile
    errors, accum, stats, the per-pixel tone map and the path count."""
    integ = integs
    fr = make(64)
    thr, per, lo, hi = 0.05, 8, 8, 32
    cols, _ = ah.oracle_samples(SCENE, 64, 'mk', 0, 32)
    # reference loop
    acc_ref, st_ref = np.zeros((64, 64, 3), f32), np.zeros((64, 64, 4), f32)
    state, act = np.ones(64, np.int32), np.arange(64, dtype=np.int32)
    ref = []
    for k in range(hi // per):
        if len(act) == 0:
            break
        before = act
        ah.accumulate(acc_ref, st_ref, cols[k * per:(k + 1) * per], ah.tile_mask(64, 64, 8, 8, act))
        state, E, act = ah.tile_update(state, st_ref, 8, 8, thr, lo, hi)
        ref.append((before, state.copy(), E, act))
    # the case must not degenerate
    counts = [len(r[0]) for r in ref]
    assert counts[0] == 64 and 8 <= 64 - len(ref[0][3]) <= 56, counts
    for _, _, E, _ in ref:
        fin = E[np.isfinite(E)]
        assert (np.abs(fin - f32(thr)) > 1e-3 * thr).all()
    assert 64 * per * sum(counts) < 64 * 64 * hi
    # device loop
    acc, stats = zeros(fr, 3), zeros(fr, 4)
    tiles = integ.new_tiles(fr)
    integ.reset_counters()
    for k, (before, st_k, E, after) in enumerate(ref):
        assert tiles['n'] == len(before) and eq(host(tiles['list'])[:tiles['n']], before)
        sel = None if (tiles['n'] == 64 and not always_listed) else (tiles['list'], tiles['n'])
        integ.render_mk_stats(fr, acc, stats, k * per, per, tiles=sel)
        n = integ.tile_update(fr, stats, thr, lo, hi, tiles)
        assert n == len(after)
        assert eq(host(tiles['state']), st_k) and eq(host(tiles['err']), E)
    assert tiles['n'] == 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert integ.read_counters()['paths'] == int(st_ref[..., 0].sum()) == 64 * per * sum(counts)
    assert eq(host(integ.tonemap(acc, stats=stats)), ah.tonemap(acc_ref, st_ref[..., 0]))


# ---------------------------------------------------------------- 7: tone map
def test_tonemap_stats(integs):
    import torch
    integ = integs
    rng = np.random.default_rng(11)
    a = (rng.uniform(-0.2, 3.0, (37, 53, 3)) * rng.choice([1, 7, 1024], (37, 53, 1))).astype(f32)
    acc = torch.from_numpy(a).cuda()
    st = np.zeros((37, 53, 4), f32)
    stats = torch.from_numpy(st).cuda()
    for n in (1, 7, 1024):
        stats[..., 0] = float(n)
        assert eq(host(integ.tonemap(acc, stats=stats)), host(integ.tonemap(acc, n)))
    st[..., 0] = rng.choice([0, 1, 3, 8, 24, 1000], (37, 53)).astype(f32)
    stats.copy_(torch.from_numpy(st))
    img = host(integ.tonemap(acc, stats=stats))
    assert eq(img, ah.tonemap(a, st[..., 0]))
    assert (st[..., 0] == 0).any() and len(np.unique(img)) > 100


# ---------------------------------------------------------------- 8: renderer, viewer
def _scene(spp):
    from ptmi import scenes
    random.seed(1234)
    sc = scenes.vol2_final_scene(width=64)
    sc.cam.samples_per_pixel = spp
    return sc


def _renderer(tmp_path, spp=32):
    from ptmi.renderer import MI355XRenderer
    sc = _scene(spp)
    r = MI355XRenderer(sc.world, sc.cam, str(tmp_path / 'a.png'))
    r.background_color = sc.background
    r.max_depth = sc.max_depth
    return r


def test_render_adaptive_and_checkpoints(tmp_path, capsys):
    from PIL import Image
    r = _renderer(tmp_path)
    kw = dict(target_error=0.05, pass_spp=8, min_spp=8, max_spp=32)
    r.render_adaptive(**kw)
    a, s, e = host(r.accum).copy(), host(r.stats).copy(), r.noise_map().copy()
    passes = [dict(p) for p in r.adaptive_passes]
    n = r.sample_count_map()
    traced = sum(p['traced'] for p in passes)
    assert traced < 32 * 64 * 64 and traced == int(n.sum()) == r.integrator.read_counters()['paths']
    assert r.current_sample == int(n.max()) == 8 * len(passes) and n.min() >= 8 and (n % 8 == 0).all()
    assert len(np.unique(n)) > 1 and e.shape == (8, 8) and eq(n, s[..., 0])
    assert passes[0]['active_tiles'] == 64 and passes[-1]['active_after'] == 0
    assert eq(r.image_u8(), ah.tonemap(a, s[..., 0]))
    assert eq(np.array(Image.open(r.img_path)), r.image_u8())
    out = capsys.readouterr().out
    assert 'Adaptive passes' in out and 'share of a uniform 32-spp render' in out
    # the renderer is the integrator-level loop (checked against the oracle above)
    integ, fr = r.integrator, r.frame
    acc2, st2, tiles = zeros(fr, 3), zeros(fr, 4), integ.new_tiles(fr)
    for k in range(len(passes)):
        assert tiles['n'] == passes[k]['active_tiles']
        integ.render_mk_stats(fr, acc2, st2, 8 * k, 8, None if tiles['n'] == 64 else (tiles['list'], tiles['n']))
        integ.tile_update(fr, st2, 0.05, 8, 32, tiles)
    assert eq(host(acc2), a) and eq(host(st2), s) and eq(host(tiles['err']).reshape(8, 8), e)
    # checkpoint after pass 2, resume: bit-identical
    ck = str(tmp_path / 'adaptive.npz')
    r.checkpoint_path, r.checkpoint_every = ck, 2
    r.render_adaptive(**kw)
    r.checkpoint_path = None
    assert eq(host(r.accum), a)
    with np.load(ck) as z:
        assert int(z['next_sample']) == 16 and z['stats'].shape == (64, 64, 4) and z['tile_state'].sum() == passes[2]['active_tiles']
    r.clear_accumulation_buffer()
    r.load_checkpoint(ck)
    r.render_adaptive(resume=True, **kw)
    assert eq(host(r.accum), a) and eq(host(r.stats), s) and eq(r.noise_map(), e)
    assert [p['active_tiles'] for p in r.adaptive_passes] == [p['active_tiles'] for p in passes]
    # other adaptive parameters, or a plain render, refuse the adaptive checkpoint; and the reverse
    r.load_checkpoint(ck)
    with pytest.raises(ValueError, match='adaptive differs'):
        r.render_adaptive(resume=True, **dict(kw, target_error=0.1))
    r.load_checkpoint(ck)
    with pytest.raises(ValueError, match='integrator differs'):
        r.render(resume=True)
    plain = str(tmp_path / 'plain.npz')
    r.render_sample(0)
    r.save_checkpoint(plain)
    r.load_checkpoint(plain)
    with pytest.raises(ValueError, match='integrator differs'):
        r.render_adaptive(resume=True, **kw)
    # the wavefront renders whole frames; only the stop is adaptive
    r.render_adaptive(integrator='wavefront', **kw)
    nw = r.sample_count_map()
    assert (nw == nw[0, 0]).all() and r.current_sample == int(nw[0, 0]) <= 32


def test_viewer_stops_at_target_error(tmp_path):
    from ptmi.interactive_viewer import InteractiveViewer
    sc = _scene(64)
    v = InteractiveViewer(sc.world, sc.cam, str(tmp_path / 'v.png'))
    v.background_color = sc.background
    v.render_interactive(target_error=10.0, min_spp=4)
    assert 4 <= v.current_sample < 64 and not v.is_rendering_active and os.path.exists(tmp_path / 'v.png')
    n = v.sample_count_map()
    assert (n == v.current_sample).all() and (host(v._tiles['state']) == 0).all()
    assert eq(v.image_u8(), ah.tonemap(host(v.accum), n))
    v.restart_rendering()
    assert not host(v.stats).any() and not host(v.accum).any() and (host(v._tiles['state']) == 1).all()
    assert v.current_sample == 0 and v.is_rendering_active
