"""GPU: the per-frame image and tile kernels at the sizes where their grid caps
and list bounds start to matter, bit for bit against the numpy f32 references
of adaptive_helpers, denoise_helpers and guide_helpers over synthetic inputs or
the CPU oracle's per-sample colours. Every shape is the smallest that reaches
its path (SHAPES below; tests/test_frame_scale_shapes.py ties each to the
constant it is measured against):

* tile update, 256 x 256: 1024 tiles, the last count at which every thread of
  tile_compact's one block owns exactly one tile (per = 1).
* tile update, 197 x 325: 1025 tiles, the first count with per = 2; owner
  thread 512 holds a single tile and threads 513 .. 1023 none. Ragged right
  column and bottom row.
* tile update, 264 x 250: 1056 tiles, per = 2 with whole runs only.
* tile update, 509 x 261: 2112 tiles, the first count with per = 3 on a
  64-tile-wide grid; owner threads 704 .. 1023 are empty.
* clears, 1025 x 1024: 1,049,600 pixels, the first whole frame of that width
  past the 4096 x 256 threads of the capped grid; and a (4, 2, 1) band frame
  of 2049 x 512 owned pixels in a 2050 x 1024 image: no band frame of that
  size fits into 1025 x 1024.
* tone maps, 601 x 587: 1,058,361 elements, past the same cap with three
  elements per pixel, so a pixel's three elements can fall on two trips.
* denoiser load and store, 1025 x 1024: past 4096 blocks of 256 pixels; the
  a-trous pass is checked on the rows around pixel 4096 * 256, where the flat
  kernels' first trip ends.
* stats resolve and the listed traces, vol2_final_scene at 796 x 796: 633,616
  pixels, past the 2048 x 256 threads of the stats resolve; 100 x 100 tiles
  with a right column and a bottom row 4 pixels wide, so a list of 8599 tiles
  (550,336 items) is past the cap as well, and the adaptive loop's third pass
  compacts 10,000 tiles with per = 10.
* history validation, 80 x 50 (validate_helpers.FRAMES, run by
  test_gpu_validate.py and the CPU check program): the one frame with tiles
  whose radius-7 halo is staged unclipped.

The oracle's 796-wide camera is the compiled scene's (guide_helpers.scene_inputs:
the fixture holds cameras of 64, 800 and 1000 pixels only; at 800 the two
agree bit for bit), so its samples come from oracle.render on those inputs,
one sample per call into a zero image, as parity_helpers.oracle_render does."""
import os
import time

import numpy as np
import pytest

import adaptive_helpers as ah
import denoise_helpers as dh
import guide_helpers as gh
from parity_helpers import scene_inputs

pytestmark = pytest.mark.gpu

SCENE = 'vol2_final_scene'
f32 = np.float32

# (width, height) throughout. The one table of this module's shapes.
SHAPES = {
    'tile_update': {(256, 256): (32, 32), (197, 325): (25, 41), (264, 250): (33, 32), (509, 261): (64, 33)},
    'clear_whole': (1025, 1024),
    'clear_band': {'image': (2050, 1024), 'window': (1, 0, 2049, 1024), 'band': (4, 2, 1)},
    'tonemap': (601, 587),
    'denoise': (1025, 1024),
    'denoise_band_rows': 96,
    'resolve_width': 796,  # the frame is 796 x 796
    'resolve_tiles': (100, 100),
    'listed_skip': 7,  # the listed case drops every tile whose id is a multiple of 7
    'adaptive': {'pass_spp': 2, 'min_spp': 2, 'max_spp': 6, 'percentile': 10},
}


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def pattern(fr, c, lo):
    """A non-zero pattern no render produces (for 'this pixel was not touched')."""
    import torch
    n = fr.height * fr.width * c
    v = (torch.arange(n, dtype=torch.float32, device='cuda') % 7.0) * 0.125 + lo
    return v.reshape(fr.height, fr.width, c).contiguous()


def zeros(fr, c):
    import torch
    return torch.zeros((fr.height, fr.width, c), dtype=torch.float32, device='cuda')


def blank_frame(width, height, window=None, band=(1, 1, 0)):
    """A frame of the zero camera: for the calls that read no scene."""
    from ptmi import device
    cam = {k: np.zeros(3, f32) for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = 0.0
    return device.make_frame(cam, (0, 0, 0), 50, 0, width, height, window, band)


@pytest.fixture(scope='module')
def integ():
    """One Integrator for the synthetic cases: they read no scene."""
    from ptmi import device
    return device.Integrator(device.DeviceScene.from_arrays(scene_inputs(SCENE, 64)[0]))


# ---------------------------------------------------------------- 1: tile update past 1024 tiles
THR, LO, HI = 0.25, 4, 32


def compact_runs(ntiles, scan_block=1024):
    """(per, first tile of every owner thread's run) of tile_compact."""
    per = -(-ntiles // scan_block)
    return per, np.minimum(np.arange(scan_block + 1) * per, ntiles)


def synthetic_tile_stats(w, h):
    """(stats (h, w, 4), state0) as test_gpu_adaptive's synthetic case makes
    them, for any frame: per-tile n from a small set, a random mean and M2,
    single pixels with n < 2, an all-zero tile, a black tile without variance,
    a NaN mean, tiles at max_spp, and a random initial state with whole owner
    runs of done tiles, one owner run that stays all active and an active last
    tile."""
    lr, col, valid, (tx, ty) = ah.tile_lanes(w, h, 8, 8)
    nt = tx * ty
    per, first = compact_runs(nt)
    rng = np.random.default_rng(1000 * w + h)
    n_tile = rng.choice([0, 1, 2, 5, 16, 31, 32, 40], size=nt).astype(f32)
    zero_t, black_t, nan_t = tx + 1, 2 * tx + 3, 3 * tx + 5  # whole tiles inside the frame
    n_tile[[zero_t, black_t, nan_t]] = [0, 16, 16]
    n_tile[[0, tx - 1, nt - tx]] = [5, 16, 2]  # the corner tiles get error values
    keep = slice(first[7], first[8])  # owner 7's run: below min_spp, so all active
    n_tile[keep] = 1
    n_tile[nt - 1] = 2  # the last tile of the last non-empty run is listed
    st = np.zeros((h, w, 4), f32)
    st[lr[valid], col[valid], 0] = np.broadcast_to(n_tile[:, None], valid.shape)[valid]
    st[..., 1] = rng.uniform(-1, 2, (h, w)).astype(f32)
    st[..., 2] = (rng.uniform(0, 1, (h, w)) ** 4 * st[..., 0] * 2).astype(f32)
    st[3, 12, 0], st[20, 20, 0] = 1, 0  # single pixels with n < 2 (not lane 0 of their tiles)

    def tile_px(t):
        return lr[t][valid[t]], col[t][valid[t]]

    st[tile_px(zero_t)] = 0
    st[tile_px(black_t)] = [16, 0, 0, 0]  # sampled, black, no variance: E = 0
    y, x = tile_px(nan_t)
    st[y[9], x[9], 1] = np.nan
    state0 = (rng.uniform(size=nt) > 0.1).astype(np.int32)
    for k in rng.choice(np.flatnonzero(np.diff(first) > 0), 40, replace=False):
        state0[first[k]:first[k + 1]] = 0  # whole runs already done
    state0[[zero_t, black_t, nan_t, nt - 1]] = 1
    state0[keep] = 1
    return st, state0, dict(zero=zero_t, black=black_t, nan=nan_t, keep=keep)


@pytest.mark.parametrize('size', list(SHAPES['tile_update']), ids=lambda s: f'{s[0]}x{s[1]}')
def test_tile_update_past_one_tile_per_thread(integ, size):
    """tile_error and tile_compact against ah.tile_update on synthetic stats,
    then again on noisier stats: tiles that were done stay done."""
    import torch
    w, h = size
    tx, ty = SHAPES['tile_update'][size]
    nt = tx * ty
    fr = blank_frame(w, h)
    assert integ.tile_grid(fr) == (8, 8, tx, ty)
    st, state0, at = synthetic_tile_stats(w, h)
    new, E, act = ah.tile_update(state0, st, 8, 8, THR, LO, HI)
    # the reference alone shows the case is not degenerate
    per, first = compact_runs(nt)
    runs = [new[a:b] for a, b in zip(first[:-1], first[1:]) if b > a]
    print(f'{w}x{h}: {nt} tiles, per {per}, {len(runs)} owner threads, {len(act)} active')
    assert nt / 8 < len(act) < 7 * nt / 8
    assert any(not r.any() for r in runs) and any(r.all() for r in runs) and new[at['keep']].all()
    assert np.isnan(E[at['nan']]) and new[at['nan']] == 0 and E[at['black']] == 0 and new[at['black']] == 0
    assert np.isinf(E[at['zero']]) and new[at['zero']] == 1 and new[nt - 1] == 1
    assert (new[st[::8, ::8, 0].reshape(-1) >= HI] == 0).all()

    stats = dev(st)
    tiles = integ.new_tiles(fr)
    assert tiles['n'] == nt
    tiles['state'].copy_(torch.from_numpy(state0))
    n = integ.tile_update(fr, stats, THR, LO, HI, tiles)
    lst = host(tiles['list'])
    assert eq(host(tiles['err']), E)
    assert eq(host(tiles['state']), new)
    assert n == len(act) and eq(lst[:n], act)
    assert (np.diff(lst[:n]) > 0).all()
    assert eq(lst[n:], np.arange(n, nt))  # nothing written past the count
    # noisier stats, fewer samples: done tiles stay done
    st2 = st.copy()
    st2[..., 2] *= f32(400)
    st2[..., 0] = np.minimum(st2[..., 0], f32(8))
    stats.copy_(torch.from_numpy(st2))
    n2 = integ.tile_update(fr, stats, THR, LO, HI, tiles)
    new2, E2, act2 = ah.tile_update(new, st2, 8, 8, THR, LO, HI)
    free = ah.tile_update(np.ones(nt, np.int32), st2, 8, 8, THR, LO, HI)[0]
    assert (free > new2).any()  # some done tile would be active again without the monotone rule
    assert nt / 8 < len(act2) < 7 * nt / 8
    lst = host(tiles['list'])
    assert eq(host(tiles['err']), E2) and eq(host(tiles['state']), new2)
    assert n2 == len(act2) and eq(lst[:n2], act2) and (np.diff(lst[:n2]) > 0).all()


# ---------------------------------------------------------------- 2: flat grid-stride kernels, second trip
def clear_frames():
    w, h = SHAPES['clear_whole']
    b = SHAPES['clear_band']
    return {'whole': blank_frame(w, h), 'band': blank_frame(*b['image'], b['window'], b['band'])}


@pytest.mark.parametrize('kind', ['whole', 'band'])
def test_clears_on_their_second_trip(integ, kind):
    from ptmi import device
    fr = clear_frames()[kind]
    rows = device.frame_pixel_rows(fr)
    assert fr.w * len(rows) > 4096 * 256
    own = np.zeros((fr.height, fr.width), bool)
    own[rows, fr.x0:fr.x0 + fr.w] = True
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    assert acc_ref.all() and st_ref.all()  # the pattern has no zero
    integ.clear(fr, acc)
    integ.clear_stats(fr, stats)
    acc_ref[own] = 0
    st_ref[own] = 0
    g, s = host(acc), host(stats)
    assert eq(g, acc_ref) and eq(s, st_ref)  # the owned pixels zero, every other byte as it was
    assert eq(g == 0, np.broadcast_to(own[..., None], g.shape)) and eq(s == 0, np.broadcast_to(own[..., None], s.shape))
    assert not np.signbit(g[own]).any() and not np.signbit(s[own]).any()


def test_tonemaps_on_their_second_trip(integ):
    w, h = SHAPES['tonemap']
    rng = np.random.default_rng(23)
    a = (rng.uniform(-0.2, 3.0, (h, w, 3)) * rng.choice([1, 7, 1024], (h, w, 1))).astype(f32)
    flat = a.reshape(-1)
    hostile = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, -0.0, 1e-40], f32)
    at = rng.choice(flat.size, 4000, replace=False)
    flat[at] = rng.choice(hostile, at.size)
    flat[-3:] = [np.inf, np.nan, 2.5]  # the last pixel, on the second trip
    cnt = rng.choice([0, 1, 3, 8, 24, 1000], (h, w)).astype(f32)
    st = np.zeros((h, w, 4), f32)
    st[..., 0] = cnt
    st[..., 1:] = rng.uniform(-1, 1, (h, w, 3)).astype(f32)  # read by nothing
    acc, stats = dev(a), dev(st)
    with np.errstate(invalid='ignore'):  # the reference casts NaN to u8 as the kernel does: 0
        want_stats = ah.tonemap(a, cnt)
        want_spp = {spp: ah.tonemap(a, np.full((h, w), spp, f32)) for spp in (1, 7)}
    img = host(integ.tonemap(acc, stats=stats))
    assert eq(img, want_stats)
    assert set(np.unique(cnt)) == {0, 1, 3, 8, 24, 1000} and len(np.unique(img)) > 200
    for spp, want in want_spp.items():
        assert eq(host(integ.tonemap(acc, spp)), want)
    assert not eq(want_spp[1], want_spp[7])


_dn = {}


def denoise_inputs():
    """(accum, stats, guides, invalid pixels) at SHAPES['denoise'], made once."""
    if not _dn:
        w, h = SHAPES['denoise']
        t0 = time.perf_counter()
        accum, stats, invalid = dh.synthetic(w, h, seed=w * 1000 + h)
        guides = gh.synthetic_guides(w, h, seed=w * 1000 + h)
        print(f'synthetic {w}x{h}: {time.perf_counter() - t0:.2f} s')
        for a in (accum, stats, guides):
            a.setflags(write=False)
        _dn['in'] = (accum, stats, guides, invalid)
    return _dn['in']


def test_denoiser_load_and_store_on_their_second_trip(integ):
    """iterations = 0: dn_load and dn_store alone, unguided and guided with
    and without the demodulation."""
    accum, stats, guides, invalid = denoise_inputs()
    assert accum.shape[0] * accum.shape[1] > 4096 * 256
    a, s, g = dev(accum), dev(stats), dev(guides)
    c0, v0 = dh.load(accum, stats)
    rgb, var = integ.denoise(a, s, 0, 4.0)
    assert eq(host(rgb), c0) and eq(host(var), v0)
    for p in invalid:
        assert not (np.isfinite(dh.lum(c0[p])) and np.isfinite(v0[p]))
    for demodulate in (True, False):
        want = gh.denoise_guided(accum, stats, guides, iterations=0, demodulate=demodulate)
        rgb, var = integ.denoise_guided(a, s, g, 0, demodulate=demodulate)
        assert eq(host(rgb), want[0]) and eq(host(var), want[1]), demodulate
        assert eq(want[0], c0) != demodulate  # the demodulation rounds; without it the load itself


def trip_band(w, h):
    """Image rows [lo, hi): SHAPES['denoise_band_rows'] rows around the row of
    pixel 4096 * 256, cut to the image."""
    mid, half = (4096 * 256) // w, SHAPES['denoise_band_rows'] // 2
    return max(0, mid - half), min(h, mid + half)


@pytest.mark.parametrize('guided', [False, True], ids=['unguided', 'guided'])
def test_one_pass_where_the_first_trip_ends(integ, guided):
    """One a-trous pass behind the flat load and before the flat store, against
    the numpy pass on the band of rows where the flat kernels' first trip ends
    plus the two rows the pass reads on either side of it."""
    accum, stats, guides, _ = denoise_inputs()
    h, w = stats.shape[:2]
    lo, hi = trip_band(w, h)
    assert lo < (4096 * 256) // w < hi and hi - lo >= SHAPES['denoise_band_rows'] // 2
    a, s = dev(accum), dev(stats)
    if guided:
        rgb, var = integ.denoise_guided(a, s, dev(guides), 1)
    else:
        rgb, var = integ.denoise(a, s, 1, 4.0)
    top, bottom = max(0, lo - 2), min(h, hi + 2)  # a step-1 pass reads two rows up and down
    rows = slice(top, bottom)
    if guided:
        want = gh.denoise_guided(accum[rows], stats[rows], guides[rows], iterations=1)
    else:
        want = dh.denoise(accum[rows], stats[rows], 1, 4.0)
    cut = slice(lo - top, hi - top)
    assert eq(host(rgb)[lo:hi], want[0][cut]) and eq(host(var)[lo:hi], want[1][cut])
    loaded = dh.load(accum[lo:hi], stats[lo:hi])[0]
    assert not eq(want[0][cut], loaded)  # the pass did filter


# ---------------------------------------------------------------- 3: stats resolve and listed traces, 796 x 796
W3 = SHAPES['resolve_width']
_oracle = {}


def inputs3():
    """(SceneArrays, camera upload dict, background) of the scene at 796 pixels."""
    return gh.scene_inputs(SCENE, W3)


def oracle_cols(variant, s_begin, s_count):
    """(s_count, 796, 796, 3) f32: the oracle's colours of samples [s_begin,
    s_begin + s_count) of every pixel, one render of one sample into a zero
    image each; cached per variant and sample."""
    import oracle
    sa, cam, bg = inputs3()
    W, H = cam['width'], cam['height']
    todo = [s for s in range(s_begin, s_begin + s_count) if (variant, s) not in _oracle]
    if todo:
        if 'scene' not in _oracle:
            _oracle['scene'] = oracle.OracleScene(sa)
        fr = oracle.make_frame(cam, bg, 50, 0, W, H)
        t0 = time.perf_counter()
        for s in todo:
            img = np.zeros((H, W, 3), f32)
            st = oracle.render(_oracle['scene'], fr, variant, img, (0, 0, W, H), s, 1,
                               threads=min(16, os.cpu_count() or 1))
            assert st['paths'] == W * H
            img.setflags(write=False)
            _oracle[variant, s] = img
        print(f'oracle {variant}: samples {todo} of {W}x{H} in {time.perf_counter() - t0:.2f} s')
    return np.stack([_oracle[variant, s] for s in range(s_begin, s_begin + s_count)])


@pytest.fixture(scope='module')
def integ3():
    from ptmi import device
    return device.Integrator(device.DeviceScene.from_arrays(inputs3()[0]))


def frame3():
    from ptmi import device
    _, cam, bg = inputs3()
    assert (cam['width'], cam['height']) == (W3, W3)
    return device.make_frame(cam, bg, 50, 0, W3, W3)


def render_stats(integ, variant):
    return integ.render_mk_stats if variant == 'mk' else integ.render_wf_stats


@pytest.mark.parametrize('variant', ['mk', 'wf'])
def test_stats_resolve_whole_frame(integ3, variant):
    """stats_resolve<false> past its grid: samples 0 - 1 in one call and as two
    calls, against the plain render and the reference."""
    integ, fr = integ3, frame3()
    npix = W3 * W3
    assert npix > 2048 * 256 and integ.tile_grid(fr) == (8, 8) + SHAPES['resolve_tiles']
    cols = oracle_cols(variant, 0, 2)
    acc_ref, st_ref = np.zeros((W3, W3, 3), f32), np.zeros((W3, W3, 4), f32)
    ah.accumulate(acc_ref, st_ref, cols)
    plain = zeros(fr, 3)
    (integ.render_mk if variant == 'mk' else integ.render_wf)(fr, plain, 0, 2)
    plain = host(plain)
    for calls in ([(0, 2)], [(0, 1), (1, 1)]):
        acc, stats = zeros(fr, 3), zeros(fr, 4)
        integ.reset_counters()
        for b, c in calls:
            render_stats(integ, variant)(fr, acc, stats, b, c)
        g, s = host(acc), host(stats)
        assert eq(g, plain), calls
        assert eq(g, acc_ref), calls
        assert eq(s, st_ref), calls
        assert integ.read_counters()['paths'] == 2 * npix
    assert (st_ref[..., 0] == 2).all() and (st_ref[..., 3] == 0).all()


def listed_ids(ntiles, tiles_x):
    """Every tile whose id is no multiple of SHAPES['listed_skip'], and with
    them the last tile, the partial right column and the partial bottom row."""
    t = np.arange(ntiles)
    keep = (t % SHAPES['listed_skip'] != 0) | (t % tiles_x == tiles_x - 1) | (t >= ntiles - tiles_x)
    return t[keep].astype(np.int32)


@pytest.mark.parametrize('variant', ['mk', 'wf'])
def test_listed_trace_past_8192_tiles(integ3, variant):
    """Samples 0 - 1 on the whole frame, then 2 - 3 on a list of more than 8192
    tiles with three ids outside the grid in it: the listed pixels advance to
    n = 4, every other byte stays."""
    integ, fr = integ3, frame3()
    tx, ty = SHAPES['resolve_tiles']
    nt = tx * ty
    ids = listed_ids(nt, tx)
    assert 64 * len(ids) > 2048 * 256 and len(ids) < nt
    assert len(ids) >= nt - (nt + 6) // 7 and {nt - 1, tx - 1, nt - tx} <= set(ids.tolist())
    dev_list = dev(np.concatenate([ids[:5], [-3, nt, 1 << 30], ids[5:]]).astype(np.int32))
    listed = ah.tile_mask(W3, W3, 8, 8, ids)
    assert listed[:, -4:].all() and listed[-4:, :].all() and not listed.all()
    cols = oracle_cols(variant, 0, 4)
    acc_ref, st_ref = np.zeros((W3, W3, 3), f32), np.zeros((W3, W3, 4), f32)
    ah.accumulate(acc_ref, st_ref, cols[:2])
    acc, stats = zeros(fr, 3), zeros(fr, 4)
    integ.reset_counters()
    render_stats(integ, variant)(fr, acc, stats, 0, 2)
    before = host(acc).copy(), host(stats).copy()
    assert eq(before[0], acc_ref) and eq(before[1], st_ref)
    render_stats(integ, variant)(fr, acc, stats, 2, 2, tiles=(dev_list, dev_list.numel()))
    ah.accumulate(acc_ref, st_ref, cols[2:4], listed)
    g, s = host(acc), host(stats)
    assert eq(g[listed], acc_ref[listed]) and eq(s[listed], st_ref[listed])
    assert g[~listed].tobytes() == before[0][~listed].tobytes()
    assert s[~listed].tobytes() == before[1][~listed].tobytes()
    assert (s[..., 0][listed] == 4).all() and (s[..., 0][~listed] == 2).all()
    assert integ.read_counters()['paths'] == int(st_ref[..., 0].sum()) == 2 * W3 * W3 + 2 * int(listed.sum())


_loops = {}


def clear_threshold(E, percentile):
    """The percentile of the positive finite tile errors E, moved to the middle
    of the nearest gap between two distinct values of E that keeps every E
    further than 2e-3 of the threshold away (twice the margin asserted). The
    tiles with E == 0 are left out: no threshold keeps them active."""
    fin = E[np.isfinite(E)].astype(np.float64)
    p, u = np.percentile(fin[fin > 0], percentile), np.unique(fin)
    mid, gap = (u[:-1] + u[1:]) / 2, np.diff(u)
    ok = np.flatnonzero(gap / 2 > 2e-3 * mid)
    return float(f32(mid[ok[np.argmin(np.abs(mid[ok] - p))]]))


def reference_loop(variant):
    """The adaptive loop in numpy on the oracle's samples at 796 x 796: (threshold,
    per-pass (list before, state, E, list after, accum, stats), the last
    pass's being the loop's result). The threshold comes from the tile errors
    the reference has after the first pass."""
    if variant not in _loops:
        prm = SHAPES['adaptive']
        per, lo, hi = prm['pass_spp'], prm['min_spp'], prm['max_spp']
        tx, ty = SHAPES['resolve_tiles']
        nt = tx * ty
        cols = oracle_cols(variant, 0, hi)
        acc_ref, st_ref = np.zeros((W3, W3, 3), f32), np.zeros((W3, W3, 4), f32)
        state, act = np.ones(nt, np.int32), np.arange(nt, dtype=np.int32)
        ref, thr = [], None
        for k in range(hi // per):
            if len(act) == 0:
                break
            before = act
            ah.accumulate(acc_ref, st_ref, cols[k * per:(k + 1) * per], ah.tile_mask(W3, W3, 8, 8, act))
            if thr is None:
                thr = clear_threshold(ah.tile_errors(st_ref, 8, 8)[0], prm['percentile'])
            state, E, act = ah.tile_update(state, st_ref, 8, 8, thr, lo, hi)
            ref.append((before, state.copy(), E, act, acc_ref.copy(), st_ref.copy()))
        _loops[variant] = (thr, ref)
    return _loops[variant]


@pytest.mark.parametrize('variant', ['mk', 'wf'])
def test_adaptive_loop_at_frame_scale(integ3, variant):
    """The adaptive loop (pass_spp 2, min_spp 2, max_spp 6) with every pass
    listed, the first one with all 10,000 tiles: per-pass active lists, tile
    states and errors, accum, stats and path counts, and the per-pixel tone map
    at the end.

    After two samples 5108 ('mk') and 5124 ('wf') of the 10,000 tiles have
    E == 0 exactly (every pixel black twice) and end there whatever the
    threshold, so no second pass of this scene lists more than 8192 tiles: the
    list past the stats resolve's grid is the first pass's here (and
    test_listed_trace_past_8192_tiles' 8599 with gaps), and the threshold is
    the 10th percentile of the positive errors, which leaves the second and
    third lists (4251 and 4247 tiles for 'mk', 4215 and 4211 for 'wf') past
    tile_compact's one tile per thread and different from each other."""
    integ, fr = integ3, frame3()
    prm = SHAPES['adaptive']
    per, lo, hi = prm['pass_spp'], prm['min_spp'], prm['max_spp']
    tx, ty = SHAPES['resolve_tiles']
    nt = tx * ty
    thr, ref = reference_loop(variant)
    # the reference alone shows which paths the passes reach
    counts = [len(r[0]) for r in ref]
    print(f'{variant}: threshold {thr!r}, tiles listed per pass {counts}, active after the last {len(ref[-1][3])}')
    zero = int((ref[0][2] == 0).sum())
    print(f'{variant}: {zero} tiles with E == 0 after the first pass')
    assert len(counts) == 3 and counts[0] == nt == 10000 > 8192  # the listed resolve's and traces' second trip
    assert nt - zero < 8192  # why the second list cannot be that long
    assert 1024 < counts[2] < counts[1] < nt - zero  # tile_compact with per = 10, its list past one block's threads
    for r in ref:
        fin = r[2][np.isfinite(r[2])]
        assert (np.abs(fin - f32(thr)) > 1e-3 * thr).all()
    acc, stats = zeros(fr, 3), zeros(fr, 4)
    tiles = integ.new_tiles(fr)
    integ.reset_counters()
    for k, (before, state_k, E, after, acc_k, st_k) in enumerate(ref):
        assert tiles['n'] == len(before) and eq(host(tiles['list'])[:tiles['n']], before), k
        render_stats(integ, variant)(fr, acc, stats, k * per, per, tiles=(tiles['list'], tiles['n']))
        assert eq(host(acc), acc_k) and eq(host(stats), st_k), k
        assert integ.read_counters()['paths'] == int(st_k[..., 0].sum()), k
        n = integ.tile_update(fr, stats, thr, lo, hi, tiles)
        assert n == len(after), k
        assert eq(host(tiles['state']), state_k) and eq(host(tiles['err']), E), k
        assert eq(host(tiles['list'])[:n], after) and (np.diff(after) > 0).all(), k
    acc_ref, st_ref = ref[-1][4], ref[-1][5]
    assert len(np.unique(st_ref[..., 0])) == 3 and st_ref[..., 0].max() == hi
    assert eq(host(integ.tonemap(acc, stats=stats)), ah.tonemap(acc_ref, st_ref[..., 0]))
