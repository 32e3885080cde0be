"""GPU: tile-listed wavefront batches (include/ptmi_wf_tiles.h), bit for bit
against numpy f32 over the CPU oracle's per-sample wavefront colours
(adaptive_helpers) or against the unlisted wavefront: the listed trace, short
lists and odd sample counts, batch halving, the tail launch, ragged and banded
frames, every traversal rung, the adaptive loop end to end and the renderer."""
import ctypes as C
import random

import numpy as np
import pytest

import adaptive_helpers as ah
from parity_helpers import scene_inputs

pytestmark = pytest.mark.gpu

SCENE = 'vol2_final_scene'
f32 = np.float32
IDS = np.array(list(range(1, 64, 3)) + [63], np.int32)  # 22 of the 64 tiles of the 64 x 64 frame


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope='module')
def integs():
    """One Integrator for the module: the scene arrays do not depend on the camera width."""
    from ptmi import device
    sa = scene_inputs(SCENE, 64)[0]
    return device.Integrator(device.DeviceScene.from_arrays(sa))


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


def dev(ids):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()


def listed_mask():
    return ah.tile_mask(64, 64, 8, 8, IDS)


def with_strays(ids):
    """The list with ids outside the grid interleaved: they are ignored on the device."""
    return np.concatenate([ids[:5], [-3, 64, 1 << 30], ids[5:]]).astype(np.int32)


def c_render_tiles(integ, fr, ws, ws_bytes, acc, stats, tl, n, s0, sc):
    from ptmi import wf_tiles
    return wf_tiles.load().ptmi_wf_render_tiles_stats(
        C.byref(integ.scene.view), C.byref(fr), C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(acc.data_ptr()),
        C.c_void_p(stats.data_ptr()), C.c_void_p(tl.data_ptr()), n, s0, sc, integ._cnt(), None)


# ---------------------------------------------------------------- 1, 4: listed trace, the tail
def listed_trace(integ):
    fr = make(64)
    assert len(IDS) == 22
    dev_list = dev(with_strays(IDS))
    listed = listed_mask()
    cols, ost = ah.oracle_samples(SCENE, 64, 'wf', 0, 4, mask=listed)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    ws = integ.workspace(fr, 4)
    ws.fill_(float('nan'))
    integ.reset_counters()
    # an empty list is a no-op
    integ.render_wf_stats(fr, acc, stats, 0, 4, tiles=(dev_list, 0))
    assert c_render_tiles(integ, fr, ws, ws.numel() * 4, acc, stats, dev_list, 0, 0, 4) == 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref) and integ.read_counters()['paths'] == 0
    assert np.isnan(host(ws)).all()
    integ.render_wf_stats(fr, acc, stats, 0, 4, tiles=(dev_list, dev_list.numel()))
    ah.accumulate(acc_ref, st_ref, cols, listed)
    g, s = host(acc), host(stats)
    assert eq(g[listed], acc_ref[listed]) and eq(s[listed], st_ref[listed])
    assert eq(g[~listed], acc_ref[~listed]) and eq(s[~listed], st_ref[~listed])  # the pattern, untouched
    assert np.isfinite(g).all() and np.isfinite(s).all()
    cnt = integ.read_counters()
    assert cnt['paths'] == 64 * 22 * 4
    assert cnt == {k: int(v) for k, v in ost.items()}
    return g, s, cnt


def test_listed_trace_wf(integs):
    listed_trace(integs)


def test_listed_trace_wf_tail(integs):
    """The same under the one-launch tail as soon as the pool is dry (drain_at
    1) and without it (0): identical results."""
    integ = integs
    prev = integ.lib.ptmi_wf_set_drain_at(1)
    try:
        assert prev >= 0
        a = listed_trace(integ)
        tail1 = integ.tail_segments()
        assert integ.lib.ptmi_wf_set_drain_at(0) == 1
        b = listed_trace(integ)
        tail0 = integ.tail_segments()
    finally:
        integ.lib.ptmi_wf_set_drain_at(prev)
    assert eq(a[0], b[0]) and eq(a[1], b[1]) and a[2] == b[2]
    assert tail1 > 0 and tail0 == 0  # the tail launch ran, and did not


# ---------------------------------------------------------------- 2: short lists, odd sample counts
@pytest.mark.parametrize('s_begin', [0, 5], ids=['from0', 'from5'])
@pytest.mark.parametrize('s_count', [1, 3, 5], ids=['s1', 's3', 's5'])
@pytest.mark.parametrize('n_tiles', [1, 7, 9], ids=['n1', 'n7', 'n9'])
def test_short_lists(integs, n_tiles, s_count, s_begin):
    """Fewer tiles than pool shards (8) and no multiple of them; fewer samples
    than a chunk holds (4) and no multiple of that."""
    integ = integs
    fr = make(64)
    ids = {1: IDS[3:4], 7: IDS[0:21:3][::-1], 9: IDS[1:19:2]}[n_tiles]  # (not ascending: the order is free)
    assert len(ids) == n_tiles and len(set(ids.tolist())) == n_tiles
    sub = ah.tile_mask(64, 64, 8, 8, ids)
    cols, _ = ah.oracle_samples(SCENE, 64, 'wf', 0, 10, mask=listed_mask())
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    integ.reset_counters()
    integ.render_wf_stats(fr, acc, stats, s_begin, s_count, tiles=(dev(ids), n_tiles))
    ah.accumulate(acc_ref, st_ref, cols[s_begin:s_begin + s_count], sub)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert integ.read_counters()['paths'] == 64 * n_tiles * s_count


# ---------------------------------------------------------------- 3: batch halving
def test_batch_halving(integs):
    """5 samples through a workspace that holds 2: batches of 2, 2 and 1."""
    import torch
    integ = integs
    fr = make(64)
    need = int(integ.lib.ptmi_wf_workspace_bytes(fr, 2))
    assert 0 < need < int(integ.lib.ptmi_wf_workspace_bytes(fr, 3))
    ws = torch.full(((need + 3) // 4,), float('nan'), dtype=torch.float32, device='cuda')
    listed = listed_mask()
    cols, _ = ah.oracle_samples(SCENE, 64, 'wf', 0, 10, mask=listed)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    dev_list = dev(with_strays(IDS))
    integ.reset_counters()
    assert c_render_tiles(integ, fr, ws, need, acc, stats, dev_list, dev_list.numel(), 0, 5) == 0
    ah.accumulate(acc_ref, st_ref, cols[:5], listed)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert integ.read_counters()['paths'] == 64 * 22 * 5
    # one byte less no longer holds two samples: batches of one still do
    acc2, st2 = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    assert c_render_tiles(integ, fr, ws, need - 16, acc2, st2, dev_list, dev_list.numel(), 0, 5) == 0
    assert eq(host(acc2), acc_ref) and eq(host(st2), st_ref)


# ---------------------------------------------------------------- 5: ragged frame
def test_ragged_frame(integs):
    """A 53 x 37 window: 7 x 5 tiles, the right column 5 pixels wide, the bottom row 5 high."""
    integ = integs
    fr = make(64, window=(5, 9, 53, 37))
    assert integ.tile_grid(fr) == (8, 8, 7, 5)
    ids = np.array([34, 0, 6, 28, 3, 13, 31, 14, 17], np.int32)  # corners, edges, one inside
    local = ah.tile_mask(53, 37, 8, 8, ids)
    assert local.sum() == 64 * 4 + 40 * 4 + 25  # tiles 0, 3, 14, 17 whole; 6, 13, 28, 31 cut once; 34 twice
    listed = np.zeros((64, 64), bool)
    listed[9:46, 5:58] = local
    whole = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    part = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    pat = [host(t).copy() for t in part]
    integ.render_wf_stats(fr, *whole, 2, 5)
    integ.reset_counters()
    integ.render_wf_stats(fr, *part, 2, 5, tiles=(dev(ids), len(ids)))
    window = np.zeros((64, 64), bool)
    window[9:46, 5:58] = True
    for got, ref, untouched in zip(part, whole, pat):
        got, ref = host(got), host(ref)
        assert eq(got[listed], ref[listed])
        assert eq(got[~listed], untouched[~listed])
        assert not eq(ref[window & ~listed], untouched[window & ~listed])  # the unlisted render did render there
        assert eq(ref[~window], untouched[~window])
    assert integ.read_counters()['paths'] == int(listed.sum()) * 5


# ---------------------------------------------------------------- 6: banded window
def test_banded_window(integs):
    """16 x 4 tiles on a 2-rank band frame whose window width (80) is no
    multiple of 16: a whole-frame wavefront stats render of samples 0..3, a
    listed one of every second tile for 4..7, then the tile update."""
    from ptmi import device
    integ = integs
    fr = make(800, (96, 200, 80, 40), (4, 2, 1))
    assert integ.tile_grid(fr) == (16, 4, 5, 5)
    owned = device.frame_pixel_rows(fr)
    assert len(owned) == 20
    own = np.zeros((800, 800), bool)
    own[owned, 96:176] = True
    cols, _ = ah.oracle_samples(SCENE, 800, 'wf', 0, 8, mask=own)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    integ.clear(fr, acc)
    integ.clear_stats(fr, stats)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    integ.render_wf_stats(fr, acc, stats, 0, 4)
    ah.accumulate(acc_ref, st_ref, cols[:4], own)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    ids = np.arange(0, 25, 2, dtype=np.int32)
    local = ah.tile_mask(80, 20, 16, 4, ids)
    listed = np.zeros((800, 800), bool)
    lr, lc = np.nonzero(local)
    listed[owned[lr], 96 + lc] = True
    integ.reset_counters()
    integ.render_wf_stats(fr, acc, stats, 4, 4, tiles=(dev(ids), len(ids)))
    ah.accumulate(acc_ref, st_ref, cols[4:8], listed)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert set(np.unique(st_ref[own][:, 0])) == {4.0, 8.0}
    assert integ.read_counters()['paths'] == int(listed.sum()) * 4
    tiles = integ.new_tiles(fr)
    n = integ.tile_update(fr, stats, 0.5, 6, 64, tiles)
    new, E, act = ah.tile_update(np.ones(25, np.int32), st_ref[owned][:, 96:176], 16, 4, 0.5, 6, 64)
    assert eq(host(tiles['err']), E) and eq(host(tiles['state']), new)
    assert n == len(act) and eq(host(tiles['list'])[:n], act)


BANDS = [(4, 2, 1), (2, 2, 1), (1, 2, 0)]


@pytest.mark.parametrize('band', BANDS, ids=lambda b: '%dx%d' % (64 // b[0], b[0]))
def test_banded_window_shapes(integs, band):
    """The wavefront stats render on a 2-rank band frame, every tile shape a banded frame can have
    (16 x 4, 32 x 2, 64 x 1): the 64 x 64 image, window x0 = 3, y0 = 2, 37 x 24
    (12 owned rows, a ragged right edge), 3 samples on the whole frame, then 3
    on a list of every second tile, an id outside the grid and the last (edge)
    tile, then the tile update; bit for bit against the oracle."""
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
    cols, _ = ah.oracle_samples(SCENE, 64, 'wf', 0, 6, mask=own)
    acc, stats = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    integ.clear(fr, acc)
    integ.clear_stats(fr, stats)
    acc_ref, st_ref = host(acc).copy(), host(stats).copy()
    integ.render_wf_stats(fr, acc, stats, 0, 3)
    ah.accumulate(acc_ref, st_ref, cols[:3], own)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    ids = np.array(list(range(0, nt - 1, 2)) + [nt, nt - 1], np.int32)
    local = ah.tile_mask(w, 12, tw, th, ids[ids < nt])
    listed = np.zeros((fr.height, fr.width), bool)
    lr, lc = np.nonzero(local)
    listed[owned[lr], x0 + lc] = True
    integ.reset_counters()
    integ.render_wf_stats(fr, acc, stats, 3, 3, tiles=(dev(ids), len(ids)))
    ah.accumulate(acc_ref, st_ref, cols[3:6], listed)
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert set(np.unique(st_ref[own][:, 0])) == {3.0, 6.0}
    assert integ.read_counters()['paths'] == int(listed.sum()) * 3
    tiles = integ.new_tiles(fr)
    n = integ.tile_update(fr, stats, 0.5, 6, 64, tiles)
    new, E, act = ah.tile_update(np.ones(nt, np.int32), st_ref[owned][:, x0:x0 + w], tw, th, 0.5, 6, 64)
    assert eq(host(tiles['err']), E) and eq(host(tiles['state']), new)
    assert n == len(act) and eq(host(tiles['list'])[:n], act)


# ---------------------------------------------------------------- 7: every rung
def _rung(slots):
    """The wavefront's traversal kernel for max_leaf_depth + 1 stack slots (the coarse ladder)."""
    return next((r for r in (16, 20, 24, 32, 64) if slots <= r and slots <= 63), 'reference walk')


@pytest.mark.parametrize('name,traversal,rung', [
    ('chain17', 'stack', 20), ('chain18', 'stack', 20), ('chain19', 'stack', 20), ('chain20', 'stack', 20),
    ('chain22', 'stack', 24), ('chain29', 'stack', 32), ('chain52', 'stack', 64),
    ('chainx70', 'stack', 'reference walk'), ('chain22', 'stackless', 24)])
def test_listed_wf_on_every_traversal_rung(name, traversal, rung):
    """The listed wavefront of every rung of the traversal dispatch but the
    16-slot one (test_listed_trace_wf) against the unlisted wavefront, which
    test_gpu_edge ties to the oracle: bit-equal on the listed tiles, nothing
    else touched. 32 x 18: 4 x 3 tiles of 8 x 8, the last row 2 pixels high."""
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
    dev_list = dev([1, -3, 4, 6, 12, 9, 1 << 30, 11])  # 3 ids outside the grid
    listed = ah.tile_mask(W, H, 8, 8, ids)
    assert listed.sum() == 64 * 3 + 16 * 2  # tiles 9 and 11 are 8 x 2
    whole = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    part = pattern(fr, 3, 0.5), pattern(fr, 4, 1.25)
    pat = [host(t).copy() for t in part]
    integ.render_wf_stats(fr, *whole, 0, spp)
    integ.reset_counters()
    integ.render_wf_stats(fr, *part, 0, spp, tiles=(dev_list, dev_list.numel()))
    for got, ref, untouched in zip(part, whole, pat):
        got, ref = host(got), host(ref)
        assert eq(got[listed], ref[listed])
        assert eq(got[~listed], untouched[~listed])
        assert not eq(ref[~listed], untouched[~listed])  # the unlisted render did render there
    assert integ.read_counters()['paths'] == int(listed.sum()) * spp


# ---------------------------------------------------------------- 8: adaptive end to end
THR, PER, LO, HI = 0.05, 8, 8, 32
_loop = {}


def reference_loop():
    """The adaptive loop in numpy on the oracle's wavefront samples, shared by cases 8 and 9."""
    if not _loop:
        cols, _ = ah.oracle_samples(SCENE, 64, 'wf', 0, HI)
        acc_ref, st_ref = np.zeros((64, 64, 3), f32), np.zeros((64, 64, 4), f32)
        state, act = np.ones(64, np.int32), np.arange(64, dtype=np.int32)
        ref = []
        for k in range(HI // PER):
            if len(act) == 0:
                break
            before = act
            ah.accumulate(acc_ref, st_ref, cols[k * PER:(k + 1) * PER], ah.tile_mask(64, 64, 8, 8, act))
            state, E, act = ah.tile_update(state, st_ref, 8, 8, THR, LO, HI)
            ref.append((before, state.copy(), E, act))
        for a in (acc_ref, st_ref):
            a.setflags(write=False)
        _loop.update(ref=ref, acc=acc_ref, stats=st_ref)
    return _loop['ref'], _loop['acc'], _loop['stats']


def test_adaptive_end_to_end_wf(integs):
    """The adaptive loop (pass_spp 8, min_spp 8, max_spp 32, target 0.05) with
    the listed wavefront and in numpy on the oracle's 'wf' samples: per-pass
    active sets, tile states and errors, accum, stats, the per-pixel tone map
    and the path count."""
    integ = integs
    fr = make(64)
    ref, acc_ref, st_ref = reference_loop()
    # the case must not degenerate
    counts = [len(r[0]) for r in ref]
    assert counts[0] == 64 and 8 <= 64 - len(ref[0][3]) <= 56, counts
    assert counts == [64, 39, 39, 38] and len(ref[-1][3]) == 0
    for _, _, E, _ in ref:
        fin = E[np.isfinite(E)]
        assert (np.abs(fin - f32(THR)) > 1e-3 * THR).all()
    assert 64 * PER * sum(counts) == 92160 < 64 * 64 * HI == 131072
    # device loop
    acc, stats = zeros(fr, 3), zeros(fr, 4)
    tiles = integ.new_tiles(fr)
    integ.reset_counters()
    for k, (before, st_k, E, after) in enumerate(ref):
        assert tiles['n'] == len(before) and eq(host(tiles['list'])[:tiles['n']], before)
        sel = None if tiles['n'] == 64 else (tiles['list'], tiles['n'])
        integ.render_wf_stats(fr, acc, stats, k * PER, PER, tiles=sel)
        n = integ.tile_update(fr, stats, THR, LO, HI, tiles)
        assert n == len(after)
        assert eq(host(tiles['state']), st_k) and eq(host(tiles['err']), E)
    assert tiles['n'] == 0
    assert eq(host(acc), acc_ref) and eq(host(stats), st_ref)
    assert integ.read_counters()['paths'] == int(st_ref[..., 0].sum()) == 92160
    assert eq(host(integ.tonemap(acc, stats=stats)), ah.tonemap(acc_ref, st_ref[..., 0]))


# ---------------------------------------------------------------- 9: renderer
def _renderer(tmp_path, spp=32):
    from ptmi import scenes
    from ptmi.renderer import MI355XRenderer
    random.seed(1234)
    sc = scenes.vol2_final_scene(width=64)
    sc.cam.samples_per_pixel = spp
    r = MI355XRenderer(sc.world, sc.cam, str(tmp_path / 'a.png'))
    r.background_color = sc.background
    r.max_depth = sc.max_depth
    return r


def test_render_adaptive_wavefront_tiles(tmp_path, capsys):
    r = _renderer(tmp_path)
    kw = dict(target_error=THR, pass_spp=PER, min_spp=LO, max_spp=HI, integrator='wavefront')
    ref, acc_ref, st_ref = reference_loop()
    r.render_adaptive(tiles=True, **kw)
    a, s = host(r.accum).copy(), host(r.stats).copy()
    n = r.sample_count_map()
    passes = [dict(p) for p in r.adaptive_passes]
    assert len(np.unique(n)) > 1 and eq(n, s[..., 0])
    assert eq(a, acc_ref) and eq(s, st_ref)
    assert [p['active_tiles'] for p in passes] == [len(q[0]) for q in ref]
    assert [p['traced'] for p in passes] == [64 * len(q[0]) * PER for q in ref]
    assert sum(p['traced'] for p in passes) == 92160 == r.integrator.read_counters()['paths']
    out = capsys.readouterr().out
    assert 'Adaptive passes' in out and f'{64 * 39 * PER:13,}' in out  # the passes table shows the listed passes
    # checkpoint after pass 2, resume: bit-identical
    ck = str(tmp_path / 'wf_tiles.npz')
    r.checkpoint_path, r.checkpoint_every = ck, 2
    r.render_adaptive(tiles=True, **kw)
    r.checkpoint_path = None
    assert eq(host(r.accum), a)
    with np.load(ck) as z:
        assert int(z['next_sample']) == 16 and z['adaptive'].size == 5 and z['adaptive'][4] == 1.0
        assert z['tile_state'].sum() == passes[2]['active_tiles']
        old = {k: z[k] for k in z.files}
    r.clear_accumulation_buffer()
    r.load_checkpoint(ck)
    r.render_adaptive(resume=True, tiles=True, **kw)
    assert eq(host(r.accum), a) and eq(host(r.stats), s)
    assert [p['traced'] for p in r.adaptive_passes] == [p['traced'] for p in passes]
    # resuming under the other setting raises
    r.load_checkpoint(ck)
    with pytest.raises(ValueError, match='adaptive differs'):
        r.render_adaptive(resume=True, **kw)
    r.load_checkpoint(ck)
    with pytest.raises(ValueError, match='adaptive differs'):
        r.render_adaptive(resume=True, tiles=False, **kw)
    # a checkpoint written without the flag loads as the integrator's default: whole frames
    old['adaptive'] = old['adaptive'][:4]
    legacy = str(tmp_path / 'legacy.npz')
    np.savez(legacy, **old)
    r.load_checkpoint(legacy)
    with pytest.raises(ValueError, match='adaptive differs'):
        r.render_adaptive(resume=True, tiles=True, **kw)
    r.load_checkpoint(legacy)
    r.render_adaptive(resume=True, **kw)  # accepted (the state is the listed render's: only the acceptance is checked)
    # the megakernel always lists
    with pytest.raises(ValueError, match='tiles=False'):
        r.render_adaptive(**dict(kw, integrator='megakernel'), tiles=False)
    # the default call still renders whole frames
    r.render_adaptive(**kw)
    nw = r.sample_count_map()
    assert (nw == nw[0, 0]).all() and r.current_sample == int(nw[0, 0]) <= 32
    assert all(p['traced'] == 64 * 64 * PER for p in r.adaptive_passes)
