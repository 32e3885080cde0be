"""Reference side of the adaptive-sampling tests: per-sample colours from the
CPU oracle (or_trace_path) and the stats / tile arithmetic of include/ptmi.h
("Per-pixel error estimates and adaptive tile sampling") restated in numpy
f32, one rounding per operation, so every device value is compared bit for
bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from parity_helpers import scene_inputs

f32 = np.float32
_samples = {}


def oracle_samples(name, width, variant, s_begin, s_count, mask=None, seed=0, max_depth=50):
    """Colours of samples [s_begin, s_begin + s_count) of the pixels of mask
    ((H, W) bool; default: the whole image) as (s_count, H, W, 3) f32, zero
    elsewhere, and the oracle's counters summed over those paths. Cached: the
    tests share one reference per (scene, integrator, sample range, pixel set)."""
    import oracle
    sa, cam, bg = scene_inputs(name, width)
    W, H = cam['width'], cam['height']
    mask = np.ones((H, W), bool) if mask is None else np.asarray(mask, bool)
    pix = [(int(y), int(x)) for y, x in zip(*np.nonzero(mask))]
    key = (name, width, variant, s_begin, s_count, mask.tobytes(), seed, max_depth)
    if key not in _samples:
        lib = oracle.load()
        osc = oracle.OracleScene(sa)
        fr = oracle.make_frame(cam, bg, max_depth, seed, W, H)
        out = np.zeros((s_count, H, W, 3), f32)
        st = oracle.OrStats()
        v = 0 if variant == 'mk' else 1
        base, sc_p, fr_p, st_p = out.ctypes.data, C.byref(osc.s), C.byref(fr), C.byref(st)
        for s in range(s_count):
            for y, x in pix:
                lib.or_trace_path(sc_p, fr_p, v, x, y, s_begin + s, C.c_void_p(base + 12 * ((s * H + y) * W + x)), st_p)
        out.setflags(write=False)
        _samples[key] = (out, {'segments': st.segments, 'medium': st.medium, 'paths': st.paths, 'rr': st.rr,
                               'depth_cap': st.depth_cap})
    return _samples[key]


def luminance(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def accumulate(acc, stats, cols, mask=None):
    """acc += colour and the Welford update of stats = {n, mean, M2, 0}, per
    sample in order, on the pixels of mask (all by default). In place."""
    m = np.ones(acc.shape[:2], bool) if mask is None else mask
    a = acc[m]
    n, mean, m2 = stats[m][:, 0], stats[m][:, 1], stats[m][:, 2]
    with np.errstate(all='ignore'):
        for c in cols:
            c = c[m]
            a = a + c
            y = luminance(c)
            n1 = n + f32(1)
            d = y - mean
            mean1 = mean + d / n1
            m2 = m2 + d * (y - mean1)
            n, mean = n1, mean1
    assert a.dtype == f32 and m2.dtype == f32 and mean.dtype == f32
    acc[m] = a
    st = stats[m]
    st[:, 0], st[:, 1], st[:, 2] = n, mean, m2
    stats[m] = st


def pixel_error(stats):
    n, mean, m2 = stats[..., 0], stats[..., 1], stats[..., 2]
    with np.errstate(all='ignore'):
        e = np.sqrt((m2 / (n - f32(1))) / n) / (np.abs(mean) + f32(0.01))
    return np.where(n < f32(2), f32(np.inf), e).astype(f32)


def tile_lanes(w, n_rows, tw, th):
    """Per tile t = ty * tiles_x + tx: (local rows, columns, valid) of its 64 lanes."""
    tiles_x, tiles_y = -(-w // tw), -(-n_rows // th)
    p = np.arange(64)
    ty, tx = np.divmod(np.arange(tiles_x * tiles_y), tiles_x)
    lr = ty[:, None] * th + p[None, :] // tw
    col = tx[:, None] * tw + p[None, :] % tw
    return lr, col, (lr < n_rows) & (col < w), (tiles_x, tiles_y)


def tile_mask(w, n_rows, tw, th, ids):
    """(n_rows, w) mask of the pixels of the listed tiles."""
    lr, col, valid, _ = tile_lanes(w, n_rows, tw, th)
    m = np.zeros((n_rows, w), bool)
    for t in ids:
        m[lr[t][valid[t]], col[t][valid[t]]] = True
    return m


def tile_errors(stats_local, tw, th):
    """Tile errors of a frame's stats in local rows (n_rows, w, 4): lanes
    outside the frame contribute 0, xor-butterfly sum, / (float)valid lanes.
    Also each tile's n (lane 0's pixel)."""
    n_rows, w = stats_local.shape[:2]
    lr, col, valid, _ = tile_lanes(w, n_rows, tw, th)
    e = pixel_error(stats_local)
    v = np.where(valid, e[np.minimum(lr, n_rows - 1), np.minimum(col, w - 1)], f32(0)).astype(f32)
    lane = np.arange(64)
    with np.errstate(all='ignore'):
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ off]
        E = v[:, 0] / valid.sum(axis=1).astype(f32)
    assert E.dtype == f32
    return E, stats_local[lr[:, 0], col[:, 0], 0]


def tile_update(state, stats_local, tw, th, threshold, min_spp, max_spp):
    """(new state, E, ascending active ids): active' = active && n < max_spp
    && (n < min_spp || E > threshold); E = NaN gives done."""
    E, n = tile_errors(stats_local, tw, th)
    with np.errstate(all='ignore'):
        more = (n < f32(max_spp)) & ((n < f32(min_spp)) | (E > f32(threshold)))
    new = ((state != 0) & more).astype(np.int32)
    return new, E, np.flatnonzero(new).astype(np.int32)


def tonemap(acc, n):
    """u8 image with each pixel's own count: scale = f32(1.0 / max(n, 1))."""
    scale = (1.0 / np.maximum(n.astype(np.float64), 1.0)).astype(f32)[..., None]
    with np.errstate(all='ignore'):
        g = np.sqrt(np.maximum(acc * scale, f32(0))) * f32(255.999)
    return np.clip(g, 0, 255).astype(np.uint8)
