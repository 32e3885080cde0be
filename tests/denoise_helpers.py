"""numpy f32 reference of the denoiser's contract (include/ptmi_post.h): straight
loops over the taps, vectorised over the pixels, one f32 rounding per operation
in the order the contract writes them. Plus the synthetic inputs the CPU and
GPU tests share."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
K = (f32(0.375), f32(0.25), f32(0.0625))
G = (f32(0.5), f32(0.25))


def lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def finite(x):
    with np.errstate(invalid='ignore'):
        return np.abs(x) <= FLT_MAX  # False for NaN


def load(accum, stats):
    """accum (H, W, 3) and stats (H, W, 4) to the working colour and variance."""
    accum, stats = np.asarray(accum, f32), np.asarray(stats, f32)
    n, m2 = stats[..., 0], stats[..., 2]
    with np.errstate(all='ignore'):
        nn = np.where(n > 1, n, f32(1))  # max(n, 1); a NaN n gives 1
        scale = (1.0 / nn.astype(np.float64)).astype(f32)
        c = accum * scale[..., None]
        v = np.where(n >= 2, (m2 / (n - f32(1))) / n, f32(1e10)).astype(f32)
    return c, v


def shifted(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
    return out


def one_pass(c, v, step, sigma, g=None, sigma_z=0.0, sigma_a=0.0, normal_power_log2=0):
    """One a-trous pass. With a guide image g (H, W, 8) the tap weight takes the
    depth, albedo and normal terms of include/ptmi_guide.h as well."""
    sigma, sigma_z, sigma_a = f32(sigma), f32(sigma_z), f32(sigma_a)
    h, w = v.shape
    with np.errstate(all='ignore'):
        l = lum(c)
        valid = finite(l) & finite(v)
        # 1. prefiltered variance, unit spacing
        vs, gs = np.zeros((h, w), f32), np.zeros((h, w), f32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = shifted(valid, dx, dy, False)
                gk = G[abs(dx)] * G[abs(dy)]
                vq = shifted(v, dx, dy, f32(0))
                vs = np.where(ok, vs + gk * vq, vs)
                gs = np.where(ok, gs + gk, gs)
        vbar = vs / gs
        # 2.
        den = sigma * np.sqrt(vbar) + f32(1e-4)
        if g is not None:
            den_z = sigma_z * g[..., 3] + f32(1e-4)
            den_a = sigma_a + f32(1e-4)
            hit_p = g[..., 7] != 0
        # 3. 5x5 taps at spacing `step`
        C = np.zeros((h, w, 3), f32)
        V, W = np.zeros((h, w), f32), np.zeros((h, w), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = shifted(valid, dx * step, dy * step, False)
                hk = K[abs(dx)] * K[abs(dy)]
                lq = shifted(l, dx * step, dy * step, f32(0))
                cq = shifted(c, dx * step, dy * step, f32(0))
                vq = shifted(v, dx * step, dy * step, f32(0))
                x = np.abs(l - lq) / den
                t = np.fmax(f32(0), f32(1) - x)
                wt = hk * (t * t)
                if g is not None:
                    gq = shifted(g, dx * step, dy * step, f32(0))
                    tz = np.fmax(f32(0), f32(1) - np.abs(g[..., 3] - gq[..., 3]) / den_z)
                    da = (np.abs(g[..., 4] - gq[..., 4]) + np.abs(g[..., 5] - gq[..., 5])) + np.abs(g[..., 6] - gq[..., 6])
                    ta = np.fmax(f32(0), f32(1) - da / den_a)
                    dn = np.fmin(f32(1), np.fmax(f32(0), (g[..., 0] * gq[..., 0] + g[..., 1] * gq[..., 1])
                                                 + g[..., 2] * gq[..., 2]))
                    for _ in range(normal_power_log2):
                        dn = dn * dn
                    hit_q = gq[..., 7] != 0
                    wn = np.where(hit_p & hit_q, dn, np.where(~hit_p & ~hit_q, f32(1), f32(0))).astype(f32)
                    wt = (wt * (tz * tz)) * ((ta * ta) * wn)
                C = np.where(ok[..., None], C + wt[..., None] * cq, C)
                V = np.where(ok, V + (wt * wt) * vq, V)
                W = np.where(ok, W + wt, W)
        # 4.
        c1 = C / W[..., None]
        v1 = V / (W * W)
    return (np.where(valid[..., None], c1, c).astype(f32), np.where(valid, v1, v).astype(f32))


def denoise(accum, stats, iterations=5, sigma=4.0):
    """(rgb (H, W, 3), var (H, W)) of ptmi_denoise."""
    c, v = load(accum, stats)
    for i in range(iterations):
        c, v = one_pass(c, v, 1 << i, sigma)
    return c, v


def tonemap(rgb, spp=1):
    """ptmi_tonemap(rgb, spp) of a finite image: adaptive_helpers' per-pixel tone map with one count."""
    from adaptive_helpers import tonemap as tonemap_stats
    rgb = np.asarray(rgb, f32)
    return tonemap_stats(rgb, np.full(rgb.shape[:2], spp, f32))


def synthetic(width, height, seed=0):
    """accum and stats as after an adaptive render, with every special case of
    the contract that fits the image: n varying per 8x8 tile, n = 0 and n = 1
    pixels, a black region (v = 0, so den = 1e-4f), a hard edge, a firefly, a
    NaN pixel and an M2 = inf pixel. Returns (accum, stats, invalid) with
    invalid the (y, x) of the two invalid pixels."""
    rng = np.random.default_rng(seed)
    ty, tx = np.meshgrid(np.arange(height) // 8, np.arange(width) // 8, indexing='ij')
    n = (16 * (1 + (ty * 3 + tx * 5) % 4)).astype(f32)  # 16 .. 64 per tile
    base = np.empty((height, width, 3), f32)
    base[:] = (0.6, 0.4, 0.2)
    base[:, width // 2:] = (0.05, 0.3, 0.9)  # hard vertical edge
    y0, y1, x0, x1 = height // 2, min(height, height // 2 + 5), 1, min(width, 7)
    base[y0:y1, x0:x1] = 0  # black region
    sd = (f32(0.5) * lum(base) * (1 + rng.random((height, width)).astype(f32))).astype(f32)  # of one sample
    noise = rng.standard_normal((height, width, 3)).astype(f32) * (sd / np.sqrt(n))[..., None]  # of the mean
    mean = np.maximum(base + noise * (base > 0), 0).astype(f32)
    m2 = (sd * sd * (n - 1)).astype(f32)
    accum = (mean * n[..., None]).astype(f32)
    stats = np.zeros((height, width, 4), f32)
    stats[..., 0], stats[..., 1], stats[..., 2] = n, lum(mean), m2

    def at(fy, fx):
        return min(height - 1, int(fy * height)), min(width - 1, int(fx * width))

    p = at(0.2, 0.3)  # n = 0: nothing accumulated
    accum[p], stats[p] = 0, 0
    p = at(0.25, 0.7)  # n = 1: a colour, no variance
    accum[p], stats[p] = mean[p], (1, lum(mean[p]), 0, 0)
    p = at(0.7, 0.25)  # firefly
    accum[p] = accum[p] * f32(1e4)
    stats[p][2] = stats[p][2] * f32(1e8)
    nan_px, inf_px = at(0.4, 0.6), at(0.8, 0.8)
    accum[nan_px] = (np.nan, 1, 1)
    stats[nan_px][1:3] = np.nan
    stats[inf_px][2] = np.inf
    return accum, stats, (nan_px, inf_px)
