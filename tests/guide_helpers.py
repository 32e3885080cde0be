"""numpy f32 reference of the guide ABI (include/ptmi_guide.h).

The guide trace is restated over the CPU oracle: one ``oracle.traverse`` per
traversal with the moved origin, the hit normal and the solid and checker
textures in numpy f32, the image texture through ``func_probe('sphere_uv')``
plus the index arithmetic, Perlin through ``func_probe('perlin_turb')`` and
``math_probe('sin')``. Materials are looked up in the reference-layout arrays
(``sa.mats(type)``) by the oracle's primitive index, so the device's leaf-order
permutation is no part of the contract.

The guided filter is ``denoise_helpers.one_pass`` with a guide image (the depth,
albedo and normal terms) and the demodulation around it; ``synthetic_guides`` is
a guide image for ``denoise_helpers.synthetic``."""
import numpy as np

import denoise_helpers as dh

f32 = np.float32
MISS_DEPTH = f32(1e10)
TRAVERSALS = 4


# ---------------------------------------------------------------- the guide trace
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _f2i(x):
    """pt_f2i: truncation, saturating, NaN -> 0."""
    x = np.asarray(x, f32)
    with np.errstate(invalid='ignore'):
        y = np.where(np.isnan(x), 0.0, np.clip(x.astype(np.float64), -2147483648.0, 2147483647.0))
    return np.trunc(y).astype(np.int64)


def _albedo(osc, sa, ty, ix, hp):
    """Guide albedo of surface hits: ty, ix (n,) the oracle's primitive type and index, hp (n, 3)."""
    import oracle
    n = len(ty)
    out = np.ones((n, 3), f32)
    for pt in range(3):
        m = sa.mats(pt)
        sel = np.nonzero(ty == pt)[0]
        if not len(sel):
            continue
        pi = ix[sel]
        mt = np.asarray(m['material_type'])[pi]
        metal = sel[mt == 1]
        out[metal] = np.asarray(m['material_albedo'], f32)[ix[metal]]
        tex_sel = sel[(mt == 0) | (mt == 4)]
        pi = ix[tex_sel]
        tt = np.asarray(m['texture_type'])[pi]
        c1 = np.asarray(m['texture_color1'], f32)[pi]
        c2 = np.asarray(m['texture_color2'], f32)[pi]
        scale = np.asarray(m['texture_scale'], f32)[pi]
        h = hp[tex_sel]
        res = np.ones((len(tex_sel), 3), f32)
        res[tt == 0] = c1[tt == 0]
        k = tt == 1  # checker
        if k.any():
            inv = f32(1) / scale[k]
            s = _f2i(np.floor(inv * h[k, 0])) + _f2i(np.floor(inv * h[k, 1])) + _f2i(np.floor(inv * h[k, 2]))
            res[k] = np.where((s % 2 == 0)[:, None], c1[k], c2[k])
        k = tt == 2  # image: spheres only, magenta elsewhere
        if k.any():
            if pt != 0:
                res[k] = (1.0, 0.0, 1.0)
            else:
                img = np.asarray(m['texture_image_idx'])[pi[k]]
                centre = np.asarray(sa.sphere_data, f32)[pi[k], 0:3]
                uv = oracle.func_probe(osc, 'sphere_uv', np.concatenate([h[k], centre], axis=1))
                rk = np.ones((int(k.sum()), 3), f32)
                for j in range(len(img)):
                    if 0 <= img[j] < len(sa.images):
                        im = sa.images[img[j]]
                        H, W = im.shape[0], im.shape[1]
                        u = np.fmax(f32(0), np.fmin(f32(1), uv[j, 0]))
                        v = f32(1) - np.fmax(f32(0), np.fmin(f32(1), uv[j, 1]))
                        ii = int(np.clip(_f2i(u * f32(W)), 0, W - 1))
                        jj = int(np.clip(_f2i(v * f32(H)), 0, H - 1))
                        rk[j] = im[jj, ii, 0:3].astype(f32) / f32(255)
                res[k] = rk
        k = tt == 3  # noise
        if k.any():
            rec = np.concatenate([h[k], np.full((int(k.sum()), 1), 3, f32)], axis=1)
            turb = oracle.func_probe(osc, 'perlin_turb', rec)[:, 0]
            nv = oracle.math_probe('sin', scale[k] * h[k, 2] + f32(10) * turb)
            res[k] = (c1[k] * f32(0.5)) * (f32(1) + nv)[:, None]
        out[tex_sel] = res
    return out


def trace_guides(sa, cam, traversal='stack'):
    """(H, W, 8) f32: what ptmi_guide_trace writes for the scene arrays `sa`
    and the camera upload dict `cam`."""
    import oracle
    osc = oracle.OracleScene(sa)
    W, H = int(cam['width']), int(cam['height'])
    c, p00, du, dv = (np.asarray(cam[k], f32) for k in ('center', 'pixel00', 'delta_u', 'delta_v'))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ps = (p00 + du * px.astype(f32)[..., None]) + dv * py.astype(f32)[..., None]
    d = (ps - c).astype(f32)
    length = np.sqrt(_dot(d, d)).astype(f32)
    g = np.zeros((H, W, 8), f32)
    g[..., 3], g[..., 4:7] = MISS_DEPTH, 1
    surf = []
    for y in range(H):
        for x in range(W):
            o, dd, z = c, d[y, x], f32(0)
            for _ in range(TRAVERSALS):
                hit, t, ty, ix = oracle.traverse(osc, o, dd, 0.001, 1e10, traversal)
                if not hit:
                    break
                hp = (o + dd * f32(t)).astype(f32)
                z = z + f32(t) * length[y, x]
                if int(sa.mats(ty)['is_constant_medium'][ix]) > 0:
                    o = hp
                    continue
                surf.append((y, x, ty, ix, hp, z))
                break
    if surf:
        ys, xs, ty, ix = (np.array([s[k] for s in surf], np.int64) for k in range(4))
        hp = np.array([s[4] for s in surf], f32)
        dd = d[ys, xs]
        n = np.zeros((len(surf), 3), f32)
        k = ty == 0  # sphere: (hp - centre) / radius
        sd = np.asarray(sa.sphere_data, f32)[ix[k]]
        n[k] = (hp[k] - sd[:, 0:3]) / sd[:, 3:4]
        k = ty == 2  # quad: the stored normal, against d
        qn = np.asarray(sa.quads['quad_normal'], f32)[ix[k]]
        n[k] = np.where((_dot(qn, dd[k]) < 0)[:, None], qn, -qn)
        k = ty == 1  # triangle
        tn = np.asarray(sa.tris['triangle_normal'], f32)[ix[k]]
        n[k] = np.where((_dot(dd[k], tn) > 0)[:, None], -tn, tn)
        g[ys, xs, 0:3] = n
        g[ys, xs, 3] = np.array([s[5] for s in surf], f32)
        g[ys, xs, 4:7] = _albedo(osc, sa, ty, ix, hp)
        g[ys, xs, 7] = 1
    return g


# ---------------------------------------------------------------- the guided filter
def modulation(guides):
    """(m (H, W, 3), lm * lm (H, W)) of the demodulation."""
    m = np.fmax(np.asarray(guides, f32)[..., 4:7], f32(0)) + f32(1e-3)
    lm = dh.lum(m)
    return m, lm * lm


def denoise_guided(accum, stats, guides, iterations=5, sigma=4.0, sigma_z=0.1, sigma_a=0.2, normal_power_log2=5,
                   demodulate=True):
    """(rgb (H, W, 3), var (H, W)) of ptmi_denoise_guided."""
    g = np.asarray(guides, f32)
    c, v = dh.load(accum, stats)
    with np.errstate(all='ignore'):
        if demodulate:
            m, lm2 = modulation(g)
            c, v = c / m, v / lm2
        for i in range(iterations):
            c, v = dh.one_pass(c, v, 1 << i, sigma, g, sigma_z, sigma_a, normal_power_log2)
        if demodulate:
            c, v = c * m, v * lm2
    return c.astype(f32), v.astype(f32)


def synthetic_guides(width, height, seed=0):
    """A guide image for denoise_helpers.synthetic(width, height): a depth ramp
    with a step, two normal regions (one curved, one flat), an albedo checker
    with a little noise, a black and a negative albedo (the demodulation's
    floor), and a block of miss pixels that includes the image corner."""
    rng = np.random.default_rng(seed + 77)
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
    g = np.zeros((height, width, 8), f32)
    n = np.stack([0.02 * (x - width / 2), 0.02 * (y - height / 2), np.ones_like(x, float)], -1)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    n[y >= height // 2] = (0.6, 0.0, 0.8)
    g[..., 0:3] = n
    g[..., 3] = 1.0 + 0.05 * x + 0.02 * y + 3.0 * (x >= (2 * width) // 3)
    a = np.where((((x // 4) + (y // 4)) % 2 == 0)[..., None], (0.8, 0.6, 0.3), (0.2, 0.3, 0.7))
    g[..., 4:7] = a + 0.05 * rng.random((height, width, 3))
    g[..., 7] = 1
    g[height - 1 - height // 5:, width // 2:width // 2 + 3, 4:7] = 0  # black albedo
    g[height // 3, width - 1, 4] = -0.5  # floored at 0 by the demodulation
    my, mx = max(1, height // 4), max(1, width // 4)
    g[:my, :mx] = (0, 0, 0, MISS_DEPTH, 1, 1, 1, 0)  # misses, the corner included
    return g


# ---------------------------------------------------------------- scenes
_scenes = {}


def scene_inputs(name, width):
    """(SceneArrays, camera upload dict, background) of a guide test scene: the
    parity scenes of parity_helpers where they have a camera of that width,
    else the scene compiled here as the renderer compiles it."""
    import random

    import parity_helpers as ph
    from ptmi import scene_data as sd, scenes
    if name in ph.BUILT or (name, width) == ('vol2_final_scene', 64):
        return ph.scene_inputs(name, width)
    if (name, width) not in _scenes:
        random.seed(1234)
        sc = scenes.SCENES[name]()
        sc.cam.img_width = width
        sc.cam.initialize()
        _scenes[name, width] = (sd.compile_world(sc.world), sd.camera_upload(sc.cam), tuple(sc.background))
    return _scenes[name, width]
