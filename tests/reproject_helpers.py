"""numpy f32 reference of the temporal ABI (include/ptmi_temporal.h): the
contract restated step by step, vectorised over the image, one f32 rounding
per operation in the order the header writes them. Plus the cameras, scenes
and synthetic inputs the CPU and GPU tests share."""
import copy

import numpy as np

import denoise_helpers as dh
import guide_helpers as gh

f32 = np.float32
DEFAULTS = dict(max_history=32.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _cam(cam):
    return tuple(np.asarray(cam[k], f32) for k in ('center', 'pixel00', 'delta_u', 'delta_v'))


def reproject(cur, prev, guides_cur, guides_prev, accum, stats, max_history=32.0, sigma_z=0.1, normal_min=0.9,
              sigma_a=0.2, details=False):
    """(accum_out (H, W, 3), stats_out (H, W, 4)) of ptmi_reproject. With
    ``details`` a third value: {'has': pixels with history, 'lo', 'hi': per
    channel the least and the greatest c_q of the counted taps, 'valid': the
    geometric validity, 'ab': the previous-frame position, 'lam'}."""
    g, gp = np.asarray(guides_cur, f32), np.asarray(guides_prev, f32)
    accum, stats = np.asarray(accum, f32), np.asarray(stats, f32)
    H, W = stats.shape[:2]
    max_history, sigma_z, normal_min, sigma_a = f32(max_history), f32(sigma_z), f32(normal_min), f32(sigma_a)
    c, p00, du, dv = _cam(cur)
    pc, pp00, pdu, pdv = _cam(prev)
    with np.errstate(all='ignore'):
        # 1.
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        fpx, fpy = px.astype(f32)[..., None], py.astype(f32)[..., None]
        ps = (p00 + du * fpx) + dv * fpy
        d = (ps - c).astype(f32)
        length = np.sqrt(_dot(d, d)).astype(f32)
        # 2.
        hit_p = g[..., 7] != 0
        s = g[..., 3] / length
        P = c + d * s[..., None]
        v = np.where(hit_p[..., None], P - pc, d).astype(f32)
        # 3.
        r = (pp00 - pc).astype(f32)
        w = _cross(pdu, pdv)
        lam = _dot(r, w) / _dot(v, w)
        q = v * lam[..., None] - r
        a = _dot(q, pdu) / _dot(pdu, pdu)
        b = _dot(q, pdv) / _dot(pdv, pdv)
        zexp = np.sqrt(_dot(v, v)).astype(f32)
        # 4.
        valid = (lam > 0) & (a > -1) & (a < f32(W)) & (b > -1) & (b < f32(H))
        a0, b0 = np.where(valid, a, f32(0)), np.where(valid, b, f32(0))
        fx0, fy0 = np.floor(a0), np.floor(b0)
        fx, fy = a0 - fx0, b0 - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        # 5., 6.
        tol_z = sigma_z * zexp + f32(1e-4)
        Ws, S, N = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
        C = np.zeros((H, W, 3), f32)
        lo, hi = np.full((H, W, 3), np.inf, f32), np.full((H, W, 3), -np.inf, f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                ok = valid & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                wt = (fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)
                st = stats[qyc, qxc]
                n_q = st[..., 0]
                ok &= n_q >= 2
                scale = (1.0 / n_q.astype(np.float64)).astype(f32)
                c_q = accum[qyc, qxc] * scale[..., None]
                s2_q = st[..., 2] / (n_q - f32(1))
                ok &= dh.finite(c_q).all(-1) & dh.finite(s2_q)
                gq = gp[qyc, qxc]
                ok &= (gq[..., 7] != 0) == hit_p
                same = (np.abs(gq[..., 3] - zexp) <= tol_z) & (_dot(g[..., 0:3], gq[..., 0:3]) >= normal_min) & \
                    ((np.abs(g[..., 4] - gq[..., 4]) + np.abs(g[..., 5] - gq[..., 5]))
                     + np.abs(g[..., 6] - gq[..., 6]) <= sigma_a)
                ok &= ~hit_p | same
                Ws = np.where(ok, Ws + wt, Ws)
                C = np.where(ok[..., None], C + wt[..., None] * c_q, C)
                S = np.where(ok, S + wt * s2_q, S)
                N = np.where(ok, N + wt * n_q, N)
                lo = np.where(ok[..., None], np.fmin(lo, c_q), lo)
                hi = np.where(ok[..., None], np.fmax(hi, c_q), hi)
        # 7.
        has = valid & (Ws > 0)
        c1 = C / Ws[..., None]
        s2 = S / Ws
        n1 = np.floor(np.fmin(N / Ws, max_history))
        has &= n1 >= 1
        accum_out = np.where(has[..., None], c1 * n1[..., None], f32(0)).astype(f32)
        stats_out = np.zeros((H, W, 4), f32)
        stats_out[..., 0] = np.where(has, n1, f32(0))
        stats_out[..., 1] = np.where(has, dh.lum(c1), f32(0))
        stats_out[..., 2] = np.where(has, s2 * (n1 - f32(1)), f32(0))
    if details:
        return accum_out, stats_out, {'has': has, 'lo': lo, 'hi': hi, 'valid': valid,
                                      'ab': np.stack([a, b], -1), 'lam': lam}
    return accum_out, stats_out


def countable(accum, stats):
    """Pixels of a history that pass a tap's own tests (count, finite colour and variance)."""
    with np.errstate(all='ignore'):
        n = stats[..., 0]
        ok = n >= 2
        scale = (1.0 / n.astype(np.float64)).astype(f32)
        return ok & dh.finite(accum * scale[..., None]).all(-1) & dh.finite(stats[..., 2] / (n - f32(1)))


def check_properties(accum_out, stats_out, det, max_history):
    """What holds for every output of the contract, asserted on `accum_out`,
    `stats_out` (the device's or the check program's) with the reference's
    details `det`."""
    n = stats_out[..., 0]
    has = n > 0
    assert np.array_equal(has, det['has'])
    assert np.array_equal(n, np.floor(n)) and (n <= f32(max_history)).all() and (n[has] >= 1).all()
    assert (stats_out[..., 2][has] >= 0).all()  # M2' of non-negative M2
    assert not accum_out[~has].any() and not stats_out[~has].any()  # no history: all zeros (+0 or -0)
    assert (stats_out[..., 3] == 0).all()
    # a convex combination of the counted taps: within their range up to the
    # roundings of four products, three sums and two divisions (relative 1e-5)
    with np.errstate(all='ignore'):
        c1 = accum_out[has] / n[has][..., None]
    lo, hi = det['lo'][has], det['hi'][has]
    slack = f32(1e-5) * np.maximum(np.abs(lo), np.abs(hi)) + f32(1e-30)
    fin = np.isfinite(c1) & np.isfinite(lo) & np.isfinite(hi)
    assert (c1[fin] >= (lo - slack)[fin]).all() and (c1[fin] <= (hi + slack)[fin]).all()


# ---------------------------------------------------------------- cameras and scenes
def orbit(cam_obj, dx, dy):
    """The camera-upload dict after the viewer's orbit by the mouse delta
    (dx, dy) (orbit_step / spherical_offset); `cam_obj` itself is left alone."""
    from ptmi import scene_data as sd
    from ptmi.interactive_viewer import orbit_step, spherical_from, spherical_offset
    cam = copy.deepcopy(cam_obj)
    cam.initialize()
    if dx or dy:
        r, theta, phi = spherical_from(cam.lookfrom, cam.lookat)
        theta, phi = orbit_step(theta, phi, dx, dy)
        x, y, z = spherical_offset(r, theta, phi)
        cam.lookfrom = cam.lookat + type(cam.lookfrom - cam.lookat)(x, y, z)
        cam.initialize()
    return sd.camera_upload(cam)


_scenes = {}


def scene(name, width):
    """(SceneArrays, camera object, background) of a guide test scene, `width`
    pixels wide: the arrays and the background are guide_helpers.scene_inputs';
    the camera object, which `orbit` needs and scene_inputs does not keep, is
    the scene's own and uploads to scene_inputs' camera."""
    import random

    from ptmi import scene_data as sd, scenes
    if (name, width) not in _scenes:
        sa, cam, bg = gh.scene_inputs(name, width)
        random.seed(1234)
        if name == 'coverage':
            from coverage_scene import coverage_scene
            cam_obj = coverage_scene(width).cam
        elif name == 'vol2_final_scene':
            cam_obj = scenes.vol2_final_scene(width=width).cam
        else:
            cam_obj = scenes.SCENES[name]().cam
        cam_obj.img_width = width
        cam_obj.initialize()
        up = sd.camera_upload(cam_obj)
        assert all(np.array_equal(up[k], cam[k]) for k in up), (name, width)
        _scenes[name, width] = (sa, cam_obj, tuple(bg))
    return _scenes[name, width]


_oracle_guides = {}


def oracle_guides(name, width, delta):
    """(camera-upload dict, guides) of the scene's camera orbited by `delta`,
    the guides from the numpy guide trace over the CPU oracle; cached."""
    key = (name, width, tuple(delta))
    if key not in _oracle_guides:
        sa, cam_obj, _ = scene(name, width)
        cam = orbit(cam_obj, *delta)
        g = gh.trace_guides(sa, cam)
        g.setflags(write=False)
        _oracle_guides[key] = (cam, g)
    return _oracle_guides[key]


def history(width, height, seed=None):
    """Synthetic accum and stats of a previous frame (denoise_helpers.synthetic:
    n varying per tile, n = 0 and n = 1 pixels, a NaN pixel, an M2 = inf pixel,
    a firefly), plus an infinite accumulator value."""
    accum, stats, _ = dh.synthetic(width, height, seed=width * 1000 + height if seed is None else seed)
    if width * height > 6:
        accum[min(height - 1, height // 2 + 1), width // 3, 1] = np.inf
    return accum, stats


def flat_camera(width, height, shift=(0.0, 0.0, 0.0)):
    """A pinhole camera-upload dict at `shift` looking down -z, one unit from a
    2 x 2 * height / width image plane; delta_u is perpendicular to delta_v."""
    du = np.array([2.0 / width, 0, 0], f32)
    dv = np.array([0, -2.0 / width, 0], f32)
    c = np.array(shift, f32)
    p00 = (c + np.array([-1.0, height / width, -1.0], f32) + f32(0.5) * (du + dv)).astype(f32)
    return {'center': c, 'pixel00': p00, 'delta_u': du, 'delta_v': dv, 'defocus_u': np.zeros(3, f32),
            'defocus_v': np.zeros(3, f32), 'defocus_angle': 0.0, 'width': width, 'height': height}


def flat_guides(cam, depth=3.0):
    """Guides of a wall at z = center.z - depth seen by a flat_camera: unit
    normal +z, depth along each pixel's ray, two albedos, one miss pixel."""
    W, H = cam['width'], cam['height']
    c, p00, du, dv = _cam(cam)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = ((p00 + du * px.astype(f32)[..., None]) + dv * py.astype(f32)[..., None]) - c
    g = np.zeros((H, W, 8), f32)
    g[..., 2] = 1
    g[..., 3] = (np.sqrt(_dot(d, d)) * f32(depth) / np.abs(d[..., 2])).astype(f32)
    g[..., 4:7] = np.where(((px + py) % 2 == 0)[..., None], (0.7, 0.6, 0.5), (0.65, 0.6, 0.55))
    g[..., 7] = 1
    if W * H > 1:
        g[H - 1, W - 1] = (0, 0, 0, gh.MISS_DEPTH, 1, 1, 1, 0)
    return g


def tiny_history(width, height):
    """accum and stats of an image too small for denoise_helpers.synthetic:
    counts 4, 5, ..., with an n = 1 pixel and a NaN pixel where they fit."""
    rng = np.random.default_rng(width * 10 + height)
    n = (4 + np.arange(width * height)).reshape(height, width).astype(f32)
    mean = rng.random((height, width, 3)).astype(f32)
    stats = np.zeros((height, width, 4), f32)
    stats[..., 0], stats[..., 1], stats[..., 2] = n, dh.lum(mean), f32(0.01) * (n - 1)
    accum = (mean * n[..., None]).astype(f32)
    if width * height > 2:
        stats[0, 1] = (1, dh.lum(mean[0, 1]), 0, 0)
        accum[0, 1] = mean[0, 1]
        accum[height - 1, 0] = np.nan
    return accum, stats


# The cases of the CPU check program and of the device alike: (kind, name, width, delta).
# Oracle scenes at 48 px and at 33 px (ragged against 16 x 16 blocks); the camera
# not moved, an orbit step, a large one, and one that faces away (lam <= 0).
DELTAS = ((0, 0), (4, 2), (40, 20), (600, 0))
ORACLE_CASES = [(name, width, delta) for name in ('cornell_box', 'cornell_smoke') for width in (48, 33)
                for delta in DELTAS]
FLAT_CASES = [(1, 1), (3, 2)]


def oracle_case(name, width, delta):
    """(cur, prev, guides_cur, guides_prev, accum, stats) of an oracle case: the
    synthetic history of `history`, and an infinite depth in each guide image."""
    prev, gp = oracle_guides(name, width, (0, 0))
    cur, gc = oracle_guides(name, width, delta)
    H, W = gp.shape[:2]
    accum, stats = history(W, H)
    gc, gp = gc.copy(), gp.copy()
    gc[H // 3, W // 3, 3] = np.inf
    gp[H // 2, W // 2 + 1, 3] = np.inf
    return cur, prev, gc, gp, accum, stats


def flat_case(width, height):
    prev, cur = flat_camera(width, height), flat_camera(width, height, (0.05, 0.02, 0.0))
    accum, stats = tiny_history(width, height)
    return cur, prev, flat_guides(cur), flat_guides(prev), accum, stats


def pack_input(cur, prev, prm, guides_cur, guides_prev, accum, stats):
    """The raw f32 input file of csrc/reproject_check.cpp."""
    head = [np.concatenate(_cam(cur)), np.concatenate(_cam(prev)),
            np.array([prm['max_history'], prm['sigma_z'], prm['normal_min'], prm['sigma_a']], f32)]
    return np.concatenate([np.asarray(x, f32).reshape(-1) for x in head + [guides_cur, guides_prev, accum, stats]])
