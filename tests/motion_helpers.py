"""numpy f32 reference of the motion ABI (include/ptmi_motion.h), and the inputs
the CPU and GPU tests share.

``reproject_moved`` restates step 2' (the place a surface point had on its
primitive before an update) in numpy f32, one rounding per operation in the
header's order, and leaves steps 3 - 7 to ``reproject_helpers.reproject``
itself, called with inputs that make its own step 2 hand over the wanted point
(see ``_carried``). ``trace_ids`` is the id image over the CPU oracle, by the
walk of ``guide_helpers.trace_guides``."""
import numpy as np

import guide_helpers as gh
import reproject_helpers as rh

f32 = np.float32
SPHERE, TRIANGLE, QUAD = 0, 1, 2  # the leaf type codes of include/ptmi.h
ROW_FLOATS = {SPHERE: 4, QUAD: 16, TRIANGLE: 12}
NO_ID = -1


def make_id(ptype, prim):
    return np.int32(int(ptype) << 28 | int(prim))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def rows_of(spheres=None, quads=None, tris=None):
    """{type code: (n, row floats) f32} of row arrays in any shape."""
    given = {SPHERE: spheres, QUAD: quads, TRIANGLE: tris}
    return {t: np.zeros((0, ROW_FLOATS[t]), f32) if a is None else np.array(a, f32).reshape(-1, ROW_FLOATS[t])
            for t, a in given.items()}


def decode(ids, counts):
    """(ok, type, prim) of an id image: ok where the id names a row of its type."""
    ids = np.asarray(ids, np.int32).astype(np.int64)
    ptype, prim = ids >> 28, ids & 0x0fffffff
    count = np.zeros(ids.shape, np.int64)
    for t, n in counts.items():
        count[ptype == t] = n
    return (ids >= 0) & (prim < count), ptype, prim


def surface_points(cur, guides_cur):
    """Step 2's P of every pixel (meaningful on hit pixels), (H, W, 3) f32."""
    g = np.asarray(guides_cur, f32)
    H, W = g.shape[:2]
    c, p00, du, dv = rh._cam(cur)
    with np.errstate(all='ignore'):
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        fpx, fpy = px.astype(f32)[..., None], py.astype(f32)[..., None]
        ps = (p00 + du * fpx) + dv * fpy
        d = (ps - c).astype(f32)
        length = np.sqrt(_dot(d, d)).astype(f32)
        s = g[..., 3] / length
        return (c + d * s[..., None]).astype(f32)


def previous_points(P, ids_cur, rows_cur, rows_prev):
    """Step 2': (P_prev (H, W, 3) f32, ok (H, W)) — ok where the id names a
    row; P_prev is P where the primitive's two rows are bitwise equal."""
    counts = {t: len(r) for t, r in rows_cur.items()}
    ok, ptype, prim = decode(ids_cur, counts)
    out = np.full(P.shape, np.nan, f32)
    with np.errstate(all='ignore'):
        for t in (SPHERE, QUAD, TRIANGLE):
            sel = ok & (ptype == t)
            if not sel.any():
                continue
            new, old, p = rows_cur[t][prim[sel]], rows_prev[t][prim[sel]], P[sel]
            if t == SPHERE:
                k = old[:, 3] / new[:, 3]
                moved = old[:, 0:3] + (p - new[:, 0:3]) * k[:, None]
            elif t == QUAD:  # {n, D, Q, u, v, w}
                h = p - new[:, 4:7]
                w = new[:, 13:16]
                alpha = _dot(w, _cross(h, new[:, 10:13]))
                beta = _dot(w, _cross(new[:, 7:10], h))
                moved = (old[:, 4:7] + old[:, 7:10] * alpha[:, None]) + old[:, 10:13] * beta[:, None]
            else:  # {v0, e1, e2, n}
                e1, e2 = new[:, 3:6], new[:, 6:9]
                h = p - new[:, 0:3]
                m = _cross(e1, e2)
                mm = _dot(m, m)
                alpha = _dot(_cross(h, e2), m) / mm
                beta = _dot(_cross(e1, h), m) / mm
                moved = (old[:, 0:3] + old[:, 3:6] * alpha[:, None]) + old[:, 6:9] * beta[:, None]
            same = (new.view(np.uint32) == old.view(np.uint32)).all(-1)
            out[sel] = np.where(same[:, None], p, moved.astype(f32))
    return out, ok


def _carried(prev, guides_cur, guides_prev, accum, stats, P_prev, details, prm):
    """``reproject_helpers.reproject`` with step 2's surface point of every hit
    pixel replaced by P_prev, bit for bit. Its step 2 forms P = c + d * s with
    s = depth / len and d = pixel00 - c (for delta_u = delta_v = -0). Given
    c = P_prev per pixel, pixel00 = -1e30 and depth = 0: d is about -1e30 per
    component, len overflows to inf, s = +0, d * s = -0, and P = P_prev + -0 is
    P_prev in every bit (a non-finite P_prev gives a NaN P: no history either
    way). The guide depth of the current frame is used nowhere else. Miss
    pixels come out meaningless; the caller does not take them from here."""
    g = np.array(guides_cur, f32)
    g[..., 3] = 0
    neg0 = np.full(3, -0.0, f32)
    cam = {'center': P_prev, 'pixel00': np.full(3, -1e30, f32), 'delta_u': neg0, 'delta_v': neg0}
    return rh.reproject(cam, prev, g, guides_prev, accum, stats, details=details, **prm)


DETAIL_KEYS = ('has', 'lo', 'hi', 'valid', 'ab', 'lam')


def reproject_moved(cur, prev, guides_cur, guides_prev, accum, stats, ids_cur, ids_prev, rows_cur, rows_prev,
                    match_ids=True, details=False, **prm):
    """(accum_out, stats_out[, details]) of ptmi_reproject_moved; rows_cur and
    rows_prev are ``rows_of`` dicts. Miss pixels are ``reproject``'s own. A hit
    pixel takes steps 3 - 7 from ``_carried``; with ``match_ids`` from the call
    whose history holds only the pixels of ids_prev that show its id (a tap
    skipped for its count is a tap skipped for its id: step 6 sees neither)."""
    g = np.asarray(guides_cur, f32)
    ids_cur, ids_prev = np.asarray(ids_cur, np.int32), np.asarray(ids_prev, np.int32)
    stats = np.asarray(stats, f32)
    hit = g[..., 7] != 0
    P_prev, ok = previous_points(surface_points(cur, g), ids_cur, rows_cur, rows_prev)
    out = list(rh.reproject(cur, prev, g, guides_prev, accum, stats, details=True, **prm))  # the miss pixels

    def take(sel, res):
        out[0] = np.where(sel[..., None], res[0], out[0])
        out[1] = np.where(sel[..., None], res[1], out[1])
        for k in DETAIL_KEYS:
            a, b = res[2][k], out[2][k]
            out[2][k] = np.where(sel.reshape(sel.shape + (1,) * (a.ndim - 2)), a, b)

    if not match_ids:
        take(hit, _carried(prev, g, guides_prev, accum, stats, P_prev, True, prm))  # not ok: P_prev is NaN, zeros
    else:
        none = {'has': np.zeros(hit.shape, bool), 'lo': np.full(hit.shape + (3,), np.inf, f32),
                'hi': np.full(hit.shape + (3,), -np.inf, f32), 'valid': np.zeros(hit.shape, bool),
                'ab': np.full(hit.shape + (2,), np.nan, f32), 'lam': np.full(hit.shape, np.nan, f32)}
        take(hit & ~ok, (np.zeros_like(out[0]), np.zeros_like(out[1]), none))
        for k in np.unique(ids_cur[hit & ok]):
            st = stats.copy()
            st[ids_prev != k, 0] = 0  # those taps do not count
            take(hit & ok & (ids_cur == k), _carried(prev, g, guides_prev, accum, st, P_prev, True, prm))
    return tuple(out) if details else (out[0], out[1])


# ---------------------------------------------------------------- the id image
_device_index = {}


def device_index(sa):
    """Per type code, the device primitive index of every reference primitive
    (the inverse of the packed layout's prim_perm)."""
    from ptmi import scene_data as sd
    if id(sa) not in _device_index:
        perm = sd.pack_device(sa).prim_perm
        inv = []
        for p in perm:
            a = np.empty(len(p), np.int64)
            a[np.asarray(p, np.int64)] = np.arange(len(p))
            inv.append(a)
        _device_index[id(sa)] = (sa, inv)
    return _device_index[id(sa)][1]


def trace_ids(sa, cam, traversal='stack'):
    """(H, W) int32: what ptmi_guide_trace_ids writes into ids for the scene
    arrays ``sa`` and the camera-upload dict ``cam``: guide_helpers.trace_guides'
    walk over the CPU oracle, keeping the primitive of the surface hit."""
    import oracle
    osc = oracle.OracleScene(sa)
    dev = device_index(sa)
    W, H = int(cam['width']), int(cam['height'])
    c, p00, du, dv = (np.asarray(cam[k], f32) for k in ('center', 'pixel00', 'delta_u', 'delta_v'))
    ids = np.full((H, W), NO_ID, np.int32)
    for y in range(H):
        for x in range(W):
            o = c
            dd = (((p00 + du * f32(x)) + dv * f32(y)) - c).astype(f32)
            for _ in range(gh.TRAVERSALS):
                hit, t, ty, ix = oracle.traverse(osc, o, dd, 0.001, 1e10, traversal)
                if not hit:
                    break
                if int(sa.mats(ty)['is_constant_medium'][ix]) > 0:
                    o = (o + dd * f32(t)).astype(f32)
                    continue
                ids[y, x] = make_id(ty, dev[ty][ix])
                break
    return ids


def device_rows(sa):
    """``rows_of`` dict of the scene's primitive rows in device order."""
    from ptmi import scene_data as sd
    lay = sd.pack_device(sa)
    return rows_of(lay.spheres, lay.quads, lay.tris)


# ---------------------------------------------------------------- cases
W, H = 48, 27  # the frame of every test; the id trace also gets RAGGED
RAGGED = (37, 21)  # partial 8 x 8 squares on both edges


def camera(name, width=W, height=H, delta=(0, 0)):
    """Camera-upload dict of a test scene's camera (reproject_helpers.scene) on
    a width x height frame, orbited by the mouse delta ``delta``."""
    import copy
    cam = copy.deepcopy(rh.scene(name, 48)[1])
    cam.img_width, cam.aspect_ratio = width, width / (height + 0.5)
    up = rh.orbit(cam, *delta)
    assert (up['width'], up['height']) == (width, height)
    return up


ONE_DEGREE = (1.0 / 0.3, 0)  # orbit_step turns 0.3 degrees per pixel of mouse travel


def coverage_edits(sa):
    """One update of `coverage` that moves a sphere (the earth sphere, shrunk a
    little), a quad (the one most pixels of the base camera see, translated and
    sheared) and a triangle together, as the arguments of
    DeviceScene.update_primitives / update_helpers.refit."""
    import update_helpers as uh
    from ptmi import scene_data as sd
    s = sa.sphere_data[1]
    q, t = sa.quads, sa.tris
    ids = traced('coverage', sa, 'base', camera('coverage'))[1]
    seen = ids[(ids >> 28) == QUAD] & 0x0fffffff
    qi = int(sd.pack_device(sa).prim_perm[QUAD][np.bincount(seen).argmax()])  # its reference index
    Q, u, v = (tuple(float(x) for x in q[k][qi]) for k in ('quad_Q', 'quad_u', 'quad_v'))
    tri = [tuple(float(x) + d for x, d in zip(t[k][0], (0.1, 0.2, 0.0)))
           for k in ('triangle_v0', 'triangle_v1', 'triangle_v2')]
    return {'spheres': uh.sphere_edit([1], [s[0:3] + np.array([0.3, 0.1, 0.2], f32)], [s[3] * f32(0.9)]),
            'quads': uh.quad_edit([qi], [((Q[0] + 0.2, Q[1] + 0.1, Q[2]), (u[0], u[1] + 0.2, u[2]), v)]),
            'triangles': uh.tri_edit([0], [tuple(tri)])}


_traced = {}


def traced(name, sa, key, cam, traversal='stack'):
    """(guides, ids) of the oracle trace of ``sa`` (named ``name`` / ``key`` for the cache), read-only."""
    k = (name, key, cam['width'], cam['height'], tuple(cam['center'].tolist()), tuple(cam['pixel00'].tolist()),
         traversal)
    if k not in _traced:
        g, i = gh.trace_guides(sa, cam, traversal), trace_ids(sa, cam, traversal)
        assert np.array_equal(i >= 0, g[..., 7] != 0)  # an id exactly where the guide pixel is a surface hit
        g.setflags(write=False)
        i.setflags(write=False)
        _traced[k] = (g, i)
    return _traced[k]


_cases = {}


def coverage_case(moved=True):
    """The inputs of ptmi_reproject_moved on `coverage`, 48 x 27: the camera
    orbited one degree; with ``moved`` the scene updated by ``coverage_edits``
    in between, else left alone. A dict: cur, prev (cameras), guides_cur,
    guides_prev, ids_cur, ids_prev, accum, stats, rows_cur, rows_prev, sa_prev,
    sa_cur, edits."""
    import update_helpers as uh
    if moved not in _cases:
        sa = rh.scene('coverage', 48)[0]
        edits = coverage_edits(sa) if moved else {}
        sa1 = uh.refit(sa, edits) if moved else sa
        prev, cur = camera('coverage'), camera('coverage', delta=ONE_DEGREE)
        gp, ip = traced('coverage', sa, 'base', prev)
        gc, ic = traced('coverage', sa1, 'moved' if moved else 'base', cur)
        accum, stats = rh.history(W, H)
        _cases[moved] = dict(cur=cur, prev=prev, guides_cur=gc, guides_prev=gp, ids_cur=ic, ids_prev=ip, accum=accum,
                             stats=stats, rows_cur=device_rows(sa1), rows_prev=device_rows(sa), sa_prev=sa,
                             sa_cur=sa1, edits=edits)
    return _cases[moved]


def reference(case, match_ids=True, details=False, **prm):
    prm = dict(rh.DEFAULTS, **prm)
    return reproject_moved(case['cur'], case['prev'], case['guides_cur'], case['guides_prev'], case['accum'],
                           case['stats'], case['ids_cur'], case['ids_prev'], case['rows_cur'], case['rows_prev'],
                           match_ids=match_ids, details=details, **prm)


SYNTHETIC_KINDS = ('spheres', 'quads', 'tris', 'nan_row', 'ulp')


def synthetic_case(kind, seed=0):
    """A 48 x 27 frame of a wall at z = -3 seen by two flat cameras
    (reproject_helpers.flat_camera), its pixels assigned in blocks to six
    primitives of one type (and to no id), with random current rows near the
    wall and previous rows a little off:
      'spheres'  centres moved, radii changed;
      'quads'    translated and sheared (rows by the scene compiler's arithmetic);
      'tris'     translated, one vertex moved;
      'nan_row'  spheres whose previous rows are all NaN;
      'ulp'      spheres with r_new == r_old and the centre's x moved by one ulp.
    The previous id image is the current one shifted by a pixel, so taps near a
    block's edge show another id."""
    import update_helpers as uh
    rng = np.random.default_rng(1000 + seed)
    prev, cur = rh.flat_camera(W, H), rh.flat_camera(W, H, (0.05, 0.02, 0.0))
    accum, stats = rh.history(W, H)
    n = 6
    small = lambda k, s=0.05: tuple(float(x) for x in rng.uniform(-s, s, k))  # noqa: E731
    if kind in ('spheres', 'nan_row', 'ulp'):
        ptype = SPHERE
        new = np.concatenate([rng.uniform(-1, 1, (n, 1)), rng.uniform(-0.5, 0.5, (n, 1)), np.full((n, 1), -3.4),
                              rng.uniform(0.4, 0.6, (n, 1))], 1).astype(f32)
        old = new.copy()
        if kind == 'spheres':
            old[:, 0:3] += rng.uniform(-0.05, 0.05, (n, 3)).astype(f32)
            old[:, 3] *= rng.uniform(0.95, 1.05, n).astype(f32)
        elif kind == 'ulp':
            old[:, 0] = np.nextafter(old[:, 0], f32(np.inf))
        else:
            old[:] = np.nan
        rows_cur, rows_prev = rows_of(spheres=new), rows_of(spheres=old)
    elif kind == 'quads':
        ptype = QUAD
        quads = [((-2 + a, -1.2 + b, -3.0), (4.0 + c, d, 0.0), (e, 2.4 + f, 0.0))
                 for a, b, c, d, e, f in (small(6, 0.1) for _ in range(n))]
        moved = [(tuple(x + s for x, s in zip(Q, small(3))), tuple(x + s for x, s in zip(u, small(3, 0.2))),
                  tuple(x + s for x, s in zip(v, small(3, 0.2)))) for Q, u, v in quads]
        rows_cur, rows_prev = rows_of(quads=uh.quad_edit(range(n), quads)[1]), \
            rows_of(quads=uh.quad_edit(range(n), moved)[1])
    else:
        ptype = TRIANGLE
        tris = [((-2.2 + a, -1.3 + b, -3.0), (2.6 + c, -1.3 + d, -3.0), (-2.2 + e, 1.6 + f, -3.0))
                for a, b, c, d, e, f in (small(6, 0.1) for _ in range(n))]
        shift = [small(3) for _ in range(n)]
        moved = [(tuple(x + s for x, s in zip(a, sh)), tuple(x + s for x, s in zip(b, sh)),
                  tuple(x + s + t for x, s, t in zip(c, sh, small(3)))) for (a, b, c), sh in zip(tris, shift)]
        rows_cur, rows_prev = rows_of(tris=uh.tri_edit(range(n), tris)[1]), \
            rows_of(tris=uh.tri_edit(range(n), moved)[1])
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    block = (py // 7) * 6 + px // 8
    which = block % (n + 1)
    ids = np.where(which == n, NO_ID, ptype << 28 | which).astype(np.int32)
    gc, gp = rh.flat_guides(cur), rh.flat_guides(prev)
    ids[gc[..., 7] == 0] = NO_ID
    ids_prev = np.roll(ids, 1, axis=1)
    return dict(cur=cur, prev=prev, guides_cur=gc, guides_prev=gp, ids_cur=ids, ids_prev=ids_prev, accum=accum,
                stats=stats, rows_cur=rows_cur, rows_prev=rows_prev)


# The property that shows the feature: an opaque sphere that slides across a
# fixed view takes its history along.
COLOUR_A, COLOUR_B = np.array([0.8, 0.2, 0.1], f32), np.array([0.1, 0.3, 0.9], f32)
SLIDE_FROM, SLIDE_TO, SLIDE_RADIUS = (-1.0, 0.3, -1.0), (1.0, 0.3, -1.0), 0.8  # 2.0 along the image's x, diameter 1.6


def slide_world(centre):
    from ptmi import core
    w = core.hittable_list()
    grey = core.lambertian(core.solid_color(core.vec3(.5, .5, .5)))
    w.add(core.Sphere.stationary(core.vec3(0, -100.5, -1), 100, grey))
    w.add(core.Sphere.stationary(core.vec3(*centre), SLIDE_RADIUS,
                                 core.lambertian(core.solid_color(core.vec3(.7, .3, .3)))))
    w.add(core.quad(core.vec3(-4, -0.5, -3), core.vec3(8, 0, 0), core.vec3(0, 4, 0), grey))
    w.add(core.triangle(core.vec3(-2.5, -0.5, 0.5), core.vec3(-1.5, -0.5, 0.5), core.vec3(-2, 0.5, 0.5), grey))
    return w


def slide_camera_object():
    from ptmi import core
    cam = core.camera()
    cam.aspect_ratio, cam.img_width, cam.samples_per_pixel, cam.vfov = W / (H + 0.5), W, 4, 50
    cam.lookfrom, cam.lookat, cam.vup = core.vec3(0, 0.5, 3), core.vec3(0, 0, -1), core.vec3(0, 1, 0)
    cam.defocus_angle = 0.0
    return cam


def slide_history(ids_prev, sphere_id):
    """n = 8 everywhere, colour A on the sphere's old pixels and B elsewhere, a finite M2."""
    import denoise_helpers as dh
    colour = np.where((ids_prev == sphere_id)[..., None], COLOUR_A, COLOUR_B).astype(f32)
    stats = np.zeros(ids_prev.shape + (4,), f32)
    stats[..., 0], stats[..., 1], stats[..., 2] = 8, dh.lum(colour), f32(0.07)
    return (colour * f32(8)).astype(f32), stats


def slide_case():
    """coverage_case's dict for the sliding sphere, camera fixed, plus
    'sphere_id'; guides and ids from the oracle trace."""
    import random

    import update_helpers as uh
    from ptmi import scene_data as sd
    if 'slide' not in _cases:
        random.seed(1234)
        sa = sd.compile_world(slide_world(SLIDE_FROM))
        cam_obj = slide_camera_object()
        cam_obj.initialize()
        cam = sd.camera_upload(cam_obj)
        assert (cam['width'], cam['height']) == (W, H)
        edits = {'spheres': uh.sphere_edit([1], [SLIDE_TO], [SLIDE_RADIUS])}
        sa1 = uh.refit(sa, edits)
        gp, ip = traced('slide', sa, 'base', cam)
        gc, ic = traced('slide', sa1, 'moved', cam)
        sphere_id = make_id(SPHERE, device_index(sa)[SPHERE][1])
        accum, stats = slide_history(ip, sphere_id)
        _cases['slide'] = dict(cur=cam, prev=cam, guides_cur=gc, guides_prev=gp, ids_cur=ic, ids_prev=ip, accum=accum,
                               stats=stats, rows_cur=device_rows(sa1), rows_prev=device_rows(sa), sa_prev=sa,
                               sa_cur=sa1, edits=edits, sphere_id=sphere_id)
    return _cases['slide']


# What the reference gives for slide_case (asserted by the CPU test before anything relies on them).
SLIDE_SPHERE_PIXELS = 113
SLIDE_INTERIOR_PIXELS = 75


def check_slide(case, accum_out, stats_out, plain_accum, plain_stats, det):
    """The assertions of the sliding sphere on an output of ptmi_reproject_moved
    (match_ids on) and one of ptmi_reproject, both for ``case``; ``det`` the
    reference's details. Returns (sphere pixels, interior pixels)."""
    sid = case['sphere_id']
    on_sphere = case['ids_cur'] == sid
    ab = det['ab']
    with np.errstate(all='ignore'):
        x0, y0 = np.floor(ab[..., 0]), np.floor(ab[..., 1])
    interior = on_sphere & det['valid']
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = interior & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            tap = case['ids_prev'][np.where(inside, qy, 0).astype(np.int64), np.where(inside, qx, 0).astype(np.int64)]
            interior = inside & (tap == sid)
    has = stats_out[..., 0] > 0
    assert has[interior].all()  # four taps on the old sphere: history
    with np.errstate(all='ignore'):
        c1 = accum_out / stats_out[..., 0:1]
        c0 = plain_accum / plain_stats[..., 0:1]
    kept = on_sphere & has
    assert kept.any() and (np.abs(c1[kept] - COLOUR_A) <= f32(1e-6) * COLOUR_A).all()  # means of equal values
    # the static reprojection looks where the sphere is now, and was not: never colour A
    plain = on_sphere & (plain_stats[..., 0] > 0)
    assert not (np.abs(c0[plain] - COLOUR_A) <= f32(1e-3)).all(-1).any()
    return int(on_sphere.sum()), int(interior.sum())


# ---------------------------------------------------------------- the check program's files
def pack_input(cur, prev, prm, guides_cur, guides_prev, accum, stats, rows_cur, rows_prev):
    """The raw f32 input file of csrc/motion_check.cpp."""
    rows = [r[t].reshape(-1) for r in (rows_cur, rows_prev) for t in (SPHERE, QUAD, TRIANGLE)]
    return np.concatenate([rh.pack_input(cur, prev, prm, guides_cur, guides_prev, accum, stats)] + rows).astype(f32)


def pack_ids(ids_cur, ids_prev):
    return np.concatenate([np.asarray(ids_cur, np.int32).reshape(-1), np.asarray(ids_prev, np.int32).reshape(-1)])
