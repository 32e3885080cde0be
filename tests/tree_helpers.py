"""numpy f32 reference of the tree-quality ABI (include/ptmi_tree.h), in the
kernels' own order, and the small trees its tests share.

``areas(ref_nodes)`` and ``growth(ref_nodes, base)`` are ptmi_tree_areas and
ptmi_tree_growth on (n, 12) f32 ``ref_nodes`` rows (DeviceLayout.ref_nodes):
growth keeps one f64 sum, one f32 maximum and one count per lane of the 1024,
fed in ascending row order, then folds them for s = 512 .. 1, so every bit is
the kernel's. ``remap(ids, maps)`` is ptmi_ids_remap. ``rebuilt(sa)`` is the
host half of DeviceScene.rebuild: the native builder on the arrays' builder-form
records."""
import dataclasses

import numpy as np

from ptmi import bvh, scene_data as sd

f32 = np.float32
LANES = 1024
# (fraction, seed) of a ``scatter`` of vol2 after which the rebuilt tree's max_leaf_depth is 16 against the refit
# tree's 15: the nearest sweep point and the first seed that have such a change (+-50 % has none for seeds 1 .. 8)
DEPTH_CASE = (0.25, 3)


def areas(ref_nodes):
    rn = np.asarray(ref_nodes, f32).reshape(-1, 12)
    d = rn[:, 4:7] - rn[:, 0:3]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return (f32(2.0) * ((dx * dy + dy * dz) + dz * dx)).astype(f32)


def is_inner(ref_nodes):
    rn = np.ascontiguousarray(np.asarray(ref_nodes, f32).reshape(-1, 12))
    return rn.view(np.int32)[:, 3] >= 0


def terms(ref_nodes, base):
    """r(i) of every row (the leaves' too: growth skips them)."""
    a, base = areas(ref_nodes), np.asarray(base, f32).reshape(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(base > 0, a / np.where(base > 0, base, f32(1.0)), f32(1.0)).astype(f32)


def growth(ref_nodes, base):
    """out[4] of ptmi_tree_growth as an f32 array: {mean, max, n, 0}."""
    inner = is_inner(ref_nodes)
    n = inner.shape[0]
    r = terms(ref_nodes, base) if n else np.zeros(0, f32)
    rows = (n + LANES - 1) // LANES
    pad = rows * LANES - n
    # a skipped row adds +0.0 (s + 0.0 == s bit for bit, sums being >= 0), leaves the maximum (>= 1) and counts 0
    rs = np.concatenate([np.where(inner, r, f32(0.0)), np.zeros(pad, f32)]).reshape(rows, LANES).astype(np.float64)
    rm = np.concatenate([np.where(inner, r, f32(1.0)), np.ones(pad, f32)]).reshape(rows, LANES)
    rc = np.concatenate([inner, np.zeros(pad, bool)]).reshape(rows, LANES).astype(np.int64)
    s, m, c = np.zeros(LANES, np.float64), np.ones(LANES, f32), np.zeros(LANES, np.int64)
    for j in range(rows):  # lane k's walk: rows k, k + 1024, ... in ascending order
        s = s + rs[j]
        m = np.where(m > rm[j], m, rm[j])
        c = c + rc[j]
    w = LANES // 2
    while w >= 1:
        s[:w] = s[:w] + s[w:2 * w]
        m[:w] = np.where(m[:w] > m[w:2 * w], m[:w], m[w:2 * w])
        c[:w] = c[:w] + c[w:2 * w]
        w //= 2
    mean = f32(s[0] / np.float64(c[0])) if c[0] else f32(1.0)
    return np.array([mean, m[0], f32(c[0]), 0.0], f32)


def remap(ids, maps):
    """ptmi_ids_remap: ``maps`` by type code (spheres, triangles, quads), int32 arrays; the counts are their lengths."""
    ids = np.asarray(ids, np.int32)
    out = np.full(ids.shape, -1, np.int32)
    t, p = ids >> 28, ids & 0x0fffffff
    for code, m in enumerate(maps):
        m = np.asarray(m, np.int32)
        sel = (ids >= 0) & (t == code) & (p < len(m))
        new = m[p[sel]] if len(m) else np.zeros(0, np.int32)
        ok = (new >= 0) & (new < len(m))
        out[sel] = np.where(ok, (code << 28) | new, -1)
    return out


def hostile_ids(counts, rng, n=4096):
    """An id image's worth of ids around every rejection of ptmi_ids_remap, for maps of these counts."""
    counts = [int(c) for c in counts]
    ids = [-1, -2, -(1 << 31), (1 << 31) - 1]
    for t in range(8):  # types 3 .. 7 are unknown
        c = counts[t] if t < 3 else 5
        for p in (0, 1, c - 1, c, c + 1, (1 << 28) - 1):
            if 0 <= p < (1 << 28):
                ids.append(t << 28 | p)
    ids = np.array(ids, np.int64)
    fill = rng.integers(0, 3, n) << 28 | rng.integers(0, max(counts) + 2, n)
    return np.concatenate([ids, fill]).astype(np.int64).astype(np.uint32).view(np.int32)


def builder_records(sa):
    """(spheres, quads, tris) of a SceneArrays in the builder's form: {c, r}; {Q, u, v}; {v0, v1, v2}."""
    q, t = sa.quads, sa.tris
    return (sa.sphere_data, np.concatenate([q['quad_Q'], q['quad_u'], q['quad_v']], axis=1),
            np.concatenate([t['triangle_v0'], t['triangle_v1'], t['triangle_v2']], axis=1))


def rebuilt(sa):
    """``sa`` with the BVH the native builder makes of its geometry arrays."""
    b = bvh.build_sah(*builder_records(sa))
    return dataclasses.replace(sa, bvh={k: b[k] for k in sd.BVH_KEYS})


def sphere_arrays(spheres):
    """A SceneArrays of Lambertian spheres ((n, 4) {c, r}) with the builder's tree: the synthetic trees."""
    sph = np.ascontiguousarray(spheres, f32).reshape(-1, 4)
    n = sph.shape[0]
    mats = sd._empty_mats(n)
    mats['material_albedo'][:] = 0.5
    none = {k: np.zeros((0,) if k == 'quad_D' else (0, 3), f32) for k in sd.QUAD_KEYS}
    tris = {k: np.zeros((0, 3), f32) for k in sd.TRI_KEYS}
    perlin = {'perlin_randvec': np.zeros((256, 3), f32)}
    perlin.update({k: np.arange(256, dtype=np.int32) for k in sd.PERLIN_KEYS[1:]})
    b = bvh.build_sah(sph)
    return sd.SceneArrays(sph, mats, none, sd._empty_mats(0), tris, sd._empty_mats(0),
                          {k: b[k] for k in sd.BVH_KEYS}, perlin, [])


def synthetic(n_inner, seed=3, zero_radius=False):
    """sphere_arrays of n_inner + 1 random spheres (so n_inner internal nodes), radius 0 on request."""
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-50, 50, (n_inner + 1, 3)), rng.uniform(0.5, 3.0, (n_inner + 1, 1))], axis=1)
    if zero_radius:
        sph[:, 3] = 0.0
    return sphere_arrays(sph.astype(f32))


def scatter(sa, frac, seed=1, side=165.0, radius=10.0):
    """update_helpers' sphere edit that displaces the spheres of this radius (vol2's
    1000 box spheres) per component by up to +-frac * side."""
    import update_helpers as uh
    rng = np.random.default_rng(seed)
    idx = np.nonzero(sa.sphere_data[:, 3] == f32(radius))[0]
    if idx.size == 0:
        idx = np.arange(sa.num_spheres)
    d = rng.uniform(-frac * side, frac * side, (idx.size, 3)).astype(f32)
    return uh.sphere_edit(idx, sa.sphere_data[idx, 0:3] + d, sa.sphere_data[idx, 3])


def mixed_edit(sa, seed=2):
    """update_helpers edits of every primitive type a scene has: its spheres
    scattered (``scatter``, +-25 %), every other quad and every third triangle
    translated by up to three median leaf extents per component, so that a
    rebuild reorders the leaves of each type."""
    import update_helpers as uh
    rng = np.random.default_rng(seed)
    b = sa.bvh
    leaves = b['bvh_prim_idx'] >= 0
    step = 3.0 * float(np.median((b['bvh_bbox_max'][leaves] - b['bvh_bbox_min'][leaves]).max(axis=1)))
    edits = {}
    if sa.num_spheres:
        edits['spheres'] = scatter(sa, 0.25, seed)
    if sa.num_quads:
        idx = np.arange(sa.num_quads)[::2]
        d = rng.uniform(-step, step, (idx.size, 3))
        q = sa.quads
        edits['quads'] = uh.quad_edit(idx, [tuple(tuple(map(float, p)) for p in
                                                  (q['quad_Q'][i] + d[k], q['quad_u'][i], q['quad_v'][i]))
                                            for k, i in enumerate(idx)])
    if sa.num_triangles:
        idx = np.arange(sa.num_triangles)[::3]
        d = rng.uniform(-step, step, (idx.size, 3))
        t = sa.tris
        edits['triangles'] = uh.tri_edit(idx, [tuple(tuple(map(float, t[key][i] + d[k])) for key in
                                                     ('triangle_v0', 'triangle_v1', 'triangle_v2'))
                                               for k, i in enumerate(idx)])
    return edits
