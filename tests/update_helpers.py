"""numpy f32 reference of the scene-update ABI (include/ptmi_update.h).

``refit(sa, edits)`` applies primitive edits to reference-layout arrays and
refits the BVH: the leaf boxes in numpy f32 by the builder's rules, then the
bottom-up union over ``bvh_left_child`` / ``bvh_right_child``. ``pack_device`` of
the result is the expected device image, and the oracle renders from it.

``edits`` maps 'spheres' / 'quads' / 'triangles' to ``(reference primitive
indices, rows, build records)``, the arguments of
``DeviceScene.update_primitives``."""
import dataclasses

import numpy as np

f32 = np.float32
DELTA, HALF = f32(0.0001), f32(5e-05)


def _min(a, b):
    return np.where(a < b, a, b).astype(f32)


def _max(a, b):
    return np.where(a > b, a, b).astype(f32)


def pad(mn, mx):
    """pad_to_minimums (sah_bvh_builder.py:31-39) on (n, 3) f32 boxes."""
    small = (mx - mn) < DELTA
    mid = (mn + mx) / f32(2.0)
    return np.where(small, mid - HALF, mn).astype(f32), np.where(small, mid + HALF, mx).astype(f32)


def sphere_boxes(build):
    b = np.asarray(build, f32).reshape(-1, 4)
    return b[:, 0:3] - b[:, 3:4], b[:, 0:3] + b[:, 3:4]


def quad_boxes(build):
    b = np.asarray(build, f32).reshape(-1, 9)
    Q, u, v = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    c1, c2, c3 = Q + u, Q + v, (Q + u) + v
    return pad(_min(_min(_min(Q, c1), c2), c3), _max(_max(_max(Q, c1), c2), c3))


def tri_boxes(build):
    b = np.asarray(build, f32).reshape(-1, 9)
    v0, v1, v2 = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    return pad(_min(_min(v0, v1), v2), _max(_max(v0, v1), v2))


def union(lmn, lmx, rmn, rmx):
    return _min(lmn, rmn), _max(lmx, rmx)


def centre(mn, mx):
    return ((mn + mx) * f32(0.5)).astype(f32)


# type code, rule, f32 per device row, f32 per build record
BOXES = {'spheres': (0, sphere_boxes, 4, 4), 'triangles': (1, tri_boxes, 12, 9), 'quads': (2, quad_boxes, 16, 9)}


def leaf_of(sa, type_code):
    """Reference node index of the leaf of every primitive of a type."""
    ptype, pidx = sa.bvh['bvh_prim_type'], sa.bvh['bvh_prim_idx']
    leaves = np.nonzero((pidx >= 0) & (ptype == type_code))[0]
    out = np.full(len(leaves), -1, np.int64)
    out[pidx[leaves]] = leaves
    return out


def refit(sa, edits=None):
    """A new SceneArrays: ``sa`` with the edits applied and every internal box
    the union of its children's boxes."""
    edits = edits or {}
    b = dict(sa.bvh, bvh_bbox_min=np.array(sa.bvh['bvh_bbox_min'], f32),
             bvh_bbox_max=np.array(sa.bvh['bvh_bbox_max'], f32))
    out = dataclasses.replace(sa, sphere_data=np.array(sa.sphere_data, f32), bvh=b,
                              quads={k: np.array(v) for k, v in sa.quads.items()},
                              tris={k: np.array(v) for k, v in sa.tris.items()})
    bmin, bmax = b['bvh_bbox_min'], b['bvh_bbox_max']
    for name, (idx, rows, build) in edits.items():
        code, rule, nrow, nbuild = BOXES[name]
        idx = np.asarray(idx, np.int64)
        rows, build = np.asarray(rows, f32).reshape(len(idx), nrow), np.asarray(build, f32).reshape(len(idx), nbuild)
        if name == 'spheres':
            out.sphere_data[idx] = rows
        elif name == 'quads':
            for key, lo, hi in (('quad_normal', 0, 3), ('quad_Q', 4, 7), ('quad_u', 7, 10), ('quad_v', 10, 13),
                                ('quad_w', 13, 16)):
                out.quads[key][idx] = rows[:, lo:hi]
            out.quads['quad_D'][idx] = rows[:, 3]
        else:
            for key, src, lo in (('triangle_v0', build, 0), ('triangle_v1', build, 3), ('triangle_v2', build, 6),
                                 ('triangle_edge1', rows, 3), ('triangle_edge2', rows, 6),
                                 ('triangle_normal', rows, 9)):
                out.tris[key][idx] = src[:, lo:lo + 3]
        leaves = leaf_of(sa, code)[idx]
        bmin[leaves], bmax[leaves] = rule(build)
    left, right = b['bvh_left_child'], b['bvh_right_child']
    for i in range(len(left) - 1, -1, -1):  # preorder: children follow their parent
        if left[i] >= 0:
            bmin[i], bmax[i] = union(bmin[left[i]], bmax[left[i]], bmin[right[i]], bmax[right[i]])
    return out


def arrays_equal(a, b):
    """Byte equality of the geometry and the BVH arrays of two SceneArrays."""
    pairs = [(a.sphere_data, b.sphere_data)]
    pairs += [(a.quads[k], b.quads[k]) for k in a.quads] + [(a.tris[k], b.tris[k]) for k in a.tris]
    pairs += [(a.bvh[k], b.bvh[k]) for k in a.bvh]
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).dtype == np.asarray(y).dtype
               for x, y in pairs)


def layouts_equal(a, b):
    """Names of the DeviceLayout members in which two layouts differ (bytes)."""
    bad = [k for k in ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris', 'mats', 'root_min', 'root_max')
           if np.asarray(getattr(a, k), f32).tobytes() != np.asarray(getattr(b, k), f32).tobytes()]
    return bad + [k for k in ('shell', 'root_ref', 'max_leaf_depth') if getattr(a, k) != getattr(b, k)]


def sphere_edit(idx, centres, radii):
    rows = np.concatenate([np.asarray(centres, f32).reshape(-1, 3), np.asarray(radii, f32).reshape(-1, 1)], axis=1)
    return np.asarray(idx, np.int64).reshape(-1), rows, rows.copy()


def quad_edit(idx, quads):
    """quads: (Q, u, v) triples of 3-tuples; rows by the scene compiler's arithmetic."""
    from ptmi import core, scene_compiler
    objs = [core.quad(core.vec3(*Q), core.vec3(*u), core.vec3(*v), None) for Q, u, v in quads]
    rows, build = scene_compiler.update_records(quads=objs)[1]
    return np.asarray(idx, np.int64).reshape(-1), rows, build


def tri_edit(idx, tris):
    from ptmi import core, scene_compiler
    objs = [core.triangle(core.vec3(*a), core.vec3(*b), core.vec3(*c), None) for a, b, c in tris]
    rows, build = scene_compiler.update_records(triangles=objs)[2]
    return np.asarray(idx, np.int64).reshape(-1), rows, build


def current(sa, name, idx):
    """The edit that writes back what ``sa`` holds for primitives ``idx``: the inverse of any edit of them."""
    from ptmi import scene_data as sd
    idx = np.asarray(idx, np.int64).reshape(-1)
    if name == 'spheres':
        rows = np.array(sa.sphere_data[idx], f32)
        return idx, rows, rows.copy()
    if name == 'quads':
        q = sa.quads
        build = np.concatenate([q['quad_Q'][idx], q['quad_u'][idx], q['quad_v'][idx]], axis=1)
        return idx, sd.pack_quads(q)[idx], build
    t = sa.tris
    return idx, sd.pack_tris(t)[idx], np.concatenate([t['triangle_v0'][idx], t['triangle_v1'][idx],
                                                      t['triangle_v2'][idx]], axis=1)
