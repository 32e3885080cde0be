"""ctypes binding of the scene-update ABI (include/ptmi_update.h): primitives of
a resident scene moved in place and its BVH refitted on the device.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.

``topology`` builds what the call needs once per scene from the reference-layout
BVH arrays; ``DeviceScene.update_primitives`` (ptmi.device) is the caller, and
its numpy halves are here: ``index_maps``, ``check_edits``, ``refresh_mirror``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .scene_data import (ByCode, KINDS, PRIM_QUAD, PRIM_SPHERE, STORAGE, fill_node_boxes, leaf_depths, node_slots,
                         shell_hint, unpack_quads, unpack_tris)

UPDATE_VERSION = 1  # PTMI_UPDATE_VERSION of include/ptmi_update.h
ONE_GROUP = 1  # PTMI_UPDATE_ONE_GROUP
ONE_GROUP_MAX_LEVELS = 64  # PTMI_UPDATE_ONE_GROUP_MAX_LEVELS
# The single-workgroup refit was measured faster than one launch per level on
# trees of 3016 to 3407 internal nodes (40 against 56 - 62 us per call,
# profiles/update/one_group_vs_per_level.json); one workgroup does not scale
# with the tree, so larger trees, not measured, keep one launch per level.
ONE_GROUP_MAX_INNER = 4096


class UpdateList(C.Structure):
    """ptmi_update_list."""
    _fields_ = [('prim', C.c_void_p), ('leaf', C.c_void_p), ('row', C.c_void_p), ('build', C.c_void_p),
                ('count', C.c_int32)]


class UpdateTopology(C.Structure):
    """ptmi_update_topology."""
    _fields_ = [('order', C.c_void_p), ('slot', C.c_void_p), ('level_end', C.POINTER(C.c_int32)),
                ('n_levels', C.c_int32), ('flags', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_update.h: name -> (restype, argtypes)."""
    P = C.c_void_p
    L, T = C.POINTER(UpdateList), C.POINTER(UpdateTopology)
    return {
        'ptmi_update_primitives': (C.c_int, [C.POINTER(_lib.SceneView), L, L, L, T, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the update export bound; a library
    without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def refit_flags(n_inner, n_levels):
    """The flags DeviceScene.update_primitives passes for a tree of this size."""
    return ONE_GROUP if 0 < n_inner <= ONE_GROUP_MAX_INNER and n_levels <= ONE_GROUP_MAX_LEVELS else 0


def topology(bvh):
    """(order, level_end, slot) of a reference-layout BVH (scene_data.BVH_KEYS):
    the internal nodes' reference indices deepest level first (within a level
    in preorder), the end of each level in ``order``, and each internal node's
    row in the device node array (-1 for leaves), all int32."""
    left, right, pidx = bvh['bvh_left_child'], bvh['bvh_right_child'], bvh['bvh_prim_idx']
    is_leaf = pidx >= 0
    slot, _ = node_slots(left, right, is_leaf)
    inner = np.nonzero(~is_leaf)[0]
    if inner.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), slot.astype(np.int32)
    depth = leaf_depths(bvh)[inner]
    by_depth = np.argsort(-depth.astype(np.int64), kind='stable')
    order = inner[by_depth].astype(np.int32)
    levels = np.bincount(depth)[::-1]  # deepest first; every depth up to the deepest internal node is taken
    level_end = np.cumsum(levels[levels > 0]).astype(np.int32)
    return order, level_end, slot.astype(np.int32)


def index_maps(bvh, prim_perm, counts):
    """What an update needs of one tree, as numpy arrays: ``topology``; ``leaf_of`` and ``dev_of``, ByCode of maps
    from a reference primitive index to its leaf's node and to its device row (``prim_perm``'s inverse); the
    internal nodes with their node rows and children. ``counts``: ByCode."""
    order, level_end, slot = topology(bvh)
    ptype, pidx = bvh['bvh_prim_type'], bvh['bvh_prim_idx']
    leaves = np.nonzero(pidx >= 0)[0]
    leaf_of = ByCode(*(np.full(n, -1, np.int64) for n in counts))
    for t in range(3):
        sel = leaves[ptype[leaves] == t]
        leaf_of[t][pidx[sel]] = sel
    inner = np.nonzero(pidx < 0)[0]
    return {'order': order, 'level_end': level_end, 'slot_np': slot, 'leaf_of': leaf_of,
            'dev_of': ByCode(*(np.argsort(p) for p in prim_perm)), 'inner': inner, 'rows': slot[inner].astype(np.int64),
            'left': bvh['bvh_left_child'][inner], 'right': bvh['bvh_right_child'][inner]}


def check_indices(name, idx, count):
    """Reference primitive indices of kind ``name`` as a 1-D int64 array: integers, within [0, count), none twice.
    A ValueError otherwise."""
    idx = np.asarray(idx)
    n = int(idx.size)
    if idx.ndim != 1 or (n and not np.issubdtype(idx.dtype, np.integer)):
        raise ValueError(f'{name}: indices must be a 1-D integer array')
    idx = idx.astype(np.int64)
    if n and (idx.min() < 0 or idx.max() >= count):
        raise ValueError(f'{name}: an index is outside [0, {count})')
    if np.unique(idx).size != n:
        raise ValueError(f'{name}: an index is repeated')
    return idx


def check_edits(counts, spheres=None, quads=None, triangles=None):
    """update_primitives' arguments checked against the ByCode ``counts``: {type code: (int64 indices,
    (n, row floats) rows, (n, build floats) build records)} of the non-empty ones. A ValueError otherwise."""
    edits = {}
    for k, arg in zip(STORAGE, (spheres, quads, triangles)):
        if arg is None:
            continue
        name, count = k.name, counts[k.code]
        idx, rows, build = arg
        idx = check_indices(name, idx, count)
        n = int(idx.size)
        rows, build = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(build, np.float32)
        if rows.size != n * k.row_floats or build.size != n * k.build_floats:
            raise ValueError(f'{name}: rows must be (n, {k.row_floats}) and build records (n, {k.build_floats}) f32')
        rows, build = rows.reshape(n, k.row_floats), build.reshape(n, k.build_floats)
        if not (np.isfinite(rows).all() and np.isfinite(build).all()):
            raise ValueError(f'{name}: rows and build records must be finite')
        points = rows[:, k.build_columns]
        if points.tobytes() != build[:, :points.shape[1]].tobytes():
            raise ValueError(f'{name}: a row and its build record name different points')
        if n:
            edits[k.code] = (idx, rows, build)
    return edits


def current_edits(sa, lay, maps, indices):
    """The edits that write back what the mirror holds: for ``indices`` ({type code: int64 reference indices})
    ``check_edits``' form {type code: (indices, rows, build records)}, the rows the layout's own, the build records
    from the mirror's arrays. The rest list of DeviceScene.set_tracks."""
    out = {}
    for t, idx in indices.items():
        k = KINDS[t]
        rows = np.ascontiguousarray(getattr(lay, k.rows)[maps['dev_of'][t][idx]], np.float32)
        if t == PRIM_SPHERE:
            build = rows.copy()
        elif t == PRIM_QUAD:
            build = np.ascontiguousarray(rows[:, k.build_columns])
        else:
            tr = sa.tris
            build = np.concatenate([tr['triangle_v0'][idx], tr['triangle_v1'][idx], tr['triangle_v2'][idx]],
                                   axis=1).astype(np.float32)
        out[t] = (idx, rows, build)
    return out


def refresh_mirror(sa, lay, maps, edits, ref_nodes):
    """A scene's SceneArrays and DeviceLayout, in place, after a finished update: the edited primitives from
    ``check_edits``' edits, the boxes from the device's ``ref_nodes`` read back (not read for an empty tree), the
    shell hint evaluated anew. ``maps``: ``index_maps`` of the tree."""
    for t, (idx, rows, build) in edits.items():
        k = KINDS[t]
        if t == PRIM_SPHERE:
            sa.sphere_data[idx] = rows
        else:
            mirror = getattr(sa, k.geometry)
            for key, values in (unpack_quads(rows) if t == PRIM_QUAD else unpack_tris(rows, build)).items():
                mirror[key][idx] = values
        getattr(lay, k.rows)[maps['dev_of'][t][idx]] = rows
    nb = sa.num_bvh_nodes
    if nb:
        rn = np.asarray(ref_nodes).reshape(-1, 12)[:nb]
        bmin, bmax = sa.bvh['bvh_bbox_min'], sa.bvh['bvh_bbox_max']
        bmin[:], bmax[:], lay.ref_nodes[:] = rn[:, 0:3], rn[:, 4:7], rn
        if maps['inner'].size:
            fill_node_boxes(lay.nodes, maps['rows'], bmin, bmax, maps['left'], maps['right'])
        lay.root_min[:], lay.root_max[:] = rn[0, 0:3], rn[0, 4:7]
        lay.shell = shell_hint(sa, maps['slot_np'], lay.max_leaf_depth, lay.nodes.shape[1] * 4)
