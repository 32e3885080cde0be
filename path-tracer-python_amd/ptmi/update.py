"""ctypes binding of the scene-update ABI (include/ptmi_update.h): primitives of
a resident scene moved in place and its BVH refitted on the device.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.

``topology`` builds what the call needs once per scene from the reference-layout
BVH arrays; ``DeviceScene.update_primitives`` (ptmi.device) is the caller.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

UPDATE_VERSION = 1  # PTMI_UPDATE_VERSION of include/ptmi_update.h
ONE_GROUP = 1  # PTMI_UPDATE_ONE_GROUP
ONE_GROUP_MAX_LEVELS = 64  # PTMI_UPDATE_ONE_GROUP_MAX_LEVELS
# The single-workgroup refit was measured faster than one launch per level on
# trees of 3016 to 3407 internal nodes (40 against 56 - 62 us per call,
# profiles/update/one_group_vs_per_level.json); one workgroup does not scale
# with the tree, so larger trees, not measured, keep one launch per level.
ONE_GROUP_MAX_INNER = 4096

# per primitive type code (scene_data.PRIM_*: sphere 0, triangle 1, quad 2): f32 per device row / build record
ROW_FLOATS = (4, 12, 16)
BUILD_FLOATS = (4, 9, 9)


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
    from .scene_data import leaf_depths, node_slots
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
