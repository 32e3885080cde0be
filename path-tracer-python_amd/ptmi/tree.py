"""ctypes binding of the tree-quality ABI (include/ptmi_tree.h): the box areas
of a resident scene's BVH, their growth since the tree was built, and the remap
of an id image across a rebuild.

The entry points live in the same libptmi.so as the integrator's and are loaded
through ``_lib.load()``; their signature table is kept here and bound by
``_lib.bind``.

``DeviceScene.tree_growth`` and ``DeviceScene.rebuild`` (ptmi.device) are the
callers; ``device_maps`` is the host half of a rebuild's row maps.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .scene_data import ByCode, KINDS

TREE_VERSION = 1  # PTMI_TREE_VERSION of include/ptmi_tree.h
GROWTH_LANES = 1024  # PTMI_TREE_GROWTH_LANES

# The mean growth above which update_primitives(rebuild='auto') rebuilds: the
# smallest swept growth at which one 64-spp 800x800 megakernel step on the refit
# tree costs more than the same step on a rebuilt tree plus the rebuild itself
# (profiles/rebuild/policy.json has the sweep and the derivation: vol2 on one
# MI355X, rebuild_bvh() 8.96 ms; the +-25 % scatter, growth 1.92, saves 2.6 ms per
# step, the +-50 % scatter, growth 3.895, saves 9.05 ms: the first to pay, by a
# narrow margin; +-100 %, growth 10.84, saves 34 ms). Just below that sweep
# point's growth, so that the point itself rebuilds. None would mean not
# measured, and 'auto' then needs an explicit rebuild_growth=.
REBUILD_GROWTH = 3.89


class IdsCounts(C.Structure):
    """ptmi_ids_counts: the primitive counts by type code."""
    _fields_ = [(k.name, C.c_int32) for k in KINDS]


def _signatures():
    """Every export of include/ptmi_tree.h: name -> (restype, argtypes)."""
    P, I = C.c_void_p, C.c_int32
    S = C.POINTER(_lib.SceneView)
    return {
        'ptmi_tree_areas': (C.c_int, [S, P, P]),
        'ptmi_tree_growth': (C.c_int, [S, P, P, P]),
        'ptmi_ids_remap': (C.c_int, [P, P, I, P, P, P, IdsCounts, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the tree exports bound; a library
    without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def device_maps(old_perm, new_perm):
    """ByCode of the int32 maps old device row -> new device row of two ``DeviceLayout.prim_perm`` (device row ->
    reference index) of the same primitives."""
    return ByCode(*(np.argsort(np.asarray(new, np.int64))[np.asarray(old, np.int64)].astype(np.int32)
                    for old, new in zip(old_perm, new_perm)))  # through the new permutation's inverse
