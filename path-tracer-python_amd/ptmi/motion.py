"""ctypes binding of the motion ABI (include/ptmi_motion.h): the guide trace that
also writes which primitive each pixel sees, and the temporal reprojection that
follows a surface point back across a scene update.

The entry points live in the same libptmi.so as the integrator's and are loaded
through ``_lib.load()``; their signature table is kept here and bound by
``_lib.bind``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib, temporal

MOTION_VERSION = 1  # PTMI_MOTION_VERSION of include/ptmi_motion.h
RPM_MATCH_IDS = 1  # PTMI_RPM_MATCH_IDS
NO_ID = -1  # the id of a pixel that shows no surface
ID_TYPE_SHIFT = 28  # id = type << 28 | device primitive index


class ReprojectMovedParams(C.Structure):
    """ptmi_reproject_moved_params."""
    _fields_ = [('base', temporal.ReprojectParams), ('flags', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_motion.h: name -> (restype, argtypes)."""
    P, I = C.c_void_p, C.c_int32
    S, F = C.POINTER(_lib.SceneView), C.POINTER(_lib.Frame)
    K, R = C.POINTER(_lib.Camera), C.POINTER(ReprojectMovedParams)
    return {
        'ptmi_guide_trace_ids': (C.c_int, [S, F, P, P, P]),
        'ptmi_reproject_moved': (C.c_int, [K, K, P, P, P, P, P, P, S, P, P, P, I, I, R, P, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the motion exports bound; a library
    without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def params(max_history=32.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2, match_ids=True):
    return ReprojectMovedParams(temporal.params(max_history, sigma_z, normal_min, sigma_a),
                                RPM_MATCH_IDS if match_ids else 0)
