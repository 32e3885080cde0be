"""ctypes binding of the temporal ABI (include/ptmi_temporal.h): reprojection of
a stats render's history (accum and stats) from the previous camera to the
current one by the guide images of both.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

TEMPORAL_VERSION = 1  # PTMI_TEMPORAL_VERSION of include/ptmi_temporal.h


class ReprojectParams(C.Structure):
    """ptmi_reproject_params."""
    _fields_ = [('max_history', C.c_float), ('sigma_z', C.c_float), ('normal_min', C.c_float),
                ('sigma_a', C.c_float), ('flags', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_temporal.h: name -> (restype, argtypes)."""
    P, I = C.c_void_p, C.c_int32
    K, R = C.POINTER(_lib.Camera), C.POINTER(ReprojectParams)
    return {
        'ptmi_reproject': (C.c_int, [K, K, P, P, P, P, I, I, R, P, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the temporal exports bound; a library
    without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def params(max_history=32.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2):
    return ReprojectParams(float(max_history), float(sigma_z), float(normal_min), float(sigma_a), 0)


def camera(cam):
    """ptmi_camera (``_lib.Camera``) of a camera-upload dict
    (scene_data.camera_upload); a ``_lib.Camera`` is returned as it is."""
    if isinstance(cam, _lib.Camera):
        return cam
    c = _lib.Camera()
    for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v'):
        if k in cam:
            arr = np.asarray(cam[k], np.float32)
            for i in range(3):
                getattr(c, k)[i] = float(arr[i])
    c.defocus_angle = float(np.float32(cam.get('defocus_angle', 0.0)))
    return c
