"""ctypes binding of the history-validation ABI (include/ptmi_validate.h): a
carried history compared with a few fresh samples over a window, its stale part
dropped, the two merged.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.

``Integrator.validate_history`` (ptmi.device) is the caller.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib

VALIDATE_VERSION = 1  # PTMI_VALIDATE_VERSION of include/ptmi_validate.h
MAX_RADIUS = 7  # PTMI_VALIDATE_MAX_RADIUS


class ValidateParams(C.Structure):
    """ptmi_validate_params."""
    _fields_ = [('radius', C.c_int32), ('k_lo', C.c_float), ('k_hi', C.c_float)]


def _signatures():
    """Every export of include/ptmi_validate.h: name -> (restype, argtypes)."""
    P, I = C.c_void_p, C.c_int32
    return {
        'ptmi_history_validate': (C.c_int, [P, P, P, P, I, I, C.POINTER(ValidateParams), P, P, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the validation export bound; a library
    without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def params(radius=3, k_lo=2.0, k_hi=4.0):
    """ptmi_validate_params; the ranges are the C call's to check, but a radius
    that is no whole number is refused here (the struct would truncate it)."""
    if isinstance(radius, float) and (not math.isfinite(radius) or radius != int(radius)):
        raise ValueError(f'radius must be a whole number, not {radius!r}')
    return ValidateParams(int(radius), float(k_lo), float(k_hi))
