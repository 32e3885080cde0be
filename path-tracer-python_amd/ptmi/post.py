"""ctypes binding of the post-processing ABI (include/ptmi_post.h): the
variance-guided a-trous denoiser on a stats render's error estimates.

The entry points live in the same libptmi.so as the integrator's and are
loaded through ``_lib.load()``; their signature table is kept here and bound by
``_lib.bind``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

POST_VERSION = 1  # PTMI_POST_VERSION of include/ptmi_post.h
MAX_ITERATIONS = 8


def _signatures():
    """Every export of include/ptmi_post.h: name -> (restype, argtypes)."""
    P, I, Z, F = C.c_void_p, C.c_int32, C.c_size_t, C.c_float
    return {
        'ptmi_denoise_workspace_bytes': (Z, [I, I]),
        'ptmi_denoise': (C.c_int, [P, P, I, I, I, F, P, Z, P, P, P]),
        'ptmi_denoise_set_lds_max_step': (C.c_int, [I]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the post-processing exports bound; a
    library without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def workspace_bytes(width, height):
    need = int(load().ptmi_denoise_workspace_bytes(int(width), int(height)))
    if need == 0:
        _lib.check(_lib.PTMI_EINVAL, 'ptmi_denoise_workspace_bytes')
    return need


def set_lds_max_step(max_step):
    """Passes of step <= max_step stage their taps in LDS (0: none; default and
    maximum 2). Same bits either way; for A/B timing and tests. Returns the
    previous value."""
    prev = load().ptmi_denoise_set_lds_max_step(int(max_step))
    if prev < 0:
        _lib.check(prev, 'ptmi_denoise_set_lds_max_step')
    return prev
