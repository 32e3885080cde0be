"""ctypes binding of the guide ABI (include/ptmi_guide.h): first-hit guide
buffers (normal, depth, albedo) and the a-trous denoiser guided by them.

The entry points live in the same libptmi.so as the integrator's and are
loaded through ``_lib.load()``; their signature table is kept here and bound by
``_lib.bind``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

GUIDE_VERSION = 1  # PTMI_GUIDE_VERSION of include/ptmi_guide.h
DN_DEMODULATE = 1  # PTMI_DN_DEMODULATE
GUIDE_CHANNELS = 8  # {nx, ny, nz, depth, ar, ag, ab, hit}
MAX_NORMAL_POWER_LOG2 = 7


class GuidedParams(C.Structure):
    """ptmi_dn_guided_params."""
    _fields_ = [('iterations', C.c_int32), ('sigma', C.c_float), ('sigma_z', C.c_float), ('sigma_a', C.c_float),
                ('normal_power_log2', C.c_int32), ('flags', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_guide.h: name -> (restype, argtypes)."""
    P, I, Z = C.c_void_p, C.c_int32, C.c_size_t
    S, F, G = C.POINTER(_lib.SceneView), C.POINTER(_lib.Frame), C.POINTER(GuidedParams)
    return {
        'ptmi_guide_trace': (C.c_int, [S, F, P, P]),
        'ptmi_denoise_guided': (C.c_int, [P, P, P, I, I, G, P, Z, P, P, P]),
        'ptmi_denoise_guided_set_lds_max_step': (C.c_int, [I]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the guide exports bound; a library
    without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def params(iterations=5, sigma=4.0, sigma_z=0.1, sigma_a=0.2, normal_power_log2=5, demodulate=True):
    return GuidedParams(int(iterations), float(sigma), float(sigma_z), float(sigma_a), int(normal_power_log2),
                        DN_DEMODULATE if demodulate else 0)


def set_lds_max_step(max_step):
    """Guided passes of step <= max_step stage their colour taps in LDS (0:
    none; default and maximum 2). Same bits either way; for A/B timing and
    tests. Returns the previous value."""
    prev = load().ptmi_denoise_guided_set_lds_max_step(int(max_step))
    if prev < 0:
        _lib.check(prev, 'ptmi_denoise_guided_set_lds_max_step')
    return prev
