"""ctypes binding of the tile-listed wavefront ABI (include/ptmi_wf_tiles.h):
the wavefront stats render restricted to a list of the frame's 64-pixel tiles.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib

WF_TILES_VERSION = 1  # PTMI_WF_TILES_VERSION of include/ptmi_wf_tiles.h


def _signatures():
    """Every export of include/ptmi_wf_tiles.h: name -> (restype, argtypes)."""
    P, I, Z = C.c_void_p, C.c_int32, C.c_size_t
    S, F = C.POINTER(_lib.SceneView), C.POINTER(_lib.Frame)
    return {
        'ptmi_wf_render_tiles_stats': (C.c_int, [S, F, P, Z, P, P, P, I, I, I, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the listed wavefront export bound; a
    library without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)
