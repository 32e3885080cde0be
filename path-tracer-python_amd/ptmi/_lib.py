"""ctypes binding of libptmi.so (the C-ABI declared in include/ptmi.h).

The library is built in-tree (``make -C path-tracer-python_amd/csrc`` or
``__graft_entry__.build()``) and loaded from ``ptmi/_lib/libptmi.so``. There is
no fallback: if the library is missing every render entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PTMI_LIB') or os.path.join(_HERE, '_lib', 'libptmi.so')  # PTMI_LIB: A/B builds
ABI_VERSION = 9  # PTMI_ABI_VERSION of include/ptmi.h
MAX_IMAGES = 16
NUM_COUNTERS = 6
COUNTER_TAIL_SEGMENTS = 5  # wavefront segments traced in the tail launch (wf_drain), part of [0]

PTMI_OK, PTMI_EINVAL, PTMI_ECAPACITY, PTMI_EHIP, PTMI_ENODEV = 0, -1, -2, -3, -4

f3 = C.c_float * 3


class SceneView(C.Structure):
    _fields_ = [
        ('nodes', C.c_void_p), ('n_inner', C.c_int32), ('root_ref', C.c_int32),
        ('root_min', f3), ('root_max', f3), ('max_leaf_depth', C.c_int32),
        ('spheres', C.c_void_p), ('quads', C.c_void_p), ('tris', C.c_void_p), ('mats', C.c_void_p),
        ('num_spheres', C.c_int32), ('num_quads', C.c_int32), ('num_triangles', C.c_int32),
        ('texels', C.c_void_p), ('num_images', C.c_int32),
        ('img_offset', C.c_int32 * MAX_IMAGES), ('img_w', C.c_int32 * MAX_IMAGES),
        ('img_h', C.c_int32 * MAX_IMAGES),
        ('perlin_vec', C.c_void_p), ('perlin_perm', C.c_void_p),
        ('ref_nodes', C.c_void_p), ('num_bvh_nodes', C.c_int32),
        ('shell', C.c_int32),  # enclosing medium shell hint (scene_data.find_shell), 0 = none
    ]


class Camera(C.Structure):
    _fields_ = [('center', f3), ('pixel00', f3), ('delta_u', f3), ('delta_v', f3),
                ('defocus_u', f3), ('defocus_v', f3), ('defocus_angle', C.c_float)]


class Frame(C.Structure):
    _fields_ = [('cam', Camera), ('bg', f3), ('max_depth', C.c_int32), ('seed', C.c_uint32),
                ('width', C.c_int32), ('height', C.c_int32),
                ('x0', C.c_int32), ('y0', C.c_int32), ('w', C.c_int32), ('h', C.c_int32),
                ('band_rows', C.c_int32), ('band_stride', C.c_int32), ('band_offset', C.c_int32),
                ('traversal', C.c_int32)]


# BVH traversal of a frame (ptmi_frame.traversal): the reference's
# traverse_bvh_legacy (default) or traverse_bvh_stackless, switched in the
# reference by USE_STACKLESS_TRAVERSAL (kernels.py:746)
TRAVERSALS = {'stack': 0, 'stackless': 1}


def _signatures():
    """Every export of include/ptmi.h: name -> (restype, argtypes)."""
    P, I, Z = C.c_void_p, C.c_int32, C.c_size_t
    S, F, IP = C.POINTER(SceneView), C.POINTER(Frame), C.POINTER(C.c_int32)
    return {
        'ptmi_version': (C.c_int, []),
        'ptmi_last_error': (C.c_char_p, []),
        'ptmi_scene_check': (C.c_int, [S]),
        'ptmi_mk_render': (C.c_int, [S, F, P, I, I, P, P]),
        'ptmi_mk_workspace_bytes': (Z, [F, I]),
        'ptmi_mk_render_ws': (C.c_int, [S, F, P, Z, P, I, I, P, P]),
        'ptmi_mk_trace_ws': (C.c_int, [S, F, P, Z, I, I, P, P]),
        'ptmi_mk_max_batch': (C.c_int64, [F]),
        'ptmi_mk_resolve_ws': (C.c_int, [F, P, Z, P, I, P]),
        'ptmi_wf_workspace_bytes': (Z, [F, I]),
        'ptmi_wf_render': (C.c_int, [S, F, P, Z, P, I, I, P, P]),
        'ptmi_clear': (C.c_int, [F, P, P]),
        'ptmi_tonemap': (C.c_int, [P, P, I, I, I, P]),
        'ptmi_bvh_build_sah': (C.c_int, [P, I, P, I, P, I, P, P, P, P, P, P, P, IP]),
        'ptmi_prof_start': (C.c_int, [I]),
        'ptmi_prof_stop': (C.c_int, [P, P, I]),
        'ptmi_prof_stop_busy': (C.c_int, [P, P, P, I]),
        'ptmi_node_bytes': (C.c_int, []),
        'ptmi_wf_set_drain_at': (C.c_int, [I]),
        # ABI v8: per-pixel error estimates and adaptive tile sampling
        'ptmi_mk_tile_grid': (C.c_int, [F, IP, IP, IP, IP]),
        'ptmi_stats_clear': (C.c_int, [F, P, P]),
        'ptmi_mk_trace_tiles_ws': (C.c_int, [S, F, P, Z, P, I, I, I, P, P]),
        'ptmi_mk_resolve_stats_ws': (C.c_int, [F, P, Z, P, P, P, I, I, P]),
        'ptmi_wf_render_stats': (C.c_int, [S, F, P, Z, P, P, I, I, P, P]),
        'ptmi_tile_update': (C.c_int, [F, P, C.c_float, I, I, P, P, P, P, P]),
        'ptmi_tonemap_stats': (C.c_int, [P, P, P, I, I, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)
PROF_KINDS = ('megakernel', 'wf_generate', 'wf_intersect', 'wf_drain', 'wf_scatter', 'wf_resolve', 'mk_resolve')

_lib = None


class PtmiError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load libptmi.so once; raises PtmiError (no silent fallback) if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise PtmiError(f'libptmi.so not built ({path}); run `make -C path-tracer-python_amd/csrc` '
                        'or __graft_entry__.build()')
    # One HIP runtime per process: torch's wheel carries its own libamdhip64
    # (soname libamdhip64.so.7, the same as /opt/rocm's). Loaded after torch,
    # libptmi binds to that copy; loaded first, it pulls in /opt/rocm's and
    # torch then maps a second runtime, under which ptmi's launches find no
    # device. So torch goes first whenever it is importable (the scene
    # compiler reaches this loader for the native SAH builder before any
    # device code runs).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ptmi_version() != ABI_VERSION:
        raise PtmiError(f'libptmi ABI version {lib.ptmi_version()} != {ABI_VERSION} (rebuild libptmi.so)')
    _lib = lib
    return lib


_bound = {}  # id of a signature table -> the library it was last bound to


def bind(lib, signatures):
    """Set restype and argtypes of the exports in ``signatures`` (name ->
    (restype, argtypes)) on ``lib``, once per table and library; a library
    without one of them raises PtmiError. Returns ``lib``."""
    if _bound.get(id(signatures)) is not lib:
        for name, (restype, argtypes) in signatures.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise PtmiError(f'libptmi.so has no {name} (rebuild libptmi.so)') from None
            fn.restype, fn.argtypes = restype, argtypes
        _bound[id(signatures)] = lib
    return lib


def check(rc: int, what: str):
    if rc != PTMI_OK:
        msg = load().ptmi_last_error().decode(errors='replace')
        raise PtmiError(f'{what} failed ({rc}): {msg}')
    return rc


class KernelTimer:
    """Per-kernel device time of libptmi's own launches (ptmi_prof_start/stop)."""

    def __init__(self, max_launches=200000):
        self.max_launches = int(max_launches)

    def __enter__(self):
        check(load().ptmi_prof_start(self.max_launches), 'ptmi_prof_start')
        self.result = None
        return self

    def __exit__(self, *exc):
        import numpy as np
        ms = np.zeros(len(PROF_KINDS), np.float64)
        busy = np.zeros(len(PROF_KINDS), np.float64)
        n = np.zeros(len(PROF_KINDS), np.uint64)
        rc = load().ptmi_prof_stop_busy(C.c_void_p(ms.ctypes.data), C.c_void_p(busy.ctypes.data),
                                        C.c_void_p(n.ctypes.data), len(PROF_KINDS))
        self.truncated = rc == PTMI_ECAPACITY  # more launches than events: totals cover the first ones
        if not self.truncated:
            check(rc, 'ptmi_prof_stop_busy')
        # ms: summed launch durations; busy_ms: union of the launches' intervals
        self.result = {k: {'ms': float(ms[i]), 'busy_ms': float(busy[i]), 'launches': int(n[i])}
                       for i, k in enumerate(PROF_KINDS)}
        return False
