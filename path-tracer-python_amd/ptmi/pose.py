"""Motion blur by poses (include/ptmi_pose.h): the host definition
of the motion model, the shutter sequence, and the ctypes binding of the pose
ABI.

A *track* names a primitive by its reference index and gives its displacement
``d`` over unit time. The posed object at a time ``t`` is made by the project's
own float64 classes, so what the device leaves can be compared bit for bit:

* sphere: ``Sphere.stationary(o + t * d, radius, mat)`` with ``o, d`` the
  object's ``center.origin, center.direction`` (exactly ``center.at(t)``);
* quad: ``quad(Q + t * d, u, v, mat)``: the constructor gives the same
  ``normal`` and ``w`` and ``D = normal.dot(Q + t * d)``;
* triangle: ``core.triangle.translated(tri, t * d)``: the vertices moved, the
  edges and the normal kept.

``tracks`` is ``{'spheres': {i: (obj, d)}, 'quads': {...}, 'triangles': {...}}``
(``tracks_of`` makes it from a renderer's primitive lists and motion dict).
``posed_records(tracks, t)`` is ``scene_compiler.update_records`` of the posed
objects as ``DeviceScene.update_primitives`` arguments: the reference the
device call is tested against. ``track_records(tracks)`` are the f64 records
``DeviceScene.set_tracks`` uploads.

Shutter times: slice ``j`` is the samples ``[j * slice_spp, (j + 1) * slice_spp)``
of the counter stream, whatever the chunks of the render calls, and is traced
at ``t_j = t0 + (t1 - t0) * vdc(j)``, ``vdc`` the base-2 radical inverse. Any
prefix of poses is spread over the shutter, so progressive and adaptive renders
converge to the same blur. With ``N = 2^m`` poses the times are ``k / N``: their
mean is ``(N - 1) / 2N``, not 1/2 (the shutter's closing instant is never
sampled). Poses are discrete: an object whose travel in pixels divided by the
number of poses exceeds about one pixel shows as separate ghosts, not a smear.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib, update
from .scene_data import STORAGE

POSE_VERSION = 1  # PTMI_POSE_VERSION of include/ptmi_pose.h
# Samples per pose. 16 gives 64 poses at 1024 spp: a choice for the blur's
# quality, not for speed. On vol2 800x800 at 1024 spp a blurred render runs at
# 0.60 (megakernel) and 0.74 (wavefront) of the unblurred rate with 16, at 0.87
# and 0.92 with 32, at 0.94 and 0.99 with 64 (profiles/motion_blur/sweep.json):
# the pose calls are 1 % of the time, the rest is that every slice is a small
# render call that has to drain before the scene may change.
SLICE_SPP = 16
# f64 per track record, by API name
REC_DOUBLES = {'spheres': 6, 'quads': 9, 'triangles': 12}


class PoseList(C.Structure):
    """ptmi_pose_list."""
    _fields_ = [('prim', C.c_void_p), ('leaf', C.c_void_p), ('rec', C.c_void_p), ('count', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_pose.h: name -> (restype, argtypes)."""
    P = C.c_void_p
    L, T = C.POINTER(PoseList), C.POINTER(update.UpdateTopology)
    return {
        'ptmi_pose_primitives': (C.c_int, [C.POINTER(_lib.SceneView), L, L, L, C.c_double, T, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the pose export bound; a library
    without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


# ------------------------------------------------------------------ the shutter sequence
def vdc(j):
    """The base-2 radical inverse of ``j``: its low 32 bits reversed, divided by 2^32 (exact in float64)."""
    return int(f'{int(j) & 0xffffffff:032b}'[::-1], 2) / 4294967296.0


def check_shutter(shutter, slice_spp):
    """``(t0, t1)`` as floats and ``slice_spp`` as an int, or a ValueError."""
    try:
        t0, t1 = (float(x) for x in shutter)
    except (TypeError, ValueError):
        raise ValueError(f'shutter must be (t0, t1), not {shutter!r}') from None
    if not (math.isfinite(t0) and math.isfinite(t1) and t0 <= t1):
        raise ValueError(f'shutter must be finite with t0 <= t1, not {shutter!r}')
    if int(slice_spp) != slice_spp or int(slice_spp) < 1:
        raise ValueError(f'slice_spp must be a whole number >= 1, not {slice_spp!r}')
    return (t0, t1), int(slice_spp)


def slice_times(sample_begin, count, slice_spp, shutter):
    """The slices that samples ``[sample_begin, sample_begin + count)`` fall into:
    a list of ``(slice, t, begin, n)``: slice ``j``, its shutter time ``t0 +
    (t1 - t0) * vdc(j)`` and the part ``[begin, begin + n)`` of the range that
    lies in it. Sample ``s`` is always in slice ``s // slice_spp``."""
    (t0, t1), slice_spp = check_shutter(shutter, slice_spp)
    begin, end, out = int(sample_begin), int(sample_begin) + int(count), []
    if begin < 0:
        raise ValueError('sample_begin must be >= 0')
    while begin < end:
        j = begin // slice_spp
        stop = min(end, (j + 1) * slice_spp)
        out.append((j, t0 + (t1 - t0) * vdc(j), begin, stop - begin))
        begin = stop
    return out


# ------------------------------------------------------------------ the motion model
def _is_zero(d):
    return d.x == 0.0 and d.y == 0.0 and d.z == 0.0


def tracks_of(prims, motion=None):
    """The tracks of a scene's primitive lists (``{'spheres': [...], 'quads':
    [...], 'triangles': [...]}``, compile order): every sphere whose
    ``center.direction`` is not zero, and the quads and triangles ``motion``
    (``{'quads': {i: vec3 d}, 'triangles': {...}}``) names."""
    motion = motion or {}
    tracks = {'spheres': {i: (s, s.center.direction) for i, s in enumerate(prims['spheres'])
                          if not _is_zero(s.center.direction)}}
    for name in ('quads', 'triangles'):
        tracks[name] = {int(i): (prims[name][i], d) for i, d in sorted(motion.get(name, {}).items())}
    return tracks


def posed_object(name, obj, d, t):
    """The object of kind ``name`` with displacement ``d`` at time ``t`` (the table above)."""
    from . import core  # the object model stays out of the import of ptmi.device, which binds this ABI
    t = float(t)
    if name == 'spheres':
        return core.Sphere.stationary(obj.center.origin + t * d, obj.radius, obj.material)
    if name == 'quads':
        return core.quad(obj.Q + t * d, obj.u, obj.v, obj.mat)
    return core.triangle.translated(obj, t * d)


def posed_records(tracks, t):
    """``DeviceScene.update_primitives``' arguments for the tracked primitives at
    ``t``: per kind, in its order, ``(indices, rows, build records)`` of
    ``scene_compiler.update_records`` of the posed objects, or None."""
    from . import scene_compiler
    order = {k.name: sorted(tracks.get(k.name, {})) for k in STORAGE}
    objs = [[posed_object(k.name, *tracks[k.name][i], t) for i in order[k.name]] for k in STORAGE]
    records = scene_compiler.update_records(*objs)
    return tuple((np.asarray(order[k.name], np.int64), rows, build) if order[k.name] else None
                 for k, (rows, build) in zip(STORAGE, records))


def track_records(tracks):
    """``DeviceScene.set_tracks``' arguments: per kind ``(indices, (n, 6 / 9 / 12) f64 records)`` as
    include/ptmi_pose.h lays them out, or None."""
    out = []
    for k in STORAGE:
        tr = tracks.get(k.name, {})
        idx = sorted(tr)
        rec = np.zeros((len(idx), REC_DOUBLES[k.name]), np.float64)
        for row, i in zip(rec, idx):
            obj, d = tr[i]
            if k.name == 'spheres':
                row[:] = obj.center.origin.to_list() + d.to_list()
            elif k.name == 'quads':
                row[:] = obj.Q.to_list() + d.to_list() + obj.normal.to_list()
            else:
                row[:] = obj.v0.to_list() + obj.v1.to_list() + obj.v2.to_list() + d.to_list()
        out.append((np.asarray(idx, np.int64), rec) if idx else None)
    return tuple(out)


def check_tracks(counts, spheres=None, quads=None, triangles=None):
    """set_tracks' arguments checked against the ByCode ``counts``, like
    ``update.check_edits``: {type code: (int64 indices, (n, 6 / 9 / 12) f64
    records)} of the non-empty ones. A ValueError otherwise."""
    tracks = {}
    for k, arg in zip(STORAGE, (spheres, quads, triangles)):
        if arg is None:
            continue
        name, count, width = k.name, counts[k.code], REC_DOUBLES[k.name]
        idx, rec = arg
        idx = update.check_indices(name, idx, count)
        n = int(idx.size)
        rec = np.ascontiguousarray(rec, np.float64)
        if rec.size != n * width:
            raise ValueError(f'{name}: track records must be (n, {width}) f64')
        rec = rec.reshape(n, width)
        if not np.isfinite(rec).all():
            raise ValueError(f'{name}: track records must be finite')
        if n:
            tracks[k.code] = (idx, rec)
    return tracks
