"""Rigid bodies (include/ptmi_rigid.h): the host definition of the
motion model of a *body*, a group of primitives that turn about an axis and
move together, and the ctypes binding of the rigid-body pose ABI.

A ``Body`` names spheres, quads and triangles by their reference indices (as in
``MI355XRenderer.primitives``) and has a ``pivot`` c, a unit ``axis`` a, a
``turn`` ω in radians per unit time and a ``displacement`` d per unit time. At a
time ``t`` the body is 15 doubles (``body_at``): ``R``, the rotation by ``ω * t``
about ``a`` (``rotation_matrix``: Rodrigues' formula with ``math.sin`` and
``math.cos``, written out once, here; the device receives the nine doubles and
never evaluates a sine), ``c`` and ``c'(t) = c + t * d``. A point goes to ``R *
(p - c) + c'`` and a vector to ``R * v``, every product rounded, then the sums of
a row left to right (``core.rigid_point``). The posed object is made by the
project's own float64 classes, so what the device leaves can be compared bit
for bit:

* sphere: ``Sphere.stationary(p'(center.origin), radius, mat)``;
* quad: ``core.quad.transformed(q, R, c, c')``;
* triangle: ``core.triangle.transformed(tri, R, c, c')``.

The quad's ``u, v, normal, w`` and the triangle's ``edge1, edge2, normal`` are
the REST object's vectors rotated, not formed anew from the posed points: the
constructors normalise through ``vec3.length_squared``, whose ``x ** 2`` is C
``pow`` and not ``x * x``, and would bring f64 ``sqrt`` and division onto the
device. Consequences:

* a posed normal is a unit vector only to float64 rounding;
* with ``ω = 0`` and ``d = 0``, ``R`` is exactly the identity and every rotated
  vector's row float compares ``==`` to the rest row's (a ``-0.0`` may become
  ``+0.0``); a point is ``(p - c) + c``, which is ``p`` wherever ``p - c`` is
  exact (a pivot at the origin, or within a factor two of ``p``) and otherwise
  ``p`` to a float64 rounding of ``|c|``, far below the f32 cast.
  ``DeviceScene.unpose`` restores every byte;
* a body with ``ω = 0`` is NOT bitwise the linear track ``p + t * d`` of
  ptmi.pose, and need not be.

``posed_records(bodies, prims, t)`` is ``scene_compiler.update_records`` of the
posed objects as ``DeviceScene.update_primitives`` arguments: the reference the
device call is tested against. ``body_records(bodies, prims)`` are the resident
f64 rest records ``DeviceScene.set_tracks(rigid=...)`` uploads.

Limits: one axis and one constant rate per body, no hierarchy; at most
``MAX_BODIES`` bodies; solid textures (checker, Perlin) and a sphere's image
texture orientation are functions of world position or normal and do not turn
with the body; poses are discrete (ptmi.pose): the arc a point travels in
pixels divided by the number of poses should stay below about one.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math

import numpy as np

from . import _lib, update
from .scene_data import STORAGE

RIGID_VERSION = 1  # PTMI_RIGID_VERSION of include/ptmi_rigid.h
MAX_BODIES = 16  # PTMI_RIGID_MAX_BODIES
BODY_DOUBLES = 15
# f64 per rest record, by API name
REC_DOUBLES = {'spheres': 3, 'quads': 15, 'triangles': 18}
KIND_NAMES = tuple(k.name for k in STORAGE)


class RigidBody(C.Structure):
    """ptmi_rigid_body."""
    _fields_ = [('R', C.c_double * 9), ('pivot', C.c_double * 3), ('pivot_t', C.c_double * 3)]


class RigidList(C.Structure):
    """ptmi_rigid_list."""
    _fields_ = [('prim', C.c_void_p), ('leaf', C.c_void_p), ('body', C.c_void_p), ('rec', C.c_void_p),
                ('count', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_rigid.h: name -> (restype, argtypes)."""
    P = C.c_void_p
    L, T = C.POINTER(RigidList), C.POINTER(update.UpdateTopology)
    return {
        'ptmi_pose_rigid': (C.c_int, [C.POINTER(_lib.SceneView), L, L, L, C.POINTER(RigidBody), C.c_int32, T, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the rigid-body pose export bound; a
    library without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


# ------------------------------------------------------------------ the motion model
def _finite3(name, v):
    from . import core
    if not isinstance(v, core.vec3) or not all(math.isfinite(x) for x in v.to_list()):
        raise ValueError(f'body: {name} must be a finite vec3')
    return v.copy()


class Body:
    """A group of primitives that turn by ``turn`` radians per unit time about
    ``axis`` through ``pivot`` while the pivot moves by ``displacement`` per unit
    time. ``spheres``, ``quads`` and ``triangles`` are reference indices. The
    axis is normalised once (``x * x``, ``math.sqrt``, ``/``). A value that is
    not finite, a zero axis or a repeated index is a ValueError."""
    __slots__ = ('pivot', 'axis', 'turn', 'displacement', 'spheres', 'quads', 'triangles')

    def __init__(self, pivot, axis, turn, displacement=None, spheres=(), quads=(), triangles=()):
        from . import core
        self.pivot = _finite3('pivot', pivot)
        a = _finite3('axis', axis)
        n = math.sqrt(a.x * a.x + a.y * a.y + a.z * a.z)
        if n == 0.0 or not math.isfinite(n):
            raise ValueError('body: the axis must not be zero')
        self.axis = core.vec3(a.x / n, a.y / n, a.z / n)
        self.turn = float(turn)
        if not math.isfinite(self.turn):
            raise ValueError('body: turn must be finite')
        self.displacement = _finite3('displacement', displacement if displacement is not None else core.vec3(0, 0, 0))
        for name, idx in zip(KIND_NAMES, (spheres, quads, triangles)):
            idx = tuple(idx)
            if not all(isinstance(i, (int, np.integer)) and i >= 0 for i in idx):
                raise ValueError(f'body: {name} must be primitive indices >= 0')
            idx = tuple(sorted(int(i) for i in idx))
            if len(set(idx)) != len(idx):
                raise ValueError(f'body: an index of {name} is repeated')
            setattr(self, name, idx)

    def members(self, name):
        return getattr(self, name)


def rotation_matrix(axis, angle):
    """The rotation by ``angle`` radians about the unit ``axis``, nine floats
    row-major, by Rodrigues' formula: ``cos I + sin [a]x + (1 - cos) a a^T``.
    ``angle == 0`` gives exactly the identity (an off-diagonal zero may be
    ``-0.0``, which changes no product's sum)."""
    s, c = math.sin(angle), math.cos(angle)
    k = 1.0 - c
    x, y, z = axis.x, axis.y, axis.z
    return (c + k * x * x, k * x * y - s * z, k * x * z + s * y,
            k * y * x + s * z, c + k * y * y, k * y * z - s * x,
            k * z * x - s * y, k * z * y + s * x, c + k * z * z)


def body_at(body, t):
    """The 15 doubles of ``body`` at time ``t`` (ptmi_rigid_body): ``R`` by
    ``rotation_matrix(axis, turn * t)``, the pivot ``c`` and ``c + t * d``."""
    t = float(t)
    moved = body.pivot + t * body.displacement
    return rotation_matrix(body.axis, body.turn * t) + tuple(body.pivot.to_list()) + tuple(moved.to_list())


def body_table(bodies, t):
    """``(RigidBody * MAX_BODIES)`` of ``body_at`` of every body: ptmi_pose_rigid's host table."""
    table = (RigidBody * MAX_BODIES)()
    for entry, b in zip(table, bodies):
        v = body_at(b, t)
        entry.R[:], entry.pivot[:], entry.pivot_t[:] = v[:9], v[9:12], v[12:]
    return table


def members_of(bodies):
    """``{'spheres': {i: body index}, 'quads': {...}, 'triangles': {...}}`` of a
    list of bodies. More than ``MAX_BODIES`` bodies, something that is not a
    Body, or a primitive in two bodies is a ValueError."""
    bodies = list(bodies)
    if len(bodies) > MAX_BODIES:
        raise ValueError(f'at most {MAX_BODIES} bodies, not {len(bodies)}')
    out = {name: {} for name in KIND_NAMES}
    for b, body in enumerate(bodies):
        if not isinstance(body, Body):
            raise ValueError(f'bodies[{b}] is not a rigid.Body')
        for name in KIND_NAMES:
            for i in body.members(name):
                if i in out[name]:
                    raise ValueError(f'{name}[{i}] is in bodies {out[name][i]} and {b}')
                out[name][i] = b
    return out


def posed_object(name, obj, at):
    """The object of kind ``name`` of a body whose ``body_at`` is ``at`` (the table above)."""
    from . import core  # the object model stays out of the import of ptmi.device, which binds this ABI
    R, c, c_t = at[:9], core.vec3(*at[9:12]), core.vec3(*at[12:15])
    if name == 'spheres':
        return core.Sphere.stationary(core.rigid_point(R, c, c_t, obj.center.origin), obj.radius, obj.material)
    if name == 'quads':
        return core.quad.transformed(obj, R, c, c_t)
    return core.triangle.transformed(obj, R, c, c_t)


def posed_records(bodies, prims, t):
    """``DeviceScene.update_primitives``' arguments for the bodies' primitives at
    ``t``: per kind, in its order, ``(indices, rows, build records)`` of
    ``scene_compiler.update_records`` of the posed objects, or None. ``prims``:
    the scene's primitive lists by API name, compile order."""
    from . import scene_compiler
    members = members_of(bodies)
    at = [body_at(b, t) for b in bodies]
    order = {name: sorted(members[name]) for name in KIND_NAMES}
    objs = [[posed_object(name, prims[name][i], at[members[name][i]]) for i in order[name]] for name in KIND_NAMES]
    records = scene_compiler.update_records(*objs)
    return tuple((np.asarray(order[name], np.int64), rows, build) if order[name] else None
                 for name, (rows, build) in zip(KIND_NAMES, records))


def rest_record(name, obj):
    """The f64 rest record of one object as include/ptmi_rigid.h lays it out."""
    if name == 'spheres':
        vs = (obj.center.origin,)
    elif name == 'quads':
        vs = (obj.Q, obj.u, obj.v, obj.normal, obj.w)
    else:
        vs = (obj.v0, obj.v1, obj.v2, obj.edge1, obj.edge2, obj.normal)
    return [x for v in vs for x in v.to_list()]


def body_records(bodies, prims):
    """The resident lists of ``DeviceScene.set_tracks(rigid=(bodies, records))``:
    per kind ``(indices, int32 body index per entry, (n, 3 / 15 / 18) f64 rest
    records)``, or None."""
    members = members_of(bodies)
    out = []
    for name in KIND_NAMES:
        idx = sorted(members[name])
        if idx and idx[-1] >= len(prims[name]):
            raise ValueError(f'{name}: no primitive {idx[-1]} (the scene has {len(prims[name])})')
        rec = np.array([rest_record(name, prims[name][i]) for i in idx], np.float64).reshape(len(idx), REC_DOUBLES[name])
        out.append((np.asarray(idx, np.int64), np.array([members[name][i] for i in idx], np.int32), rec)
                   if idx else None)
    return tuple(out)


def check_bodies(counts, bodies, records):
    """set_tracks' ``rigid`` argument checked against the ByCode ``counts``:
    (the bodies as a list, {type code: (int64 indices, int32 body indices, (n, 3
    / 15 / 18) f64 records)} of the non-empty kinds). A ValueError otherwise."""
    bodies = list(bodies)
    members_of(bodies)
    if records is None or len(records) != 3:
        raise ValueError('rigid records must be (spheres, quads, triangles)')
    out = {}
    for k, arg in zip(STORAGE, records):
        if arg is None:
            continue
        name, width = k.name, REC_DOUBLES[k.name]
        idx, body, rec = arg
        idx = update.check_indices(name, idx, counts[k.code])
        n = int(idx.size)
        body = np.asarray(body)
        if body.shape != (n,) or body.dtype.kind not in 'iu' or (n and (body.min() < 0 or body.max() >= len(bodies))):
            raise ValueError(f'{name}: body indices must be n integers in [0, {len(bodies)})')
        rec = np.ascontiguousarray(rec, np.float64)
        if rec.size != n * width:
            raise ValueError(f'{name}: rest records must be (n, {width}) f64')
        rec = rec.reshape(n, width)
        if not np.isfinite(rec).all():
            raise ValueError(f'{name}: rest records must be finite')
        if n:
            out[k.code] = (idx, body.astype(np.int32), rec)
    return bodies, out


# ------------------------------------------------------------------ the swept bound of a turning primitive
PAD = 1e-4  # pt_update_math.hpp's upd_pad: a leaf box's smallest extent


def swept_box(rest_min, rest_max, body, t0, t1):
    """A box that holds the leaf box of a primitive of ``body`` at every time in
    ``[t0, t1]``, from its rest leaf box (f32 as in ``ref_nodes``, pad included,
    taken in float64): ρ is the largest distance from the pivot to the rest box's
    eight corners, plus ``1e-6 * (max(|c|, |c'|) + ρ)`` for the roundings of the
    model and of the f32 casts (of the posed values, relative to ``|c'| + ρ``,
    and of the rest box itself, relative to ``|c| + ρ``; an f32 cast is 6e-8),
    plus ``PAD`` as a margin for a posed box thinner than the pad, which is widened
    about its middle (no input is known that needs the ``|c|`` or the pad:
    DESIGN.md §25). The box is ``[min(c'(t0), c'(t1)) - ρ, max(c'(t0), c'(t1)) + ρ]``:
    a rotation keeps every point within ρ of the moved pivot, and the pivot's
    path is monotone per component. Conservative, not tight. ``rest_min`` and
    ``rest_max`` may be (n, 3) arrays of the boxes of n primitives of the body:
    the ends and the terms of ρ that do not depend on the box are computed
    once. Returns (min, max), float64, shaped like the input."""
    lo, hi = np.asarray(rest_min, np.float64), np.asarray(rest_max, np.float64)
    c = np.array(body.pivot.to_list())
    far = np.maximum(np.abs(lo - c), np.abs(hi - c))
    rho = np.sqrt((far * far).sum(axis=-1, keepdims=True))
    ends = np.array([(body.pivot + float(t) * body.displacement).to_list() for t in (t0, t1)])  # body_at's c'
    rho = rho + (1e-6 * (max(float(np.abs(ends).max()), float(np.abs(c).max())) + rho) + PAD)
    return ends.min(axis=0) - rho, ends.max(axis=0) + rho


def digest(bodies):
    """A hex digest of a list of bodies (their parameters and members): the checkpoint's ``bodies`` value."""
    h = hashlib.sha256()
    for b in bodies:
        h.update(np.array(b.pivot.to_list() + b.axis.to_list() + [b.turn] + b.displacement.to_list(),
                          np.float64).tobytes())
        for name in KIND_NAMES:
            h.update(np.array((len(b.members(name)),) + b.members(name), np.int64).tobytes())
    return h.hexdigest()
