"""What the rigid-body tests share (include/ptmi_rigid.h, ptmi/rigid.py): random
primitives and bodies as the Python definition takes them, the input and the
expected output of csrc/rigid_check.cpp, bodies of the test scenes, and the
oracle render of a blurred image, slice by slice on the numpy-refit arrays."""
import math

import numpy as np

import pose_helpers as psh
import update_helpers as uh
from ptmi import core, pose, rigid

f32 = np.float32
KINDS = psh.KINDS
MAT = psh.MAT
TIMES = [0.0, 1.0, 0.5, 1.0 / 3.0] + [pose.vdc(j) for j in range(1, 9)]
# the angle a body has turned by at t = 1: its turn
ANGLES = [0.0, 1e-9, math.pi / 7, math.pi / 2, math.pi, 2 * math.pi, 100.3]
STORAGE_POS = psh.STORAGE_POS
# what rigid_check prints of a row: the floats the kernel writes
WRITTEN = {'spheres': slice(0, 3), 'quads': slice(0, 16), 'triangles': slice(0, 12)}


def random_prims(kind, n, seed):
    """n objects of one kind, magnitudes 1e-3 .. 1e4."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if kind == 'spheres':
            out.append(core.Sphere.stationary(psh._vec(rng), float(10.0 ** rng.uniform(-3, 3)), MAT))
        elif kind == 'quads':
            u, v = psh._vec(rng), psh._vec(rng)
            out.append(core.quad(psh._vec(rng), u, v, MAT))
        else:
            a = psh._vec(rng)
            out.append(core.triangle(a, a + psh._vec(rng), a + psh._vec(rng), MAT))
    return out


def _origin(kind, obj):
    return {'spheres': lambda: obj.center.origin, 'quads': lambda: obj.Q, 'triangles': lambda: obj.v0}[kind]()


def random_bodies(kind, objs, seed):
    """16 bodies over ``objs`` (primitive i is in body i % 16): every angle of
    ANGLES with a pivot inside the data (a member's own point, nudged) and with
    one 1e4 away, axes on the coordinate axes and off them in turn, and two more:
    a body that only moves and one that turns backwards. Random displacements."""
    rng = np.random.default_rng(seed)
    specs = [(a, far) for a in ANGLES for far in (False, True)] + [(0.0, False), (-2.5, True)]
    bodies = []
    for b, (angle, far) in enumerate(specs):
        members = list(range(b, len(objs), len(specs)))
        if far:
            pivot = core.vec3(*(rng.choice([-1.0, 1.0], 3) * 1e4 * rng.uniform(0.5, 1.0, 3)))
        else:
            pivot = _origin(kind, objs[members[0]]) + psh._vec(rng, -3.0, 0.0)
        if (b // 2 + b) % 2 == 0:  # bodies 0, 3, 4, 7, ...: near and far pivots both get coordinate axes
            axis = core.vec3(*np.roll([0.0, -1.0 if b % 8 >= 4 else 1.0, 0.0], b))
        else:
            axis = psh._vec(rng, -1.0, 1.0)
        d = core.vec3(0, 0, 0) if b == 0 else psh._vec(rng, -3.0, 2.0)
        bodies.append(rigid.Body(pivot, axis, angle, d, **{kind: members}))
    return bodies


def prim_lists(kind, objs):
    return {k: (objs if k == kind else []) for k in KINDS}


def check_input(kind, objs, bodies, t):
    """rigid_check's in.f64: per primitive its body at ``t``, its rest record and the row floats the kernel keeps."""
    members = rigid.members_of(bodies)[kind]
    at = [rigid.body_at(b, t) for b in bodies]
    rows = []
    for i in sorted(members):
        extra = [float(f32(objs[i].radius))] if kind == 'spheres' else []
        rows.append(list(at[members[i]]) + rigid.rest_record(kind, objs[i]) + extra)
    return np.array(rows, np.float64)


def expected(kind, objs, bodies, t):
    """rigid_check's out.f32 from the Python definition: the written row floats of
    ``posed_records`` and the box of its build records by update_helpers' rules."""
    _, rows, build = rigid.posed_records(bodies, prim_lists(kind, objs), t)[STORAGE_POS[kind]]
    mn, mx = psh.BOX_RULE[kind](build)
    return np.concatenate([rows[:, WRITTEN[kind]], mn, mx], axis=1).astype(f32)


def scene_body(name, width=None, spheres=(), quads=(), triangles=(), axis=(0.0, 1.0, 0.0), turn=0.5,
               displacement=(0.0, 0.0, 0.0), pivot=None):
    """A body of a test scene's primitives; the pivot defaults to the mean of the members' own points."""
    prims = psh.scene_prims(name, width)
    if pivot is None:
        pts = [_origin(k, prims[k][int(i)]).to_list() for k, idx in zip(KINDS, (spheres, quads, triangles)) for i in idx]
        pivot = np.mean(np.array(pts, np.float64), axis=0)
    return rigid.Body(core.vec3(*pivot), core.vec3(*axis), turn, core.vec3(*displacement), spheres=spheres,
                      quads=quads, triangles=triangles)


def oracle_blurred(scene, variant, window, prims, bodies, tracks, shutter, slice_spp, s_begin, s_count,
                   traversal='stack', seed=0, max_depth=50):
    """pose_helpers.oracle_blurred with bodies: every slice rendered by the CPU oracle on the numpy-refit arrays
    of the linear tracks' and the bodies' posed records (both record sets in one refit)."""
    import oracle
    sa, cam, bg = scene
    W, H = cam['width'], cam['height']
    fr = oracle.make_frame(cam, bg, max_depth, seed, W, H, traversal)
    acc = np.zeros((H, W, 3), f32)
    total = {}
    for _, t, b, n in pose.slice_times(s_begin, s_count, slice_spp, shutter):
        posed = uh.refit(sa, merged_edits(prims, bodies, tracks, t))
        stats = oracle.render(oracle.OracleScene(posed), fr, variant, acc, window, b, n, 0)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    return acc, total


def merged_edits(prims, bodies, tracks, t):
    """update_helpers.refit's dict of the bodies' posed records and, if any, the linear tracks' (disjoint primitives)."""
    out = psh.as_edits(rigid.posed_records(bodies, prims, t)) if bodies else {}
    for k, (idx, rows, build) in (psh.as_edits(pose.posed_records(tracks, t)) if tracks else {}).items():
        if k in out:
            out[k] = tuple(np.concatenate([a, b]) for a, b in zip(out[k], (idx, rows, build)))
        else:
            out[k] = (idx, rows, build)
    return out
