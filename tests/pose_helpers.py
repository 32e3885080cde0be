"""What the pose tests share (include/ptmi_pose.h, ptmi/pose.py): random tracks
as the Python definition takes them, the input and the expected output of
csrc/pose_check.cpp, the tracks of the test scenes, and the oracle render of a
blurred image, slice by slice on the numpy-refit arrays."""
import random

import numpy as np

import parity_helpers as ph
import update_helpers as uh
from ptmi import core, pose, scene_compiler, scene_data as sd

f32 = np.float32
TIMES = [0.0, 1.0, 0.5, 1.0 / 3.0, 0.1] + [pose.vdc(j) for j in range(1, 9)]
KINDS = ('spheres', 'quads', 'triangles')
MAT = core.lambertian(core.solid_color(core.vec3(0.5, 0.5, 0.5)))
BOX_RULE = {'spheres': uh.sphere_boxes, 'quads': uh.quad_boxes, 'triangles': uh.tri_boxes}
# the row floats a pose changes (the table of DESIGN.md §24), and what pose_check prints of a row
CHANGED = {'spheres': [0, 1, 2], 'quads': [3, 4, 5, 6], 'triangles': [0, 1, 2]}
STORAGE_POS = {'spheres': 0, 'quads': 1, 'triangles': 2}


def _vec(rng, lo=-3.0, hi=4.0):
    """A vec3 of magnitude 10^lo .. 10^hi, random signs."""
    return core.vec3(*(rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(lo, hi)))


def random_tracks(kind, n, seed):
    """{kind: {i: (object, d)}}: n tracks of one kind, magnitudes 1e-3 .. 1e4."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n):
        d = _vec(rng)
        if kind == 'spheres':
            o = _vec(rng)
            obj = core.Sphere.moving(o, o + d, float(10.0 ** rng.uniform(-3, 3)), MAT)
            d = obj.center.direction  # (o + d) - o: what the object holds
        elif kind == 'quads':
            u, v = _vec(rng), _vec(rng)
            obj = core.quad(_vec(rng), u, v, MAT)
        else:
            a = _vec(rng)
            obj = core.triangle(a, a + _vec(rng), a + _vec(rng), MAT)
        out[i] = (obj, d)
    return {kind: out}


def check_input(kind, tracks):
    """pose_check's in.f64: the track record followed by the row floats the kernel reads."""
    rec = pose.track_records(tracks)[STORAGE_POS[kind]][1]
    objs = [tracks[kind][i][0] for i in sorted(tracks[kind])]
    if kind == 'spheres':
        extra = np.array([[f32(o.radius)] for o in objs], np.float64)
    elif kind == 'quads':
        extra = np.array([o.u.to_list() + o.v.to_list() for o in objs], np.float64).astype(f32).astype(np.float64)
    else:
        return rec
    return np.concatenate([rec, extra], axis=1)


def expected(kind, tracks, t):
    """pose_check's out.f32 from the Python definition: the changed row floats of
    ``posed_records`` and the box of its build records by update_helpers' rules."""
    _, rows, build = pose.posed_records(tracks, t)[STORAGE_POS[kind]]
    mn, mx = BOX_RULE[kind](build)
    return np.concatenate([rows[:, CHANGED[kind]], mn, mx], axis=1).astype(f32)


def rest_records(tracks):
    """update_records of the tracked objects as they are (the rest rows), per kind in storage order."""
    objs = [[tracks.get(k, {})[i][0] for i in sorted(tracks.get(k, {}))] for k in KINDS]
    return scene_compiler.update_records(*objs)


# ------------------------------------------------------------------ the test scenes
_worlds = {}


def scene_prims(name, width=None):
    """The primitive objects of a test scene in compile order, {'spheres': [...], 'quads': [...], 'triangles': [...]},
    whose compiled rows are the fixture's. Built scenes give their world's objects; a captured fixture gives
    stationary spheres made of its f32 arrays (its quads and triangles are not remade: their normals were formed from
    float64 vectors the arrays no longer hold)."""
    key = (name, width)
    if key in _worlds:
        return _worlds[key]
    sa = ph.fixture(name, width)
    if name in ph.BUILT:
        random.seed(1234)
        if name == 'coverage':
            from coverage_scene import coverage_scene
            sc = coverage_scene(width)
        else:
            from ptmi import scenes
            sc = scenes.SCENES[name]()
        out = scene_compiler.compile_scene(sc.world)
        prims = {'spheres': out[2], 'quads': out[5], 'triangles': out[8]}
    else:
        prims = {'spheres': [core.Sphere.stationary(core.vec3(*(float(x) for x in row[:3])), float(row[3]), MAT)
                             for row in sa.sphere_data], 'quads': [], 'triangles': []}
    (sr, _), (qr, _), (tr, _) = scene_compiler.update_records(prims['spheres'], prims['quads'], prims['triangles'])
    assert sr.tobytes() == np.asarray(sa.sphere_data, f32).tobytes()
    if prims['quads']:
        assert qr.tobytes() == sd.pack_quads(sa.quads).tobytes()
    if prims['triangles']:
        assert tr.tobytes() == sd.pack_tris(sa.tris).tobytes()
    _worlds[key] = prims
    return prims


def scene_tracks(name, width=None, spheres=(), quads=(), triangles=(), seed=0, reach=1.0):
    """Tracks of a test scene: the named primitives (reference indices) each with a random displacement of up to
    ``reach`` per axis; a sphere that already moves (Sphere.moving) keeps its own."""
    prims = scene_prims(name, width)
    rng = np.random.default_rng(seed)
    tracks = {k: {} for k in KINDS}
    for kind, idx in zip(KINDS, (spheres, quads, triangles)):
        for i in idx:
            obj = prims[kind][int(i)]
            d = core.vec3(*rng.uniform(-reach, reach, 3))
            if kind == 'spheres' and not pose._is_zero(obj.center.direction):
                d = obj.center.direction
            tracks[kind][int(i)] = (obj, d)
    return tracks


def small_world(kind):
    """Worlds the pose tests build themselves, with their objects at hand: 'one_sphere' (no internal node),
    'two_primitives' (a sphere and a quad: one internal node), 'zero' (a moving sphere, a quad with Q.x = -0.0, a
    triangle and two more spheres). Returns (SceneArrays, primitive lists in compile order)."""
    key = ('small', kind)
    if key not in _worlds:
        random.seed(7)
        w = core.hittable_list()
        if kind == 'zero':
            w.add(core.Sphere.moving(core.vec3(0, 0.5, -1), core.vec3(0.5, 0.75, -1), 0.5, MAT))
            w.add(core.quad(core.vec3(-0.0, -0.5, -3), core.vec3(0, 0, 4), core.vec3(0, 2, 0), MAT))
            w.add(core.triangle(core.vec3(1, 0, 0), core.vec3(2, 0, 0.5), core.vec3(1.5, 1, 0), MAT))
            w.add(core.Sphere.stationary(core.vec3(3, 0, -2), 0.25, MAT))
            w.add(core.Sphere.stationary(core.vec3(-3, 1, -2), 0.75, MAT))
        else:
            w.add(core.Sphere.stationary(core.vec3(0, 0, -1), 0.5, MAT))
            if kind == 'two_primitives':
                w.add(core.quad(core.vec3(-2, -0.5, -3), core.vec3(4, 0, 0), core.vec3(0, 0, 4), MAT))
        out = scene_compiler.compile_scene(w)
        _worlds[key] = (sd.compile_world(w), {'spheres': out[2], 'quads': out[5], 'triangles': out[8]})
    return _worlds[key]


def device_image(ds):
    """What the device holds, as numpy arrays in the layout's shapes, and the view's host fields."""
    lay = ds.layout

    def host(t, like):
        like = np.asarray(like)
        return t.cpu().numpy().view(f32)[:like.size].reshape(like.shape).copy()

    img = {'nodes': host(ds.t_nodes, lay.nodes), 'ref_nodes': host(ds.t_ref_nodes, lay.ref_nodes),
           'spheres': host(ds.t_spheres, lay.spheres), 'quads': host(ds.t_quads, lay.quads),
           'tris': host(ds.t_tris, lay.tris), 'mats': host(ds.t_mats, lay.mats),
           'texels': ds.t_texels.cpu().numpy().copy()}
    img['view_root'] = np.array(list(ds.view.root_min) + list(ds.view.root_max), f32)
    img['shell'] = int(ds.view.shell)
    return img


def images_differ(a, b, keys=None):
    """The members in which two device images differ (bytes)."""
    return [k for k in (keys or a) if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def as_edits(records):
    """posed_records' tuple as update_helpers.refit's dict."""
    return {k: r for k, r in zip(KINDS, records) if r is not None}


def oracle_blurred(scene, variant, window, tracks, shutter, slice_spp, s_begin, s_count, traversal='stack',
                   seed=0, max_depth=50):
    """The blurred image by the CPU oracle: every slice rendered on the numpy-refit arrays of its pose
    (update_helpers.refit of posed_records) and added into one accumulator. ``scene``: (SceneArrays of the rest
    scene, camera upload dict, background), parity_helpers.scene_inputs' triple. Returns (accum, summed counters)."""
    import oracle
    sa, cam, bg = scene
    W, H = cam['width'], cam['height']
    fr = oracle.make_frame(cam, bg, max_depth, seed, W, H, traversal)
    acc = np.zeros((H, W, 3), f32)
    total = {}
    for _, t, b, n in pose.slice_times(s_begin, s_count, slice_spp, shutter):
        posed = uh.refit(sa, as_edits(pose.posed_records(tracks, t)))
        stats = oracle.render(oracle.OracleScene(posed), fr, variant, acc, window, b, n, 0)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    return acc, total
