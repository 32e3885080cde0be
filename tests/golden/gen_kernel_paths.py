#!/usr/bin/env python3
"""Path fixtures from the reference's own kernel text: kernel_paths_<scene>.npz.

TEST INFRASTRUCTURE ONLY. Run where the reference is present (never at test
time, never on a GPU machine): python tests/golden/gen_kernel_paths.py [scene ...]

For each scene below the world is built from the reference's core classes and
compiled with its own compile_scene / compile_bvh (as gen_fixtures.py does),
then uploaded into the reference's `fields` by the reference's own upload code
(renderer.py:102-247: TaichiRenderer._upload_to_gpu and _upload_camera run on
a plain namespace), and the reference's kernels.py runs over ti_shim.py:

  * megakernel: kernels.render_sample(), once per sample (renderer.py:405-409);
    a path's colour is what its trace_ray returned.
  * wavefront: generate_camera_rays, then up to max_depth waves of
    intersect_rays, shade_miss_rays, reset_next_ray_count, shade_and_scatter,
    swap_ray_buffers while active_ray_count > 0 (the loop of
    renderer.py:305-334, restated in _run_wf), one sample per run. The kernels
    add a path's contributions to accum_buffer at different waves; every add
    is recorded per path, in the order made, and the path's colour is their
    f32 sum from zero in that order, ((0 + c1) + c2) + ..., which is how the
    oracle's variant 1 sums a path before the path is added to the pixel.

Two patches are made to the compiled arrays before the upload, because the
reference's compiler cannot emit them (both said again where they are made):
material type 4 (isotropic) on the primitives a scene names, and
the hand-built linear BVH of the `chainx` scene (tests/edge_scenes.py's
construction, restated in _linear_bvh). The image texture is the reference's
earthmap.jpg through its own loader (core/texture.py image_texture); the
fixture names it ('earthmap') and the tests take the committed decoded copy.

What a fixture holds, per variant (prefix mk_ / wf_), for the P = spp*H*W
paths in (sample, row, column) order: color (P,3) f32, nseg, medium (exit
traversals), rr, cap (flags), draws, seg_off (P+1) and the flat per-segment
records seg_rng_n / seg_hit / seg_t / seg_type / seg_idx / seg_kind (the
fields of or_seg, pt_oracle.h); coverage_<case> counts of paths from the
shim's own branch counters (kernels.py line, outcome); control_<switch> /
invariant_c_mod colours of reruns with one ti_shim switch flipped. Plus the
scene arrays under gen_fixtures.py's names, the f32 camera upload (cam_*),
seed, max_depth, bg, spp, traversal and the image names.

Only data is written. Measured: the whole regeneration takes 55 s on one
core, 40 s of it the `materials` scene with its four switch reruns (the log
printed per scene has the seconds); a second run reproduces the files
byte for byte (_savez fixes the archive's member times).
"""
import json
import os
import random
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, '..', '..'))
REF_SRC = '/root/reference/src'
REF_TI = os.path.join(REF_SRC, 'render_server', 'taichi_renderer')
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ti_shim  # noqa: E402

SEED = 7
KINDS = {'surface': 0, 'medium_scatter': 1, 'passthrough': 2, 'fallback': 3, 'miss': 4}  # oracle.SEG_KINDS
W, H = 16, 12

# coverage case -> minimum number of paths, in at least one fixture, for each
# variant it applies to (tests/test_kernel_paths.py holds the same table).
# 20 / 20 / 10 are set by the issue; 5 elsewhere, the controls' own bound.
COVERAGE_MIN = dict(
    {f'mat{m}_on_{p}': 5 for m in range(5) for p in ('sphere', 'triangle', 'quad')},
    metal_fuzz_absorb=20, dielectric_tir_draw=20, front_face_true=5, front_face_false=5,
    tex_solid=5, tex_checker_even=5, tex_checker_odd=5, tex_noise_scale_a=5, tex_noise_scale_b=5,
    tex_image_sphere=5, tex_image_not_sphere=5,
    medium_scatter_sphere=10, medium_scatter_box=10, medium_scatter_fog=10, medium_passthrough=10,
    medium_fallback=10, medium_scatter_then_hit_inside=10,
    rr_kill=5, rr_survive=5, depth_cap=5, defocus_on=5, defocus_off=5,
    stack_overflow_drop=5, coincident_tie=5, stackless=5, sah_tree=5,
)
WF_ONLY = dict(wf_unnormalised_dir=5, wf_passthrough_wave=10, wf_rr_kill=5)


# ---------------------------------------------------------------- scenes
def _ref():
    from core import Sphere, camera, hittable_list  # noqa: E402
    from core.constant_medium import constant_medium
    from core.material import dielectric, diffuse_light, lambertian, metal
    from core.quad import quad
    from core.texture import checker_texture, image_texture, noise_texture
    from core.triangle import triangle
    from util import color, point3, vec3
    return types.SimpleNamespace(**locals())


def _cam(R, lookfrom, lookat, vfov=40.0, defocus=0.0, focus=10.0):
    cam = R.camera()
    cam.aspect_ratio = W / H
    cam.img_width = W
    cam.samples_per_pixel = 1
    cam.vfov = vfov
    cam.lookfrom = R.point3(*lookfrom)
    cam.lookat = R.point3(*lookat)
    cam.vup = R.vec3(0, 1, 0)
    cam.defocus_angle = defocus
    cam.focus_distance = focus
    return cam


def _box(R, lo, hi, mat):
    """Six quads around [lo, hi]."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    dx, dy, dz = R.vec3(x1 - x0, 0, 0), R.vec3(0, y1 - y0, 0), R.vec3(0, 0, z1 - z0)
    b = R.hittable_list()
    b.add(R.quad(R.point3(x0, y0, z1), dx, dy, mat))
    b.add(R.quad(R.point3(x1, y0, z1), -dz, dy, mat))
    b.add(R.quad(R.point3(x1, y0, z0), -dx, dy, mat))
    b.add(R.quad(R.point3(x0, y0, z0), dz, dy, mat))
    b.add(R.quad(R.point3(x0, y1, z1), dx, -dz, mat))
    b.add(R.quad(R.point3(x0, y0, z0), dx, dz, mat))
    return b


def scene_materials(R):
    """Every material on every primitive type, the textures, fuzz-1 metal, a
    sphere of ir 1/1.5 (total internal reflection from outside), defocus."""
    c, p3, v3 = R.color, R.point3, R.vec3
    lam, met, die, lit = R.lambertian, R.metal, R.dielectric, R.diffuse_light
    w = R.hittable_list()
    iso = []   # (type name, index within type) to patch to material 4
    S = lambda x, y, z, r, m: w.add(R.Sphere.stationary(p3(x, y, z), r, m))
    # quads 0-1: fuzz-1 metal floor, checker back wall
    w.add(R.quad(p3(-7, 0, -5), v3(14, 0, 0), v3(0, 0, 13), met(c(0.85, 0.85, 0.8), 1.0)))
    w.add(R.quad(p3(-7, 0, -4), v3(14, 0, 0), v3(0, 7, 0),
                 lam.from_texture(R.checker_texture.from_colors(0.9, c(0.2, 0.3, 0.1), c(0.9, 0.9, 0.9)))))
    # spheres 0-4, the row
    S(-2.7, 0.6, 0, 0.6, lam.from_texture(R.noise_texture(4.0)))
    S(-1.35, 0.6, 0, 0.6, met(c(0.8, 0.6, 0.2), 1.0))
    S(0.0, 0.6, 0, 0.6, die(1.0 / 1.5))
    S(1.35, 0.6, 0, 0.6, die(1.5))
    S(2.7, 0.6, 0, 0.6, lam.from_texture(R.noise_texture(9.0)))
    iso.append(('sphere', 4))
    # spheres 5-8, above
    S(0.0, 2.9, -0.5, 0.55, lit.from_color(c(5, 5, 5)))
    S(-1.6, 2.1, -0.5, 0.55, lam.from_texture(R.image_texture(os.path.join(REF_SRC, 'assets/images/earthmap.jpg'))))
    S(1.6, 2.1, -0.5, 0.55, lam.from_texture(R.checker_texture.from_colors(0.3, c(0.8, 0.1, 0.1), c(0.1, 0.1, 0.8))))
    S(3.0, 2.2, -1.0, 0.5, lam.from_color(c(0.3, 0.7, 0.4)))
    # quads 2-6: upright panels in front
    mats = [lam.from_texture(R.image_texture(os.path.join(REF_SRC, 'assets/images/earthmap.jpg'))),
            met(c(0.7, 0.7, 0.9), 0.3), die(1.5), lit.from_color(c(3, 2, 1)), lam.from_color(c(0.6, 0.5, 0.8))]
    for k, m in enumerate(mats):
        w.add(R.quad(p3(-3.3 + 1.4 * k, 0.0, 2.2), v3(1.0, 0, 0), v3(0, 0.9, 0.15), m))
    iso.append(('quad', 6))
    # triangles 0-4, behind and above
    mats = [lam.from_color(c(0.8, 0.4, 0.1)), met(c(0.9, 0.9, 0.9), 1.0), die(1.5), lit.from_color(c(2, 3, 4)),
            lam.from_texture(R.checker_texture.from_colors(0.4, c(0.9, 0.8, 0.1), c(0.1, 0.5, 0.5)))]
    for k, m in enumerate(mats):
        x = -3.4 + 1.45 * k
        w.add(R.triangle(p3(x, 3.3, -1.6), p3(x + 1.3, 3.3, -1.6), p3(x + 0.65, 4.5, -2.0), m))
    iso.append(('triangle', 4))
    return dict(world=w, cam=_cam(R, (0, 2.6, 8.0), (0, 1.7, 0), 42.0, defocus=0.8, focus=8.0),
                bg=(0.7, 0.8, 1.0), max_depth=50, spp=8, iso=iso)


def _media_world(R):
    c, p3, v3 = R.color, R.point3, R.vec3
    lam = R.lambertian
    w = R.hittable_list()
    grey = lam.from_color(c(0.5, 0.5, 0.5))
    # sphere 0: the enclosing fog; 1: a smoke sphere; quads 0-5: a smoke box
    w.add(R.constant_medium.from_color(R.Sphere.stationary(p3(0, 1, 0), 3.6, grey), c(0.9, 0.9, 0.9), 0.12))
    w.add(R.constant_medium.from_color(R.Sphere.stationary(p3(-1.3, 1.0, 0.3), 0.9, grey), c(0.2, 0.4, 0.9), 1.6))
    w.add(R.constant_medium.from_color(_box(R, (0.5, 0.1, -0.6), (2.1, 1.7, 0.9), grey), c(0.9, 0.5, 0.2), 1.3))
    # spheres 2-3, quad 6
    w.add(R.Sphere.stationary(p3(0.0, 2.3, -0.8), 0.6, R.diffuse_light.from_color(c(4, 4, 4))))
    w.add(R.Sphere.stationary(p3(-0.2, 0.5, 1.6), 0.5, lam.from_color(c(0.7, 0.3, 0.3))))
    w.add(R.quad(p3(-8, 0, -8), v3(16, 0, 0), v3(0, 0, 16), lam.from_color(c(0.6, 0.6, 0.6))))
    return w


def scene_media(R):
    """Constant media on a sphere, on a six-quad box and as a fog sphere around
    the rest, seen from outside the fog; no defocus."""
    return dict(world=_media_world(R), cam=_cam(R, (0, 2.0, 9.0), (0, 1.0, 0), 42.0), bg=(0.7, 0.8, 1.0),
                max_depth=50, spp=3, iso=[])


def scene_depthcap(R):
    """The media world at max_depth 3: passthroughs use up iterations / waves."""
    return dict(world=_media_world(R), cam=_cam(R, (0, 2.0, 9.0), (0, 1.0, 0), 42.0), bg=(0.7, 0.8, 1.0),
                max_depth=3, spp=2, iso=[])


def scene_stackless(R):
    """The media world under USE_STACKLESS_TRAVERSAL = True (kernels.py:746)."""
    return dict(world=_media_world(R), cam=_cam(R, (0, 2.0, 9.0), (0, 1.0, 0), 42.0), bg=(0.7, 0.8, 1.0),
                max_depth=50, spp=1, iso=[], traversal='stackless')


def scene_coincident(R):
    """Pairs of coincident primitives (first found wins, Q16) over a floor."""
    c, p3, v3 = R.color, R.point3, R.vec3
    w = R.hittable_list()
    w.add(R.Sphere.stationary(p3(-1.2, 1.0, 0), 1.0, R.lambertian.from_color(c(0.9, 0.1, 0.1))))
    w.add(R.Sphere.stationary(p3(-1.2, 1.0, 0), 1.0, R.metal(c(0.9, 0.9, 0.9), 0.0)))
    w.add(R.quad(p3(0.4, 0.0, 0.0), v3(1.8, 0, 0), v3(0, 2.0, 0), R.diffuse_light.from_color(c(2, 2, 2))))
    w.add(R.quad(p3(0.4, 0.0, 0.0), v3(1.8, 0, 0), v3(0, 2.0, 0), R.lambertian.from_color(c(0.1, 0.8, 0.1))))
    w.add(R.quad(p3(-8, 0, -8), v3(16, 0, 0), v3(0, 0, 16), R.lambertian.from_color(c(0.6, 0.6, 0.6))))
    return dict(world=w, cam=_cam(R, (0, 1.5, 6.0), (0, 1.0, 0), 40.0), bg=(0.7, 0.8, 1.0), max_depth=50, spp=2,
                iso=[])


CHAIN_N = 70


def scene_chainx(R):
    """tests/edge_scenes.py's chainx<N> at N = 70 > 64: spheres in a row seen
    along -x under a linear BVH whose leaves are ordered far end first, so the
    64-entry stack drops pushes (kernels.py:719-740)."""
    c, p3 = R.color, R.point3
    w = R.hittable_list()
    n = CHAIN_N - 1
    for k in range(n):
        x = -4.0 + 8.0 * k / max(1, n - 1)
        m = R.metal(c(0.8, 0.8, 0.7), 0.1) if k % 3 == 0 else R.lambertian.from_color(c(0.2 + 0.6 * (k % 2), 0.5, 0.3))
        w.add(R.Sphere.stationary(p3(x, 0.3 * (k % 4), -0.5 * (k % 5)), 0.35, m))
    w.add(R.Sphere.stationary(p3(0, -100.4, 0), 100.0, R.lambertian.from_color(c(0.5, 0.5, 0.5))))
    return dict(world=w, cam=_cam(R, (12, 0.8, 0.5), (-4, 0, -1), 40.0), bg=(0.6, 0.7, 0.9), max_depth=50, spp=2,
                iso=[], linear_bvh=True)


def _linear_bvh(sphere_data):
    """The chainx construction: a linear BVH in the reference's flattened
    layout (preorder, internal node of leaf k at 2k, leaf at 2k + 1, boxes the
    unions of the children's), leaves by x ascending, the ground sphere last."""
    sd = np.asarray(sphere_data, np.float32)
    ns = sd.shape[0]
    small = sd[:, 3] < 50
    order = np.concatenate([np.flatnonzero(small)[np.argsort(sd[small, 0], kind='stable')], np.flatnonzero(~small)])
    lo, hi = sd[:, :3] - sd[:, 3:4], sd[:, :3] + sd[:, 3:4]
    n = 2 * ns - 1
    bmin, bmax = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    left, right, parent, ptype, pidx = (np.full(n, -1, np.int32) for _ in range(5))
    for k in range(ns - 1):
        node, leaf = 2 * k, 2 * k + 1
        left[node], right[node] = leaf, node + 2
        parent[leaf] = parent[node + 2] = node
        ptype[leaf], pidx[leaf] = 0, order[k]
        bmin[leaf], bmax[leaf] = lo[order[k]], hi[order[k]]
    ptype[n - 1], pidx[n - 1] = 0, order[ns - 1]
    bmin[n - 1], bmax[n - 1] = lo[order[ns - 1]], hi[order[ns - 1]]
    for k in range(ns - 2, -1, -1):
        node = 2 * k
        bmin[node] = np.minimum(bmin[left[node]], bmin[right[node]])
        bmax[node] = np.maximum(bmax[left[node]], bmax[right[node]])
    return {'bvh_bbox_min': bmin, 'bvh_bbox_max': bmax, 'bvh_left_child': left, 'bvh_right_child': right,
            'bvh_parent': parent, 'bvh_prim_type': ptype, 'bvh_prim_idx': pidx, 'num_bvh_nodes': n}


SCENES = {'materials': scene_materials, 'media': scene_media, 'depthcap': scene_depthcap,
          'stackless': scene_stackless, 'coincident': scene_coincident, 'chainx': scene_chainx}
CONTROL_SCENE = 'materials'


# ---------------------------------------------------------------- recording
class PathRec:
    def __init__(self, pixel, sample):
        self.pixel, self.sample = pixel, sample
        self.segs, self.medium, self.events, self.adds = [], 0, set(), []
        self.color, self.rr, self.cap = None, False, False


class Recorder:
    """Names the running path for the shim (random stream, branch events) and
    collects, per path, what the reference's functions returned."""

    def __init__(self, L, width):
        self.L, self.width = L, width
        self.paths, self.cur, self.sample, self.in_acm = {}, None, 0, False
        k = L.kernels
        trav, acm, scat, trace = k.traverse_bvh, k.apply_constant_medium, k.scatter, k.trace_ray
        rec = self

        def traverse_bvh(o, d, tmin, tmax):
            r = trav(o, d, tmin, tmax)
            p = rec.cur
            if rec.in_acm:
                p.medium += 1
            else:
                hit = bool(r[0])
                p.segs.append({'rng_n': L.state.streams.draws(p.pixel, p.sample), 'hit': hit,
                               't': r[1] if hit else np.float32(0.0), 'type': int(r[4]) if hit else -1,
                               'idx': int(r[5]) if hit else -1, 'acm': None, 'scatter': False})
            return r

        def apply_constant_medium(*a):
            rec.in_acm = True
            r = acm(*a)
            rec.in_acm = False
            rec.cur.segs[-1]['acm'] = bool(r[0])
            return r

        def scatter(*a):
            rec.cur.segs[-1]['scatter'] = True
            return scat(*a)

        def trace_ray(o, d):
            r = trace(o, d)
            p = rec.cur
            p.color, p.rr, p.cap = r[0], bool(r[2]), bool(r[4])
            return r

        k.traverse_bvh, k.apply_constant_medium, k.scatter, k.trace_ray = traverse_bvh, apply_constant_medium, scatter, trace_ray
        L.state.hook = self.hook

    def select(self, pixel):
        key = (int(pixel), self.sample)
        p = self.paths.get(key)
        if p is None:
            p = self.paths[key] = PathRec(*key)
        self.cur = p
        self.L.state.streams.set_path(*key)
        self.L.state.events = p.events

    def hook(self, name, v):
        f = self.L.fields
        if name in ('render_sample', 'generate_camera_rays'):
            self.select(v['py'] * self.width + v['px'])
        elif name in ('intersect_rays', 'shade_miss_rays', 'shade_and_scatter'):
            self.select(f.ray_pixel_index[v['i']])


def _kind(s):
    if not s['hit']:
        return KINDS['miss']
    if s['acm'] is None:
        return KINDS['surface']
    if s['acm']:
        return KINDS['medium_scatter']
    return KINDS['fallback'] if s['scatter'] else KINDS['passthrough']


# ---------------------------------------------------------------- one run
def _load_renderer(L):
    """The reference's renderer.py as a module over the loaded fields/kernels
    (its preview window stubbed), for its upload code."""
    pv = types.ModuleType('render_server.taichi_renderer.preview')
    pv.LivePreview = None
    sys.modules[pv.__name__] = pv
    path = os.path.join(REF_TI, 'renderer.py')
    mod = types.ModuleType('render_server.taichi_renderer.renderer')
    mod.__package__ = 'render_server.taichi_renderer'
    mod.__file__ = path
    with open(path) as f:
        exec(compile(f.read(), path, 'exec'), mod.__dict__)
    return mod


def _compile(R, spec):
    from core.perlin import perlin
    from render_server.taichi_renderer import bvh_compiler, scene_compiler
    cam = spec['cam']
    cam.initialize()
    per = perlin()   # renderer.py:78-80: after the scene, before compile_scene
    comp = scene_compiler.compile_scene(spec['world'])
    geom, mats, spheres, qgeom, qmats, quads, tgeom, tmats, tris, _reg, img_list = comp
    if spec.get('linear_bvh'):
        bvh = _linear_bvh(geom['sphere_data'][:geom['num_spheres']])   # patch: the hand-built chainx tree
    else:
        bvh = bvh_compiler.compile_bvh(spec['world'], spheres, quads, tris)
    for tname, i in spec['iso']:   # patch: material 4 is never emitted by compile_scene (Q23)
        {'sphere': mats, 'quad': qmats, 'triangle': tmats}[tname]['material_type'][i] = 4
    return dict(cam=cam, per=per, geom=geom, mats=mats, qgeom=qgeom, qmats=qmats, tgeom=tgeom, tmats=tmats,
                bvh=bvh, img_list=img_list)


def _upload(L, ren, comp, spec):
    f = L.fields
    cam = comp['cam']
    f.allocate_dynamic_fields(cam.img_width, cam.img_height)
    f.allocate_wavefront_fields(cam.img_width, cam.img_height, spec['max_depth'])
    f.init_perlin_noise(comp['per'])
    me = types.SimpleNamespace(cam=cam, background_color=spec['bg'], max_depth=spec['max_depth'])
    T = ren.TaichiRenderer
    T._upload_to_gpu(me, comp['geom'], comp['mats'], comp['qgeom'], comp['qmats'], comp['tgeom'], comp['tmats'],
                     comp['bvh'], comp['img_list'])
    T._upload_camera(me)


def _run_mk(L, rec, spp):
    for s in range(spp):
        rec.sample = s
        L.kernels.render_sample()


def _run_wf(L, rec, spp, max_depth, width, height, info):
    f, k = L.fields, L.kernels
    for s in range(spp):
        rec.sample = s
        k.generate_camera_rays(width, height)
        d = f.ray_directions.arr[:width * height].astype(np.float64)
        info['unnormalised'] = info.get('unnormalised', 0) + int(
            np.sum(np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0) > 1e-3))
        for _bounce in range(max_depth):
            if f.active_ray_count[None] == 0:
                break
            k.intersect_rays()
            k.shade_miss_rays(width)
            k.reset_next_ray_count()
            k.shade_and_scatter(width)
            k.swap_ray_buffers()
        for i in range(int(f.active_ray_count[None])):   # rays the wave budget left behind (Q14)
            rec.paths[(int(f.ray_pixel_index[i]), s)].cap = True


class _RecField(ti_shim.Field):
    """accum_buffer that also tells the running path what was added to it."""
    rec = None

    def aug(self, i, op, v):
        self.rec.cur.adds.append(v)
        super().aug(i, op, v)

    def atomic_add(self, i, v):
        self.rec.cur.adds.append(v)
        return super().atomic_add(i, v)


def run(R_factory, name, variant, switches=()):
    import oracle
    L = ti_shim.load(REF_TI, switches, oracle.rng_probe, oracle.math_probe, SEED)
    ren = _load_renderer(L)
    random.seed(1234)
    R = R_factory()
    spec = SCENES[name](R)
    comp = _compile(R, spec)
    _upload(L, ren, comp, spec)
    if spec.get('traversal') == 'stackless':
        L.kernels.USE_STACKLESS_TRAVERSAL = True
    rec = Recorder(L, W)
    L.fields.accum_buffer.__class__ = _RecField
    L.fields.accum_buffer.rec = rec
    info = {}
    if variant == 'mk':
        _run_mk(L, rec, spec['spp'])
    else:
        _run_wf(L, rec, spec['spp'], spec['max_depth'], W, H, info)
    return spec, comp, rec, info, L


def _ev(p, line, *outcome):
    return (('kernels', line),) + outcome in p.events


def _coverage(spec, comp, rec, variant, info):
    mt = {0: comp['mats']['material_type'], 1: comp['tmats']['material_type'], 2: comp['qmats']['material_type']}
    tex = {0: comp['mats'], 1: comp['tmats'], 2: comp['qmats']}
    pname = {0: 'sphere', 1: 'triangle', 2: 'quad'}
    noise_scales = sorted({float(tex[t]['texture_scale'][i]) for t in tex
                           for i in range(len(tex[t]['texture_type'])) if tex[t]['texture_type'][i] == 3})
    cov = {k: 0 for k in list(COVERAGE_MIN) + list(WF_ONLY)}
    md = spec['max_depth']
    for p in rec.paths.values():
        got = set()
        kinds = [_kind(s) for s in p.segs]
        for s, kd in zip(p.segs, kinds):
            if kd in (KINDS['surface'], KINDS['fallback']):
                got.add(f"mat{int(mt[s['type']][s['idx']])}_on_{pname[s['type']]}")
                tr = tex[s['type']]
                if tr['texture_type'][s['idx']] == 3 and mt[s['type']][s['idx']] in (0, 4):
                    k = noise_scales.index(float(tr['texture_scale'][s['idx']]))
                    if k < 2:
                        got.add('tex_noise_scale_' + 'ab'[k])
            if kd == KINDS['medium_scatter']:
                if s['type'] == 2:
                    got.add('medium_scatter_box')
                elif s['type'] == 0:
                    got.add('medium_scatter_fog' if comp['geom']['sphere_data'][s['idx']][3] > 2 else 'medium_scatter_sphere')
            if kd == KINDS['passthrough']:
                got.add('medium_passthrough')
                if variant == 'wf':
                    got.add('wf_passthrough_wave')
            if kd == KINDS['fallback']:
                got.add('medium_fallback')
        for a, b in zip(kinds, kinds[1:]):
            if a == KINDS['medium_scatter'] and b == KINDS['fallback']:
                got.add('medium_scatter_then_hit_inside')
        flags = {'metal_fuzz_absorb': _ev(p, 869, False),
                 'dielectric_tir_draw': _ev(p, 894, True, True) or _ev(p, 894, True, False),
                 'front_face_true': _ev(p, 884, True), 'front_face_false': _ev(p, 884, False),
                 'tex_solid': _ev(p, 961, True), 'tex_checker_even': _ev(p, 972, True),
                 'tex_checker_odd': _ev(p, 972, False), 'tex_image_sphere': _ev(p, 978, True),
                 'tex_image_not_sphere': _ev(p, 978, False),
                 'defocus_on': _ev(p, 194, True), 'defocus_off': _ev(p, 194, False),
                 'stack_overflow_drop': any(_ev(p, ln, False) for ln in (719, 722, 727, 730)),
                 'coincident_tie': _ev(p, 691, True, False) or _ev(p, 561, True, False),
                 'stackless': _ev(p, 541, True) or _ev(p, 541, False),
                 'sah_tree': not spec.get('linear_bvh') and len(p.segs) > 0,
                 'depth_cap': p.cap}
        if variant == 'mk':
            flags['rr_kill'] = _ev(p, 1150, True)
            flags['rr_survive'] = _ev(p, 1150, False)
        else:
            flags['rr_kill'] = flags['wf_rr_kill'] = _ev(p, 1388, True)
            flags['rr_survive'] = _ev(p, 1388, False)
        got |= {k for k, v in flags.items() if v}
        for k in got:
            cov[k] += 1
    if variant == 'wf':
        cov['wf_unnormalised_dir'] = info.get('unnormalised', 0)
    return cov


def _finish(spec, rec, variant):
    """Per-path arrays in (sample, row, column) order."""
    spp, md = spec['spp'], spec['max_depth']
    P = spp * H * W
    out = {'color': np.zeros((P, 3), np.float32), 'nseg': np.zeros(P, np.int32), 'medium': np.zeros(P, np.int32),
           'rr': np.zeros(P, np.uint8), 'cap': np.zeros(P, np.uint8), 'draws': np.zeros(P, np.uint32),
           'seg_off': np.zeros(P + 1, np.int32)}
    segs = []
    for s in range(spp):
        for pix in range(H * W):
            q = s * H * W + pix
            p = rec.paths[(pix, s)]
            kinds = [_kind(x) for x in p.segs]
            if variant == 'mk':
                color = p.color
                rr = p.rr
                # the depth loop ran out on a passthrough: the reference's flag stays False (kernels.py:1054)
                cap = p.cap or (len(p.segs) == md and kinds[-1] == KINDS['passthrough'])
            else:
                color = ti_shim.vec((0.0, 0.0, 0.0))
                for a in p.adds:
                    color = ti_shim.binop('+', color, a)
                rr = _ev(p, 1388, True)
                cap = p.cap or _ev(p, 1383, False)   # new_depth >= max_depth, or no wave left (_run_wf)
            out['color'][q] = color.c
            out['nseg'][q], out['medium'][q], out['rr'][q], out['cap'][q] = len(p.segs), p.medium, rr, cap
            out['draws'][q] = rec.L.state.streams.draws(pix, s)
            out['seg_off'][q + 1] = out['seg_off'][q] + len(p.segs)
            for x, kd in zip(p.segs, kinds):
                segs.append((x['rng_n'], int(x['hit']), x['t'], x['type'], x['idx'], kd))
    out['seg_rng_n'] = np.array([x[0] for x in segs], np.uint32)
    out['seg_hit'] = np.array([x[1] for x in segs], np.int32)
    out['seg_t'] = np.array([x[2] for x in segs], np.float32)
    out['seg_type'] = np.array([x[3] for x in segs], np.int32)
    out['seg_idx'] = np.array([x[4] for x in segs], np.int32)
    out['seg_kind'] = np.array([x[5] for x in segs], np.int32)
    return out


def _scene_arrays(comp):
    """The uploaded arrays under gen_fixtures.py's names (ptmi.scene_data.SceneArrays.from_npz)."""
    arrs = {}
    ns = comp['geom']['num_spheres']
    arrs['sph_sphere_data'] = np.asarray(comp['geom']['sphere_data'][:ns], np.float32).reshape(ns, 4)
    for pre, m in (('sphm_', comp['mats']), ('quadm_', comp['qmats']), ('trim_', comp['tmats'])):
        for k, x in m.items():
            arrs[pre + k] = np.asarray(x)
    for g in (comp['qgeom'], comp['tgeom'], comp['bvh']):
        for k, x in g.items():
            if isinstance(x, np.ndarray):
                arrs[k] = x
    per = comp['per']
    arrs['perlin_randvec'] = np.array([[p.x, p.y, p.z] for p in per.randvec], dtype=np.float32)
    for k in ('perm_x', 'perm_y', 'perm_z'):
        arrs['perlin_' + k] = np.array(getattr(per, k), dtype=np.int32)
    return arrs


def _camera(L, cam):
    f = L.fields
    out = {'cam_' + k: getattr(f, 'cam_' + n).arr.copy() for k, n in
           (('center', 'center'), ('pixel00', 'pixel00'), ('delta_u', 'delta_u'), ('delta_v', 'delta_v'),
            ('defocus_u', 'defocus_disk_u'), ('defocus_v', 'defocus_disk_v'))}
    out['cam_defocus_angle'] = np.float32(f.cam_defocus_angle[None])
    out['cam_size'] = np.array([cam.img_width, cam.img_height], np.int32)
    return out


def generate(R_factory, name):
    t0 = time.time()
    data, log, weak = {}, {}, []
    for variant in ('mk', 'wf'):
        spec, comp, rec, info, L = run(R_factory, name, variant)
        res = _finish(spec, rec, variant)
        cov = _coverage(spec, comp, rec, variant, info)
        cov['depth_cap'] = int(res['cap'].sum())   # the flag as _finish completes it
        for k, x in res.items():
            data[f'{variant}_{k}'] = x
        for k, x in cov.items():
            data[f'{variant}_coverage_{k}'] = np.int64(x)
        log[variant] = {'paths': len(rec.paths), 'segments': int(res['nseg'].sum()), 'draws': int(res['draws'].sum()),
                        'coverage': {k: v for k, v in cov.items() if v}}
        if name == CONTROL_SCENE:
            for sw, row in ti_shim.SWITCHES.items():
                _s, _c, crec, _i, _L = run(R_factory, name, variant, (sw,))
                ccol = _finish(spec, crec, variant)['color']
                differ = int(np.sum(np.any(ccol.view(np.uint32) != res['color'].view(np.uint32), axis=1)))
                log[variant][f'differ_{sw}'] = differ
                if row['control']:
                    if differ < 5:
                        weak.append(f'{name} {variant}: control {sw} differs on {differ} paths only')
                    data[f'{variant}_control_{sw}'] = ccol
                else:
                    if differ:
                        weak.append(f'{name} {variant}: {sw} was expected to change nothing ({differ} paths)')
                    data[f'{variant}_invariant_{sw}'] = ccol
    data.update(_scene_arrays(comp))
    data.update(_camera(L, comp['cam']))
    data['seed'] = np.uint32(SEED)
    data['max_depth'] = np.int32(spec['max_depth'])
    data['spp'] = np.int32(spec['spp'])
    data['bg'] = np.asarray(L.fields.bg_color.arr, np.float32)
    data['traversal'] = np.array(spec.get('traversal', 'stack'))
    data['images'] = np.array(json.dumps(['earthmap'] * len(comp['img_list'])))
    data['upload'] = np.array('reference upload code (renderer.py:102-247) under the shim')
    log['seconds'] = round(time.time() - t0, 1)
    print(name, json.dumps(log, sort_keys=True), flush=True)
    assert not weak, '; '.join(weak)   # the scene is too weak: give it more such paths
    _savez(os.path.join(HERE, f'kernel_paths_{name}.npz'), data)
    return data


def _savez(path, data):
    """np.savez_compressed with fixed member times, so a second run reproduces the file byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', (1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def check_coverage(all_data):
    for variant in ('mk', 'wf'):
        table = dict(COVERAGE_MIN, **(WF_ONLY if variant == 'wf' else {}))
        for case, least in table.items():
            best = max(int(d[f'{variant}_coverage_{case}']) for d in all_data.values())
            assert best >= least, f'{variant}: {case} reached on {best} paths at most, needs {least}'


def main():
    from gen_fixtures import _install_stubs
    _install_stubs()
    os.chdir(REF_SRC)
    names = sys.argv[1:] or list(SCENES)
    t0 = time.time()
    for n in names:
        generate(_ref, n)
    all_data = {n: np.load(os.path.join(HERE, f'kernel_paths_{n}.npz')) for n in SCENES
                if os.path.exists(os.path.join(HERE, f'kernel_paths_{n}.npz'))}
    if set(all_data) == set(SCENES):
        check_coverage(all_data)
        print('coverage minimums hold')
    print(f'{time.time() - t0:.0f} s')


if __name__ == '__main__':
    main()
