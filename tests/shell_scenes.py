"""Scenes and render helpers of the enclosing-medium-shell tests (test
infrastructure only): a constant-medium sphere of radius R around two
Lambertian spheres, a metal sphere, a quad light and a triangle, all scaled
with R and within 0.42 R of the shell's centre (the origin), so that
scene_data.find_shell takes the sphere as the scene's shell.

What a path does at the shell depends on R: the exit search starts at
t_entry + 1e-4, which is t_entry itself once t_entry >= 2048 (half an f32 ulp
above 1e-4), so R = 5000 passes through (exit search, passthrough, escape
segment: the vol2 fog), while R = 100 and R = 1 find no exit past t_entry and
shade the shell as a surface (the fallback, kernels.py:1111-1119)."""
from __future__ import annotations

import random

import numpy as np

from ptmi import scene_data as sd
from ptmi.core import (Sphere, camera, color, constant_medium, dielectric, diffuse_light, hittable_list, lambertian,
                       metal, point3, quad, triangle, vec3)
from ptmi.scenes import _wrap

BG = (0.6, 0.7, 0.9)
WIDTH = 32
COUNTERS = ('segments', 'medium', 'paths', 'rr', 'depth_cap')

# camera name -> (lookfrom / s, lookat / s, vup, vfov) with s = R / 100
CAMERAS = {
    'inside': ((4, 6, 30), (0, 0, 0), (0, 1, 0), 50.0),   # 0.31 R from the centre: the gate passes
    'gate': ((0, 0, 80), (0, 0, 0), (0, 1, 0), 25.0),     # 0.8 R: the gate fails for the camera segment
    'pole+x': ((0, 0, 0), (1, 0, 0), (0, 1, 0), 0.01),    # from the centre along an axis: the leaf box's
    'pole-y': ((0, 0, 0), (0, -1, 0), (0, 0, 1), 0.01),   # face poles, direction components near 0 (Q15)
    'pole+z': ((0, 0, 0), (0, 0, 1), (0, 1, 0), 0.01),
}

_cache = {}


def shell_world(R, shell=True, extra=()):
    s = R / 100.0
    w = hittable_list()
    w.add(Sphere.stationary(point3(-12 * s, -3 * s, -8 * s), 6 * s, lambertian.from_color(color(0.7, 0.3, 0.2))))
    w.add(Sphere.stationary(point3(10 * s, -5 * s, 6 * s), 4 * s, lambertian.from_color(color(0.2, 0.5, 0.7))))
    w.add(Sphere.stationary(point3(3 * s, 4 * s, -12 * s), 5 * s, metal(color(0.8, 0.8, 0.7), 0.2)))
    w.add(quad(point3(-6 * s, 18 * s, -6 * s), vec3(12 * s, 0, 0), vec3(0, 0, 12 * s),
               diffuse_light.from_color(color(4, 4, 4))))
    w.add(triangle(point3(-15 * s, -10 * s, 5 * s), point3(-5 * s, -10 * s, 12 * s), point3(-10 * s, 2 * s, 8 * s),
                   lambertian.from_color(color(0.6, 0.6, 0.3))))
    for o in extra:
        w.add(o)
    if shell:
        w.add(constant_medium.from_color(Sphere.stationary(point3(0, 0, 0), R, dielectric(1.5)), color(0.8, 0.8, 0.9),
                                         0.5 / R))
    return w


def shell_arrays(R, **kw):
    random.seed(99)
    return sd.compile_world(_wrap(shell_world(R, **kw).objects))


def shell_camera(R, cam, width=WIDTH):
    s = R / 100.0
    frm, at, up, fov = CAMERAS[cam]
    c = camera()
    c.aspect_ratio = 1.0
    c.img_width = width
    c.vfov = fov
    c.lookfrom = point3(*(v * s for v in frm))
    c.lookat = point3(*(v * s for v in at))
    c.vup = vec3(*up)
    c.initialize()
    return sd.camera_upload(c)


def shell_scene(R, cam='inside'):
    """(SceneArrays, camera upload dict) of the shell scene."""
    if R not in _cache:
        _cache[R] = shell_arrays(R)
    return _cache[R], shell_camera(R, cam)


_oracle = {}


def oracle_accum(R, cam, spp, max_depth, variant='mk', traversal='stack'):
    """The oracle's accumulator (read-only) and counters, one per case."""
    import oracle
    key = (R, cam, spp, max_depth, variant, traversal)
    if key not in _oracle:
        sa, cu = shell_scene(R, cam)
        W, H = cu['width'], cu['height']
        fr = oracle.make_frame(cu, BG, max_depth, 7, W, H, traversal)
        acc = np.zeros((H, W, 3), np.float32)
        st = oracle.render(oracle.OracleScene(sa), fr, variant, acc, (0, 0, W, H), 0, spp)
        acc.setflags(write=False)
        _oracle[key] = (acc, {k: int(st[k]) for k in COUNTERS})
    return _oracle[key]


MODES = ('staged', 'overlapped', 'direct', 'listed', 'wf')


def gpu_accum(R, cam, spp, max_depth, mode='staged', traversal='stack', shell=None):
    """Accumulator and counters of the HIP integrator. mode: the staged
    megakernel, its overlapped calls, the direct one (ptmi_mk_render), the
    tile-listed trace (every tile listed), or the wavefront. shell: the scene
    view's hint, default what pack_device found."""
    import torch
    from ptmi import device
    sa, cu = shell_scene(R, cam)
    W, H = cu['width'], cu['height']
    layout = sd.pack_device(sa)
    assert layout.shell != 0, 'the test scene must have a shell'
    if shell is not None:
        layout.shell = shell
    integ = device.Integrator(device.DeviceScene(layout))
    fr = device.make_frame(cu, BG, max_depth, 7, W, H, traversal=traversal)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    if mode == 'staged':
        integ.render_mk(fr, acc, 0, spp, staged=True)
    elif mode == 'overlapped':
        half = spp // 2
        integ.render_mk(fr, acc, 0, half, overlap=True)
        integ.render_mk(fr, acc, half, spp - half, overlap=True)
    elif mode == 'direct':
        integ.render_mk(fr, acc, 0, spp, staged=False)
    elif mode == 'listed':
        tiles = integ.new_tiles(fr)
        integ.render_mk_stats(fr, acc, integ.new_stats(fr), 0, spp, tiles=(tiles['list'], tiles['n']))
    else:
        integ.render_wf(fr, acc, 0, spp)
    torch.cuda.synchronize()
    st = integ.read_counters()
    return acc.cpu().numpy(), {k: int(st[k]) for k in COUNTERS}


def same_bits(a, b):
    return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
