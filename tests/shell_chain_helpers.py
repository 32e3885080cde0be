"""Helpers of the shell-chain tests (test infrastructure only): the scenes
(shell_scenes.shell_world with extra primitives that lengthen or deepen the
chain of ancestors above the shell's leaf), the ray sets, and the call of the
CPU check program (csrc/shell_chain_check.cpp)."""
from __future__ import annotations

import os
import random
import subprocess

import numpy as np

import shell_scenes as ss
from ptmi import scene_data as sd
from ptmi.core import Sphere, color, lambertian, point3
from ptmi.scenes import _wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
CHAIN_MAX = 6  # kShellChainMax, csrc/pt_shell_chain.hpp


def kernel_slots(max_leaf_depth):
    """The staged megakernel's stack slots for a scene with a hint
    (shell_chain_stack_request, then the rungs 16, 17, 18, 20 of the dispatch)."""
    need = max_leaf_depth + 1
    assert need <= 20
    want = need + CHAIN_MAX - 2
    return 20 if want >= 19 else max(want, 16)


def build_check(path, flags=None):
    cmd = ['make', '-s', '-C', CSRC, 'shell_chain_check', f'SHELL_CHAIN_CHECK={path}']
    if flags:
        cmd.append(f'SHELL_CHAIN_CHECK_FLAGS={flags}')
    subprocess.run(cmd, check=True)
    return path


def cluster(R, n, seed, spread=0.25, centre=(0.0, 0.0, 0.0)):
    """n small Lambertian spheres within spread * R of centre * R (well inside R / 2 of the origin)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = (np.asarray(centre) + rng.uniform(-spread, spread, 3) / np.sqrt(3.0)) * R
        out.append(Sphere.stationary(point3(*p), 0.012 * R, lambertian.from_color(color(*rng.uniform(0.2, 0.8, 3)))))
    return out


# name -> extra primitives of shell_world(R): what the SAH builder makes of them
# is pinned by test_shell_chain.py (chain length, leaf depth)
EXTRAS = {
    'base': lambda R: [],
    'few': lambda R: cluster(R, 40, 5),
    'many': lambda R: cluster(R, 700, 6),
    'deep': lambda R: cluster(R, 6000, 7),
}

_arrays = {}


def chain_arrays(name, R):
    key = (name, R)
    if key not in _arrays:
        random.seed(99)
        _arrays[key] = sd.compile_world(_wrap(ss.shell_world(R, extra=EXTRAS[name](R)).objects))
    return _arrays[key]


def rechain(sa, length, flip=0):
    """The scene's arrays under a hand-built BVH (reference layout, preorder,
    left child at i + 1, node box = union of the children's): a chain of
    `length` internal nodes, each holding a balanced subtree over a share of
    the other primitives on one side and the rest of the chain on the other,
    the shell's leaf under the last. Bit k of flip puts level k's chain child
    on the left (child 0) instead of the right."""
    import dataclasses
    b = sa.bvh
    leaves = np.nonzero(b['bvh_prim_idx'] >= 0)[0]
    R = sa.sphere_data[:, 3].max()
    prim = [(int(b['bvh_prim_type'][i]), int(b['bvh_prim_idx'][i]), b['bvh_bbox_min'][i].copy(), b['bvh_bbox_max'][i].copy())
            for i in leaves]
    shell = [p for p in prim if p[0] == sd.PRIM_SPHERE and sa.sphere_data[p[1], 3] == R]
    rest = [p for p in prim if p not in shell]
    assert len(shell) == 1 and len(rest) >= length
    cuts = [round(k * len(rest) / length) for k in range(length + 1)]

    def balanced(ps):
        return ps[0] if len(ps) == 1 else (balanced(ps[:len(ps) // 2]), balanced(ps[len(ps) // 2:]))

    tree = shell[0]
    for k in reversed(range(length)):
        sib = balanced(rest[cuts[k]:cuts[k + 1]])
        tree = (tree, sib) if (flip >> k) & 1 else (sib, tree)
    n = 2 * len(prim) - 1
    out = {'bvh_bbox_min': np.zeros((n, 3), f32), 'bvh_bbox_max': np.zeros((n, 3), f32)}
    for key in ('bvh_left_child', 'bvh_right_child', 'bvh_parent', 'bvh_prim_type', 'bvh_prim_idx'):
        out[key] = np.full(n, -1, np.int32)
    count = [0]

    def emit(t, parent):
        i = count[0]
        count[0] += 1
        out['bvh_parent'][i] = parent
        if len(t) == 4:
            out['bvh_prim_type'][i], out['bvh_prim_idx'][i] = t[0], t[1]
            out['bvh_bbox_min'][i], out['bvh_bbox_max'][i] = t[2], t[3]
        else:
            l = emit(t[0], i)
            r = emit(t[1], i)
            out['bvh_left_child'][i], out['bvh_right_child'][i] = l, r
            out['bvh_bbox_min'][i] = np.minimum(out['bvh_bbox_min'][l], out['bvh_bbox_min'][r])
            out['bvh_bbox_max'][i] = np.maximum(out['bvh_bbox_max'][l], out['bvh_bbox_max'][r])
        return i

    emit(tree, -1)
    assert count[0] == n
    return dataclasses.replace(sa, bvh=out)


# name -> (extras, chain length or None for the builder's own BVH, flip)
SCENES = {
    'c1': ('base', 1, 0),       # the shell's leaf under the root
    'c3': ('few', 3, 0b010),
    'c8': ('few', 8, 0b10100101),  # longer than kShellChainMax
    'sah5': ('many', None, 0),  # the SAH builder's: 5 levels, leaf depth 13
    'deep': ('deep', None, 0),  # 5 levels under leaf depth 17: the 20-slot kernel expands 3
}


def scene_arrays(name, R):
    key = ('scene', name, R)
    if key not in _arrays:
        extras, length, flip = SCENES[name]
        sa = chain_arrays(extras, R)
        _arrays[key] = sa if length is None else rechain(sa, length, flip)
    return _arrays[key]


_oracle = {}


def oracle_accum(name, R, cam, spp, max_depth):
    """The oracle's accumulator (read-only) and counters of a chain scene, one per case."""
    import oracle
    key = (name, R, cam, spp, max_depth)
    if key not in _oracle:
        sa, cu = scene_arrays(name, R), ss.shell_camera(R, cam)
        W, H = cu['width'], cu['height']
        fr = oracle.make_frame(cu, ss.BG, max_depth, 7, W, H)
        acc = np.zeros((H, W, 3), f32)
        st = oracle.render(oracle.OracleScene(sa), fr, 'mk', acc, (0, 0, W, H), 0, spp)
        acc.setflags(write=False)
        _oracle[key] = (acc, {k: int(st[k]) for k in ss.COUNTERS})
    return _oracle[key]


def gpu_accum(name, R, cam, spp, max_depth, mode='staged', shell=None):
    """Accumulator and counters of the megakernel on a chain scene
    (shell_scenes.gpu_accum's modes). shell: the hint, default pack_device's."""
    import torch
    from ptmi import device
    sa, cu = scene_arrays(name, R), ss.shell_camera(R, cam)
    W, H = cu['width'], cu['height']
    layout = sd.pack_device(sa)
    assert layout.shell != 0
    if shell is not None:
        layout.shell = shell
    integ = device.Integrator(device.DeviceScene(layout))
    fr = device.make_frame(cu, ss.BG, max_depth, 7, W, H)
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
    else:
        assert mode == 'listed'
        tiles = integ.new_tiles(fr)
        integ.render_mk_stats(fr, acc, integ.new_stats(fr), 0, spp, tiles=(tiles['list'], tiles['n']))
    torch.cuda.synchronize()
    st = integ.read_counters()
    return acc.cpu().numpy(), {k: int(st[k]) for k in ss.COUNTERS}


def run_check(exe, tmp_path, layout, rays, stack, shell=None):
    """The check program on a DeviceLayout and an (n, 7) f32 ray array (o, d,
    tmin). Returns (info, out): the chain line as a dict and the (n, 8) u32
    results."""
    names = ('nodes', 'spheres', 'quads', 'tris')
    paths = [str(tmp_path / (n + '.f32')) for n in names] + [str(tmp_path / 'rays.f32'), str(tmp_path / 'out.u32')]
    for n, p in zip(names, paths):
        np.ascontiguousarray(getattr(layout, n), f32).tofile(p)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 7)
    rays.tofile(paths[4])
    args = [layout.shell if shell is None else shell, layout.n_inner, layout.root_ref, layout.max_leaf_depth, stack]
    r = subprocess.run([exe] + [str(int(a)) for a in args] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    w = r.stdout.split('\n')[0].split()
    assert w[0] == 'chain' and w[14] == 'off'
    info = dict(m=int(w[2]), full=int(w[4]), side=int(w[6]), plan_m=int(w[9]), skip=int(w[11]), slots=int(w[13]),
                off=[int(x) for x in w[15:]])
    return info, np.fromfile(paths[5], np.uint32).reshape(-1, 8)


def subtree(layout, ref):
    """(leaves, deepest leaf's depth below ref) of the subtree at a child ref."""
    if ref < 0:
        return 1, 0
    row = layout.nodes[ref // sd.NODE_BYTES]
    a = subtree(layout, int(row[12].view(np.int32)))
    b = subtree(layout, int(row[13].view(np.int32)))
    return a[0] + b[0], 1 + max(a[1], b[1])
