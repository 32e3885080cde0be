"""The measurements of profiles/materials/timing.json, one MI355X, one process, vol2:

  device    ptmi_update_materials (HIP events, median of 100) with 1 edit and
            with all spheres edited, the lists already on the device
  wrapper   DeviceScene.update_materials wall time (check, upload, call, sync,
            mirror, view) for the same two
  renderer  MI355XRenderer.update_materials wall time, host-inclusive (material
            records, the DeviceScene call, the image restart), for 1 sphere and
            for all of them, against a new MI355XRenderer of the edited world

  python tools/measure_materials.py --out DIR [--reps 3]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'path-tracer-python_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import material_helpers as mh  # noqa: E402
from ptmi import core, device, material, scene_data as sd, scenes  # noqa: E402
from ptmi.renderer import MI355XRenderer  # noqa: E402

SCENE, WIDTH = 'vol2_final_scene', 800


def event_us(fn, n=100, warm=10):
    """Median and extremes, in microseconds, of n calls of fn each between two HIP events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {'median_us': statistics.median(out), 'min_us': min(out), 'max_us': max(out), 'calls': n}


def wall_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return {'median_ms': statistics.median(out), 'min_ms': min(out), 'max_ms': max(out), 'calls': n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'info': {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__, 'scene': SCENE,
                    'material_version': material.MATERIAL_VERSION}}

    # the C call and the DeviceScene wrapper on the fixture
    sa = sd.load_fixture(SCENE)
    ds = device.DeviceScene.from_arrays(sa)
    ds.update_materials()
    st = ds._upd
    ns = sa.num_spheres
    res['info']['num_spheres'] = ns
    walk = mh.class_walk(len(sa.images))
    for label, idx in (('one_edit', np.array([ns // 2])), ('all_spheres', np.arange(ns))):
        rows = [np.stack([walk[(int(i) + k) % len(walk)][1] for i in idx]) for k in (0, 1)]
        tp = torch.from_numpy(st['dev_of'][0][idx].astype(np.int32)).to(dev)
        tl = torch.from_numpy(st['leaf_of'][0][idx].astype(np.int32)).to(dev)
        tr = [torch.from_numpy(r.reshape(-1)).to(dev) for r in rows]
        flip = [0]

        def call():
            flip[0] ^= 1
            ds.material_call({sd.PRIM_SPHERE: (tp.data_ptr(), tl.data_ptr(), tr[flip[0]].data_ptr(), len(idx))})

        def wrapped():
            flip[0] ^= 1
            ds.update_materials(spheres=(idx, rows[flip[0]]))

        res[label] = {'edits': int(len(idx)), 'device': event_us(call), 'wrapper': wall_ms(wrapped, 20)}
    ds.update_materials(spheres=mh.current(sa, 'spheres', np.arange(ns)))

    # the renderer, against a new renderer of the edited world
    random.seed(1234)
    sc = scenes.SCENES[SCENE](width=WIDTH)
    path = os.path.join(args.out, 'unused.png')
    new_renderer, r = [], None
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = MI355XRenderer(sc.world, sc.cam, path)
        torch.cuda.synchronize()
        new_renderer.append(1e3 * (time.perf_counter() - t0))
    res['new_renderer'] = {'wall_ms': new_renderer, 'median_ms': statistics.median(new_renderer),
                           'timing_ms': {k: 1e3 * v for k, v in r.timing.items() if v}}
    mats = [core.lambertian(core.solid_color(core.vec3(.2, .6, .3))), core.metal(core.vec3(.8, .6, .2), 0.1),
            core.dielectric(1.5)]
    n = len(r.primitives['spheres'])
    medium = np.asarray(r.arrays.sphere_mats['is_constant_medium']) > 0
    plain = [i for i in range(n) if not medium[i]]
    k = [0]

    def one():
        k[0] += 1
        r.update_materials(spheres={plain[len(plain) // 2]: mats[k[0] % 3]})

    def every():
        k[0] += 1
        r.update_materials(spheres={i: mats[(i + k[0]) % 3] for i in plain})

    res['renderer_one_edit'] = dict(wall_ms(one, 20), edits=1)
    res['renderer_all_spheres'] = dict(wall_ms(every, 5), edits=len(plain))
    with open(os.path.join(args.out, 'timing.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
