"""The measurements of profiles/device_build/ (DESIGN.md §23), one MI355X, one process:

  timing.json  ptmi_build_sah_device and ptmi_build_pack, each between two HIP
               events, median of 100, on vol2_final_scene (after a +-25 %
               scatter) and cornell_mesh_fog; the wall time of
               rebuild_bvh(builder='device') against rebuild_bvh(), alternated
               in one process on a renderer of vol2 (800 px) whose box spheres
               moved, all values and the medians; the parts of the device path,
               timed on copies of the scene's tensors, and the rest of the call
  sweep.json   tools/measure_rebuild.py's sweep, run again in this visit
  policy.json  ptmi.tree.REBUILD_GROWTH's rule with the device rebuild's wall
               time: the value of ptmi.build.REBUILD_GROWTH_DEVICE

  python tools/measure_device_build.py --out DIR [--steps 8] [--reps 3] [--walls 15]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import measure_rebuild as mr  # noqa: E402  (puts the package and tests/ on the path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import parity_helpers as ph  # noqa: E402
import tree_helpers as th  # noqa: E402
from ptmi import build, core, device, scene_data as sd, scenes  # noqa: E402
from ptmi.renderer import MI355XRenderer  # noqa: E402


def abi_calls(sa, edit):
    """HIP-event times of the two ABI calls on a resident scene after ``edit``; the pack is timed on the scene itself
    (it permutes the rows again each call, which costs the same)."""
    ds = device.DeviceScene.from_arrays(sa)
    ds.update_primitives(**edit)
    ds.rebuild(builder='device')  # leaves a packed scene: the pack timed below permutes rows onto themselves
    assert ds.last_rebuild['builder'] == 'device'
    b = build.DeviceBuilder(sd.counts_by_code(ds.layout), ds.device)
    b.upload(build.builder_records(ds.arrays), [np.argsort(np.asarray(p, np.int64)) for p in ds.layout.prim_perm])
    out = {'prims': b.n, 'nodes': b.nodes, 'workspace_bytes': b.ws_bytes,
           'build': mr.event_us(lambda: b.build(None)),
           'pack': mr.event_us(lambda: b.pack(ds.view, None))}
    _, status, info, _, _ = b.read_ints()
    out['status'] = [int(x) for x in status]
    return out


def move_balls(r, rng):
    balls = [i for i, s in enumerate(r.primitives['spheres']) if float(s.radius) == 10.0]
    move = {}
    for i in balls:
        s = r.primitives['spheres'][i]
        c = s.center.at(0.0)
        d = rng.uniform(-0.25 * 165, 0.25 * 165, 3)
        move[i] = core.Sphere.stationary(core.vec3(c.x + d[0], c.y + d[1], c.z + d[2]), s.radius, s.material)
    r.update_primitives(spheres=move)
    torch.cuda.synchronize()


def walls(args):
    random.seed(1234)
    sc = scenes.SCENES[mr.SCENE](width=mr.WIDTH)
    r = MI355XRenderer(sc.world, sc.cam, os.path.join(args.out, 'unused.png'))
    rng = np.random.default_rng(1)
    out = {'host': [], 'device': []}
    for k in range(2 * (args.walls + 1)):  # alternated; the first of each also makes its state: not counted
        builder = ('host', 'device')[k % 2]
        move_balls(r, rng)
        t0 = time.perf_counter()
        r.rebuild_bvh() if builder == 'host' else r.rebuild_bvh(builder='device')
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        assert r.dscene.last_rebuild['builder'] == builder
        if k >= 2:
            out[builder].append(dt)
    # the device path's parts, timed from outside on copies of the scene's tensors (the scene itself is not touched):
    # what is left of the whole call's wall time is the host remainder
    from ptmi import _lib
    ds = r.dscene
    names = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris', 'mats')
    copies = {k: getattr(ds, 't_' + k).clone() for k in names}
    view = _lib.SceneView.from_buffer_copy(ds.view)
    for k, t in copies.items():
        setattr(view, k, t.data_ptr())
    b = build.DeviceBuilder(sd.counts_by_code(ds.layout), ds.device)
    old_row = [np.argsort(np.asarray(p, np.int64)) for p in ds.layout.prim_perm]
    parts = []
    for k in range(args.walls + 1):
        for name, t in copies.items():
            t.copy_(getattr(ds, 't_' + name))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.upload(build.builder_records(ds.arrays), old_row)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        b.build(None)
        b.pack(view, None)
        _, status, info, _, _ = b.read_ints()
        t2 = time.perf_counter()
        b.read_boxes()
        for t in copies.values():
            t.cpu()
        t3 = time.perf_counter()
        assert int(status[0]) == 0 and int(info[10]) == 0
        if k:
            parts.append({'records and upload': 1e3 * (t1 - t0), 'kernels and int readback': 1e3 * (t2 - t1),
                          'box and tensor readback': 1e3 * (t3 - t2)})
    med = {k: statistics.median(p[k] for p in parts) for k in parts[0]}
    med['host remainder (mirror, shell hint, layout, view, topology, baseline)'] = \
        statistics.median(out['device']) - sum(med.values())
    return {'rebuild_bvh_wall_ms': out, 'median_ms': {k: statistics.median(v) for k, v in out.items()},
            'device_over_host': statistics.median(out['device']) / statistics.median(out['host']),
            'device_parts_median_ms': med, 'moved_spheres': 1000, 'num_bvh_nodes': r.num_bvh_nodes}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', required=True)
    p.add_argument('--steps', type=int, default=8)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--walls', type=int, default=15)
    args = p.parse_args()
    os.makedirs(args.out, exist_ok=True)
    device.require_gpu()

    def save(name, obj):
        with open(os.path.join(args.out, name), 'w') as f:
            json.dump(obj, f, indent=1)

    dev = torch.device('cuda', torch.cuda.current_device())
    tim = {'info': {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
                    'build_version': build.BUILD_VERSION, 'max_prims': build.MAX_PRIMS}}
    vol2 = sd.load_fixture(mr.SCENE)
    tim['vol2_final_scene'] = abi_calls(vol2, {'spheres': th.scatter(vol2, 0.25)})
    fog = ph.fixture('cornell_mesh_fog', 64)
    tim['cornell_mesh_fog'] = abi_calls(fog, th.mixed_edit(fog))
    tim['rebuild_bvh'] = walls(args)
    save('timing.json', tim)
    print(json.dumps(tim, indent=1), flush=True)
    swp = mr.sweep(args)
    save('sweep.json', swp)
    pol = mr.policy({'rebuild_bvh': {'median_ms': tim['rebuild_bvh']['median_ms']['device']}}, swp)
    pol['rule'] += " with builder='device'"
    pol['host_rebuild_bvh_ms'] = tim['rebuild_bvh']['median_ms']['host']
    pol['host_policy'] = mr.policy({'rebuild_bvh': {'median_ms': tim['rebuild_bvh']['median_ms']['host']}}, swp)[
        'rebuild_growth']
    save('policy.json', pol)
    print(json.dumps(pol, indent=1), flush=True)


if __name__ == '__main__':
    main()
