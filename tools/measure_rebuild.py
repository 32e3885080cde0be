"""The measurements of profiles/rebuild/ (DESIGN.md §20), one MI355X, one process:

  timing.json  ptmi_tree_growth (HIP events, median of 100) on vol2 and on
               synthetic rows the size of a tree of 2^20 leaves (random boxes,
               every other row internal: a timing, not a built tree);
               rebuild_bvh() wall (median of 3), the builder and pack_device
               timed on their own beside DeviceScene.rebuild, against a new
               MI355XRenderer of the same world
  sweep.json   vol2's 1000 box spheres displaced by +-5, 10, 25, 50, 100 % of the
               box side: mean / max growth and the C2 step rate (800x800,
               megakernel, 64 spp per step) on the refit tree, after rebuild()
               and on a new DeviceScene of the rebuilt arrays, alternated
  policy.json  the rule of ptmi.tree.REBUILD_GROWTH applied to the two

  python tools/measure_rebuild.py --out DIR [--steps 8] [--reps 3]
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

import tree_helpers as th  # noqa: E402
import update_helpers as uh  # noqa: E402
from ptmi import _lib, core, device, scene_data as sd, scenes, tree  # noqa: E402
from ptmi.renderer import MI355XRenderer  # noqa: E402

f32 = np.float32
SCENE, WIDTH, SPP = 'vol2_final_scene', 800, 64
BG = (0.0, 0.0, 0.0)


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


def growth_call(view, base, out):
    lib = tree.load()
    return lambda: _lib.check(lib.ptmi_tree_growth(view, base.data_ptr(), out.data_ptr(), None), 'ptmi_tree_growth')


def big_tree(leaves=1 << 20, seed=7):
    """ref_nodes of a synthetic tree of `leaves` leaves (every other row internal), a baseline and the boxes grown."""
    rng = np.random.default_rng(seed)
    n = 2 * leaves - 1
    rn = np.zeros((n, 12), f32)
    lo = rng.uniform(-1000, 1000, (n, 3)).astype(f32)
    rn[:, 0:3], rn[:, 4:7] = lo, lo + rng.uniform(0.5, 20, (n, 3)).astype(f32)
    words = rn.view(np.int32)
    words[:, 3] = np.where(np.arange(n) % 2 == 0, 1, -1)  # n_inner = leaves internal rows; never dereferenced
    base = th.areas(rn)
    rn[:, 4:7] += rng.uniform(0, 10, (n, 3)).astype(f32)
    return rn, base


def timing(args):
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'info': {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
                    'tree_version': tree.TREE_VERSION}}
    sa = sd.load_fixture(SCENE)
    ds = device.DeviceScene.from_arrays(sa)
    ds.tree_growth()
    ds.update_primitives(spheres=th.scatter(sa, 0.25))
    st = ds._tree
    res['tree_growth_vol2'] = dict(event_us(growth_call(ds.view, st['base'], st['out'])),
                                   num_bvh_nodes=sa.num_bvh_nodes, growth=list(ds.tree_growth()))
    t0 = time.perf_counter()
    for _ in range(30):
        ds.tree_growth()
    res['tree_growth_vol2']['wrapper_wall_us'] = (time.perf_counter() - t0) / 30 * 1e6
    rn, base = big_tree()
    t_rn, t_base = torch.from_numpy(rn.reshape(-1)).to(dev), torch.from_numpy(base).to(dev)
    out = torch.zeros(4, dtype=torch.float32, device=dev)
    v = _lib.SceneView()
    v.ref_nodes, v.num_bvh_nodes = t_rn.data_ptr(), rn.shape[0]
    big = event_us(growth_call(v, t_base, out), n=100, warm=3)
    want = th.growth(rn, base)
    res['tree_growth_2e20'] = dict(big, num_bvh_nodes=int(rn.shape[0]), equals_numpy=out.cpu().numpy().tobytes() ==
                                   want.tobytes(), growth=[float(want[0]), float(want[1])],
                                   bytes_touched=int(rn.shape[0]) * (48 + 4))  # 48-B rows (28 B used), 4 B baseline
    del t_rn, t_base

    # rebuild_bvh() against a new renderer of the same world
    random.seed(1234)
    sc = scenes.SCENES[SCENE](width=WIDTH)
    new_renderer, rebuild_wall, split = [], [], []
    r = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = MI355XRenderer(sc.world, sc.cam, os.path.join(args.out, 'unused.png'))
        torch.cuda.synchronize()
        new_renderer.append(time.perf_counter() - t0)
    res['new_renderer'] = {'wall_ms': [1e3 * t for t in new_renderer],
                           'median_ms': 1e3 * statistics.median(new_renderer),
                           'timing': {k: 1e3 * v for k, v in r.timing.items() if v}}
    rng = np.random.default_rng(1)
    balls = [i for i, s in enumerate(r.primitives['spheres']) if float(s.radius) == 10.0]
    for k in range(args.reps + 1):  # the first call also makes the update state: not counted
        move = {}
        for i in balls:
            s = r.primitives['spheres'][i]
            c = s.center.at(0.0)
            d = rng.uniform(-0.25 * 165, 0.25 * 165, 3)
            move[i] = core.Sphere.stationary(core.vec3(c.x + d[0], c.y + d[1], c.z + d[2]), s.radius, s.material)
        r.update_primitives(spheres=move)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.rebuild_bvh()
        torch.cuda.synchronize()
        if k:
            rebuild_wall.append(time.perf_counter() - t0)
    for k in range(args.reps):  # the parts, each timed on its own: the builder, pack_device, and the whole call
        ds = r.dscene
        t0 = time.perf_counter()
        built = th.rebuilt(ds.arrays)
        t1 = time.perf_counter()
        sd.pack_device(built)
        t2 = time.perf_counter()
        ds.rebuild()
        t3 = time.perf_counter()
        split.append({'builder': 1e3 * (t1 - t0), 'pack': 1e3 * (t2 - t1), 'rebuild': 1e3 * (t3 - t2),
                      'upload_baseline_topology': 1e3 * ((t3 - t2) - (t2 - t0))})
    res['rebuild_bvh'] = {'wall_ms': [1e3 * t for t in rebuild_wall],
                          'median_ms': 1e3 * statistics.median(rebuild_wall),
                          'moved_spheres': len(balls), 'num_bvh_nodes': r.num_bvh_nodes,
                          'split_ms': split,
                          'split_median_ms': {key: statistics.median(s[key] for s in split) for key in split[0]}}
    return res


def rate(integ, frame, acc, steps, warm=2):
    for k in range(warm):
        integ.render_mk(frame, acc, k * SPP, SPP, overlap=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        integ.render_mk(frame, acc, (warm + k) * SPP, SPP, overlap=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return frame.width * frame.height * SPP * steps / dt / 1e6


def sweep(args):
    sa = sd.load_fixture(SCENE)
    cam = sd.fixture_camera(SCENE, WIDTH)
    W, H = cam['width'], cam['height']
    frame = device.make_frame(cam, BG, 50, 0, W, H)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    cases = {}
    for pct in (5, 10, 25, 50, 100):
        edit = th.scatter(sa, pct / 100.0)
        refit = device.DeviceScene.from_arrays(sa)
        refit.update_primitives(spheres=edit)
        growth = refit.tree_growth()
        rebuilt = device.DeviceScene.from_arrays(sa)
        rebuilt.update_primitives(spheres=edit)
        rebuilt.rebuild()
        want = th.rebuilt(uh.refit(sa, {'spheres': edit}))
        new = device.DeviceScene.from_arrays(want)
        assert uh.layouts_equal(rebuilt.layout, new.layout) == []
        integ = {k: device.Integrator(ds) for k, ds in (('refit', refit), ('rebuilt', rebuilt), ('new', new))}
        runs = {k: [] for k in integ}
        for _ in range(args.reps):
            for k, it in integ.items():
                runs[k].append(rate(it, frame, acc, args.steps))
        med = {k: statistics.median(v) for k, v in runs.items()}
        cases[f'{pct}%'] = {'mean_growth': growth[0], 'max_growth': growth[1], 'msamples_per_s': runs, 'median': med,
                            'refit_over_rebuilt': med['refit'] / med['rebuilt'],
                            'depth_refit': refit.layout.max_leaf_depth, 'depth_rebuilt': rebuilt.layout.max_leaf_depth}
        print(pct, cases[f'{pct}%']['mean_growth'], med, flush=True)
    return {'workload': f'C2: {SCENE} {W}x{H}, megakernel, {SPP} spp per step, {args.steps} timed steps after 2, '
                        f'{args.reps} runs each, alternated', 'box_side': 165.0, 'cases': cases}


def policy(tim, swp):
    """ptmi.tree.REBUILD_GROWTH's rule: the smallest swept mean growth at which one 64-spp 800x800 step on the refit
    tree takes longer than the same step on the rebuilt tree plus rebuild_bvh()."""
    rebuild_ms = tim['rebuild_bvh']['median_ms']
    rows, chosen = [], None
    for name, c in sorted(swp['cases'].items(), key=lambda kv: kv[1]['mean_growth']):
        samples = 800 * 800 * SPP / 1e6
        step_refit, step_rebuilt = 1e3 * samples / c['median']['refit'], 1e3 * samples / c['median']['rebuilt']
        pays = step_refit - step_rebuilt > rebuild_ms
        rows.append({'displacement': name, 'mean_growth': c['mean_growth'], 'step_refit_ms': step_refit,
                     'step_rebuilt_ms': step_rebuilt, 'saved_per_step_ms': step_refit - step_rebuilt,
                     'rebuild_pays_within_one_step': pays})
        if pays and chosen is None:
            chosen = c['mean_growth']
    return {'rule': 'smallest swept mean growth at which (refit step - rebuilt step) of one 64-spp 800x800 megakernel '
                    'step exceeds the wall time of rebuild_bvh()', 'rebuild_bvh_ms': rebuild_ms, 'sweep': rows,
            'rebuild_growth': chosen}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', required=True)
    p.add_argument('--steps', type=int, default=8)
    p.add_argument('--reps', type=int, default=3)
    args = p.parse_args()
    os.makedirs(args.out, exist_ok=True)
    device.require_gpu()

    def save(name, obj):
        with open(os.path.join(args.out, name), 'w') as f:
            json.dump(obj, f, indent=1)

    tim = timing(args)
    save('timing.json', tim)
    swp = sweep(args)
    save('sweep.json', swp)
    save('policy.json', policy(tim, swp))


if __name__ == '__main__':
    main()
