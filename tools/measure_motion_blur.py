"""The measurements of profiles/motion_blur/ (DESIGN.md §24), one MI355X, one process:

  timing.json
    pose      ptmi_pose_primitives (HIP events, median of 100) on vol2 with 1
              track and on cornell_mesh_fog with every mesh triangle tracked,
              next to ptmi_update_primitives on the same posed records already
              on the device, DeviceScene.pose (wall, with its 24-byte root
              readback) and MI355XRenderer.update_primitives of the same posed
              objects (wall)
  sweep.json
    C2's shape (vol2 800x800, 1024 spp in 16 steps of 64, megakernel,
    overlapped) and C3's (wavefront) rendered blurred with slice_spp in
    {4, 8, 16, 32, 64} and unblurred, interleaved, --reps times each:
    Msamples/s, the spread, and the share of the time that the pose calls'
    device time is
  images.json, still_256spp.png, blurred_256spp.png
    vol2 800x800 at 256 spp without and with shutter (0, 1), and the number of
    pixels in which the two differ visibly; a crop around the moving sphere if
    the whole PNG would pass 1 MB. The PNGs are for looking at: only the JSON
    is kept under profiles/

  python tools/measure_motion_blur.py --out DIR [--reps 3]
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

from ptmi import core, device, pose, scene_data as sd, scenes  # noqa: E402
from ptmi.renderer import MI355XRenderer  # noqa: E402

SCENE, WIDTH, SPP, STEP = 'vol2_final_scene', 800, 1024, 64
SLICES = (4, 8, 16, 32, 64)
SHUTTER = (0.0, 1.0)
PNG_LIMIT = 1000000


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


def renderer_of(name, out, **kw):
    random.seed(1234)
    sc = scenes.SCENES[name](width=WIDTH) if name == SCENE else scenes.SCENES[name]()
    r = MI355XRenderer(sc.world, sc.cam, os.path.join(out, 'unused.png'), **kw)
    r.background_color, r.max_depth = sc.background, sc.max_depth
    return r


def pose_timing(name, out, tracked):
    """The pose call beside the update call and the renderer's update, for the tracks ``tracked(renderer)`` names."""
    r = renderer_of(name, out)
    motion = tracked(r)
    tracks = pose.tracks_of(r.primitives, motion)
    ds = r.dscene
    ds.set_tracks(*pose.track_records(tracks), t_range=SHUTTER)
    times = [pose.vdc(j) for j in range(1, 9)]
    k = [0]

    def t():
        k[0] += 1
        return times[k[0] % len(times)]

    # the same posed records as an update whose lists are already on the device
    from ptmi import update
    lists = []
    for tt in times:
        edits = update.check_edits(sd.counts_by_code(ds.layout), *pose.posed_records(tracks, tt))
        lists.append(ds._pack_edits(edits))
    n = sum(len(v) for v in tracks.values())

    def update_call():
        k[0] += 1
        ds.update_call(lists[k[0] % len(lists)][0])

    res = {'tracks': n, 'bvh_nodes': int(ds.view.num_bvh_nodes),
           'pose_device': event_us(lambda: ds.pose_call(t())),
           'update_device': event_us(update_call),
           'pose_wall_with_readback': wall_ms(lambda: ds.pose(t()), 50)}
    ds.unpose()
    torch.cuda.synchronize()

    def renderer_update():
        tt = t()
        r.update_primitives(**{kind: {i: pose.posed_object(kind, obj, d, tt) for i, (obj, d) in tr.items()}
                               for kind, tr in tracks.items() if tr})

    res['renderer_update_primitives_wall'] = wall_ms(renderer_update, 5, warm=1)
    return res


def vol2_motion(r):
    """The book's one moving sphere: tracked by itself."""
    moving = [i for i, s in enumerate(r.primitives['spheres']) if not pose._is_zero(s.center.direction)]
    assert len(moving) == 1, moving
    return {}


def mesh_motion(r):
    return {'triangles': {i: core.vec3(5.0, 10.0, -5.0) for i in range(len(r.primitives['triangles']))}}


def sweep(res, reps):
    """C2's and C3's shapes, blurred per slice_spp and unblurred, interleaved."""
    sa = sd.load_fixture(SCENE)
    cam = sd.fixture_camera(SCENE, WIDTH)
    W, H = cam['width'], cam['height']
    ds = device.DeviceScene.from_arrays(sa)
    # the book's moving sphere, frozen in the captured arrays at its t = 0 centre: (400, 400, 200) to (430, 400, 200)
    i = int(np.flatnonzero((sa.sphere_data[:, :3] == np.array([400, 400, 200], np.float32)).all(axis=1))[0])
    c = [float(x) for x in sa.sphere_data[i, :3]]
    ds.set_tracks(spheres=(np.array([i]), np.array([c + [30.0, 0.0, 0.0]])), t_range=SHUTTER)
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, (0, 0, 0), 50, 0, W, H)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device=ds.device)
    pose_us = res['pose']['vol2_one_track']['pose_device']['median_us']

    def run(variant, slice_spp):
        fn = integ.render_mk if variant == 'mk' else integ.render_wf
        kw = {'overlap': True} if variant == 'mk' else {}
        integ.clear(fr, acc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s0 in range(0, SPP, STEP):
            if slice_spp is None:
                fn(fr, acc, s0, STEP, **kw)
            else:
                integ.render_posed(fn, fr, s0, STEP, slice_spp, SHUTTER, acc, **kw)
        if slice_spp is not None:
            integ.unpose()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {}
    for variant, label in (('mk', 'c2_megakernel'), ('wf', 'c3_wavefront')):
        configs = [None] + list(SLICES)
        secs = {c: [] for c in configs}
        for c in configs:  # warm-up, every configuration once
            run(variant, c)
        for _ in range(reps):
            for c in configs:  # interleaved
                secs[c].append(run(variant, c))
        rows = {}
        for c in configs:
            rate = [W * H * SPP / s / 1e6 for s in secs[c]]
            row = {'msamples_per_s': rate, 'median': statistics.median(rate),
                   'spread_percent': 100.0 * (max(rate) - min(rate)) / statistics.median(rate)}
            if c is not None:
                poses = SPP // c
                row.update(poses=poses, pose_device_share_percent=100.0 * poses * pose_us * 1e-6 /
                           statistics.median(secs[c]))
            rows['unblurred' if c is None else f'slice_spp_{c}'] = row
        for key, row in rows.items():
            row['relative_to_unblurred'] = row['median'] / rows['unblurred']['median']
        out[label] = rows
    res['sweep'] = {'workload': f'{SCENE} {WIDTH}x{WIDTH}, {SPP} spp in steps of {STEP}, 1 tracked sphere, shutter (0, 1)',
                    'order': 'unblurred, 4, 8, 16, 32, 64, repeated', 'reps': reps, **out}


def images(out):
    from PIL import Image
    shots = {}
    for label, kw in (('still', {}), ('blurred', {'shutter': SHUTTER})):
        r = renderer_of(SCENE, out, **kw)
        r.cam.samples_per_pixel = 256
        r.render(enable_preview=False)
        shots[label] = r.image_u8()
    diff = np.abs(shots['still'].astype(int) - shots['blurred'].astype(int)).max(axis=2) > 24
    note = {'spp': 256, 'pixels_differing_by_more_than_24': int(diff.sum())}
    box = None
    for label, img in shots.items():
        path = os.path.join(out, f'{label}_256spp.png')
        Image.fromarray(img, mode='RGB').save(path, optimize=True)
        if os.path.getsize(path) > PNG_LIMIT:  # a crop around what moved
            if box is None:
                ys, xs = np.nonzero(diff)
                cy, cx = (int(ys.mean()), int(xs.mean())) if ys.size else (img.shape[0] // 2, img.shape[1] // 2)
                y0, x0 = min(max(0, cy - 200), img.shape[0] - 400), min(max(0, cx - 200), img.shape[1] - 400)
                box = (x0, y0, x0 + 400, y0 + 400)
            Image.fromarray(img, mode='RGB').crop(box).save(path, optimize=True)
            note['crop'] = list(box)
    return note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'info': {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
                    'pose_version': pose.POSE_VERSION},
           'pose': {'vol2_one_track': pose_timing(SCENE, args.out, vol2_motion),
                    'cornell_mesh_fog_every_triangle': pose_timing('cornell_mesh_fog', args.out, mesh_motion)}}
    with open(os.path.join(args.out, 'timing.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)
    sw = {'info': res['info'], 'pose': res['pose']}
    sweep(sw, args.reps)
    sw = {'info': res['info'], 'sweep': sw['sweep']}
    with open(os.path.join(args.out, 'sweep.json'), 'w') as f:
        json.dump(sw, f, indent=1)
    print(json.dumps(sw, indent=1), flush=True)
    note = images(args.out)
    with open(os.path.join(args.out, 'images.json'), 'w') as f:
        json.dump(note, f, indent=1)
    print(json.dumps(note), flush=True)
    for name in ('unused.png',):
        if os.path.exists(os.path.join(args.out, name)):
            os.unlink(os.path.join(args.out, name))


if __name__ == '__main__':
    main()
