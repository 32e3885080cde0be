"""The measurements of profiles/rigid/ (DESIGN.md §25), one MI355X, one process:

  timing.json
    call      ptmi_pose_rigid next to ptmi_pose_primitives on the same entries
              (HIP events, median of 100): 1 sphere of vol2, and the 3000 mesh
              triangles of cornell_mesh_fog; DeviceScene.pose of each (wall,
              with its 24-byte root readback)
    frame     what one frame of an animation costs on the host and the device
              before its first sample is traced, on the 3000-triangle mesh
              (wall): the loop's step (a new shutter on resident bodies, one
              pose, one unpose) against MI355XRenderer.update_primitives of
              the posed objects built on the host; and the loop's step on
              vol2 with its 1000 small spheres in one body, where every frame
              also evaluates the posed shell hint
  sweep.json
    C2's shape (vol2 800x800, 1024 spp in 16 steps of 64, megakernel,
    overlapped) and C3's (wavefront) rendered unblurred, with the book's moving
    sphere as a linear track, and with the same sphere in a body that turns,
    slice_spp in {16, 32, 64}, interleaved, --reps times each: Msamples/s and
    the spread

  python tools/measure_rigid.py --out DIR [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'path-tracer-python_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from measure_motion_blur import SCENE, SHUTTER, SPP, STEP, WIDTH, event_us, renderer_of, wall_ms  # noqa: E402
from ptmi import core, device, pose, rigid, scene_data as sd  # noqa: E402

SLICES = (16, 32, 64)


def call_timing(name, out, kind, members, body_kw, d):
    """The rigid call and the linear call on the same entries of one scene."""
    r = renderer_of(name, out)
    ds, prims = r.dscene, r.primitives
    idx = members(r)
    times = [pose.vdc(j) for j in range(1, 9)]
    k = [0]

    def t():
        k[0] += 1
        return times[k[0] % len(times)]

    res = {'entries': len(idx), 'bvh_nodes': int(ds.view.num_bvh_nodes)}
    # linear tracks of these primitives
    tracks = {'spheres': {}, 'quads': {}, 'triangles': {}}
    tracks[kind] = {i: (prims[kind][i], d) for i in idx}
    if kind == 'spheres':  # a sphere's own direction is its track
        tracks[kind] = {i: (prims[kind][i], prims[kind][i].center.direction) for i in idx}
    ds.set_tracks(*pose.track_records(tracks), t_range=SHUTTER)
    res['linear_device'] = event_us(lambda: ds.pose_call(t()))
    res['linear_pose_wall_with_readback'] = wall_ms(lambda: ds.pose(t()), 50)
    ds.unpose()
    # the same primitives as one body
    if kind == 'spheres':  # a body's sphere may not move by itself
        r.set_motion(spheres={i: None for i in idx})
    bodies = [rigid.Body(spheres=idx if kind == 'spheres' else (), triangles=idx if kind == 'triangles' else (),
                         **body_kw)]
    ds.set_tracks(t_range=SHUTTER, rigid=(bodies, rigid.body_records(bodies, r.primitives)))
    res['rigid_device'] = event_us(lambda: ds.rigid_call(t()))
    res['rigid_pose_wall_with_readback'] = wall_ms(lambda: ds.pose(t()), 50)
    ds.unpose()
    torch.cuda.synchronize()
    return res, r, bodies


def frame_timing(r, bodies, host=True):
    """One frame's step of the animation loop against a host edit of the same pose (``host``: measure that too)."""
    r.set_bodies(bodies)
    r.slice_spp = 16
    frame = [0]

    def loop_step():
        frame[0] += 1
        t = frame[0] / 64.0
        r.shutter = (t, t)
        shutter = r._ensure_tracks()  # what _trace does before a frame's first slice ...
        r.dscene.pose(shutter[0])     # ... the slice's pose ...
        r.dscene.unpose()             # ... and the unpose at the frame's end

    res = {'animation_loop_step_wall': wall_ms(loop_step, 20, warm=2)}
    r.shutter = None
    if not host:
        return res
    body = bodies[0]

    def host_edit():
        frame[0] += 1
        at = rigid.body_at(body, frame[0] / 64.0)
        r.update_primitives(triangles={i: rigid.posed_object('triangles', r.primitives['triangles'][i], at)
                                       for i in body.triangles})

    res['renderer_update_primitives_wall'] = wall_ms(host_edit, 5, warm=1)
    return res


def sweep(reps):
    """C2's and C3's shapes: unblurred, the moving sphere as a linear track, the same sphere in a turning body."""
    sa = sd.load_fixture(SCENE)
    cam = sd.fixture_camera(SCENE, WIDTH)
    W, H = cam['width'], cam['height']
    ds = device.DeviceScene.from_arrays(sa)
    i = int(np.flatnonzero((sa.sphere_data[:, :3] == np.array([400, 400, 200], np.float32)).all(axis=1))[0])
    c = [float(x) for x in sa.sphere_data[i, :3]]
    sphere = core.Sphere.stationary(core.vec3(*c), float(sa.sphere_data[i, 3]), None)
    # the sphere swings 30 units over the shutter on an arc about a pivot 100 below it
    body = rigid.Body(core.vec3(c[0], c[1] - 100.0, c[2]), core.vec3(0, 0, 1), -0.3, spheres=[i])
    records = ((np.array([i]), np.zeros(1, np.int32), np.array([rigid.rest_record('spheres', sphere)])), None, None)
    modes = {'linear': dict(spheres=(np.array([i]), np.array([c + [30.0, 0.0, 0.0]]))),
             'rigid': dict(rigid=([body], records))}
    integ = device.Integrator(ds)
    fr = device.make_frame(cam, (0, 0, 0), 50, 0, W, H)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device=ds.device)

    def run(variant, mode, slice_spp):
        fn = integ.render_mk if variant == 'mk' else integ.render_wf
        kw = {'overlap': True} if variant == 'mk' else {}
        if mode is not None:
            ds.set_tracks(t_range=SHUTTER, **modes[mode])
        integ.clear(fr, acc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s0 in range(0, SPP, STEP):
            if mode is None:
                fn(fr, acc, s0, STEP, **kw)
            else:
                integ.render_posed(fn, fr, s0, STEP, slice_spp, SHUTTER, acc, **kw)
        if mode is not None:
            integ.unpose()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {}
    configs = [(None, None)] + [(m, s) for s in SLICES for m in ('linear', 'rigid')]
    for variant, label in (('mk', 'c2_megakernel'), ('wf', 'c3_wavefront')):
        secs = {c: [] for c in configs}
        for c in configs:  # warm-up, every configuration once
            run(variant, *c)
        for _ in range(reps):
            for c in configs:  # interleaved
                secs[c].append(run(variant, *c))
        rows = {}
        for c in configs:
            rate = [W * H * SPP / s / 1e6 for s in secs[c]]
            rows['unblurred' if c[0] is None else f'{c[0]}_slice_spp_{c[1]}'] = {
                'msamples_per_s': rate, 'median': statistics.median(rate),
                'spread_percent': 100.0 * (max(rate) - min(rate)) / statistics.median(rate)}
        for row in rows.values():
            row['relative_to_unblurred'] = row['median'] / rows['unblurred']['median']
        out[label] = rows
    return {'workload': f'{SCENE} {WIDTH}x{WIDTH}, {SPP} spp in steps of {STEP}, one sphere moving, shutter (0, 1)',
            'order': 'unblurred, then linear and rigid per slice_spp 16, 32, 64, repeated', 'reps': reps, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device('cuda', torch.cuda.current_device())
    info = {'device': torch.cuda.get_device_name(dev), 'torch': torch.__version__,
            'rigid_version': rigid.RIGID_VERSION, 'pose_version': pose.POSE_VERSION}

    def moving_sphere(r):
        return [i for i, s in enumerate(r.primitives['spheres']) if not pose._is_zero(s.center.direction)]

    vol2, _, _ = call_timing(SCENE, args.out, 'spheres', moving_sphere,
                             dict(pivot=core.vec3(400, 300, 200), axis=core.vec3(0, 0, 1), turn=-0.3), None)
    mesh, r, bodies = call_timing('cornell_mesh_fog', args.out, 'triangles',
                                  lambda r: list(range(len(r.primitives['triangles']))),
                                  dict(pivot=core.vec3(278, 140, 278), axis=core.vec3(0, 1, 0), turn=1.0,
                                       displacement=core.vec3(5.0, 10.0, -5.0)), core.vec3(5.0, 10.0, -5.0))
    # a scene with a shell hint: every frame re-evaluates it (two poses, two ref_nodes readbacks, the swept boxes)
    rv = renderer_of(SCENE, args.out)
    small = [i for i, s in enumerate(rv.primitives['spheres']) if s.radius == 10.0]
    cluster = [rigid.Body(core.vec3(-20, 350, 475), core.vec3(0, 1, 0), 1.0, spheres=small)]
    res = {'info': info, 'call': {'vol2_one_sphere': vol2, 'cornell_mesh_fog_every_triangle': mesh},
           'frame': {'cornell_mesh_fog_every_triangle': frame_timing(r, bodies),
                     'vol2_small_spheres_with_shell_hint': dict(frame_timing(rv, cluster, host=False),
                                                                entries=len(small))}}
    with open(os.path.join(args.out, 'timing.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)
    sw = {'info': info, 'sweep': sweep(args.reps)}
    with open(os.path.join(args.out, 'sweep.json'), 'w') as f:
        json.dump(sw, f, indent=1)
    print(json.dumps(sw, indent=1), flush=True)
    if os.path.exists(os.path.join(args.out, 'unused.png')):
        os.unlink(os.path.join(args.out, 'unused.png'))


if __name__ == '__main__':
    main()
