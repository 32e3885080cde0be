"""The measurements of profiles/validate/ (DESIGN.md §21), one MI355X, one process:

  timing.json   ptmi_history_validate (radius 3) between HIP events, 100 calls
                after 5 warm-up calls, each call timed on its own (median) and
                all of them in a row (total / 100), at vol2 800x800 and
                `coverage` 3840x2160, beside ptmi_reproject and one 1-spp
                stats-path megakernel call (trace + stats resolve) of the same
                frame, measured the same way
  quality.json  the sliding sphere of tests/validate_helpers.py run by the
                renderer (64-spp history capped at 32, 4 fresh spp, against the
                oracle's 512 spp), and the 48-px `cornell_box` orbit of §15
                (64-spp history, 4 new spp, against 1024 spp) at the caps 8, 32
                and 64 with and without the validation

  python tools/measure_validate.py --out DIR
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'path-tracer-python_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import motion_helpers as mh  # noqa: E402
import parity_helpers as ph  # noqa: E402
import reproject_helpers as rh  # noqa: E402
import validate_helpers as vh  # noqa: E402
from ptmi import core, device, validate  # noqa: E402
from ptmi.renderer import MI355XRenderer  # noqa: E402

f32 = np.float32
CALLS, WARM = 100, 5


def event_us(fn):
    """CALLS calls of fn after WARM warm-up calls: each between two HIP events (median and extremes), and all
    in a row between two (total / CALLS), in microseconds."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        each.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return {'median_us': statistics.median(each), 'min_us': min(each), 'max_us': max(each),
            'in_a_row_us': a.elapsed_time(b) * 1e3 / CALLS, 'calls': CALLS, 'warm_up': WARM}


def timing():
    res = {'info': {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
                    'validate_version': validate.VALIDATE_VERSION, 'radius': 3}}
    for name, width in (('vol2_final_scene', 800), ('coverage', 3840)):
        sa, cam, bg = ph.scene_inputs(name, width)
        W, H = cam['width'], cam['height']
        integ = device.Integrator(device.DeviceScene.from_arrays(sa))
        frame = device.make_frame(cam, bg, 50, 0, W, H)
        zeros = lambda c: torch.zeros((H, W, c), dtype=torch.float32, device='cuda')  # noqa: E731
        hist, fresh, out, out2 = ((zeros(3), zeros(4)) for _ in range(4))
        integ.render_mk_stats(frame, *hist, 0, 8)   # a real history and real fresh samples: the branches a frame takes
        integ.render_mk_stats(frame, *fresh, 8, 4)
        guides = integ.trace_guides(frame)
        weight = torch.empty((H, W), dtype=torch.float32, device='cuda')
        scratch = (zeros(3), zeros(4))
        torch.cuda.synchronize()
        res[f'{name}_{W}x{H}'] = {
            'history_validate': event_us(lambda: integ.validate_history(*hist, *fresh, out=out)),
            'history_validate_with_weight': event_us(lambda: integ.validate_history(*hist, *fresh, out=out,
                                                                                    weight=weight)),
            'reproject': event_us(lambda: integ.reproject(cam, cam, guides, guides, *hist, out=out2)),
            'mk_stats_1spp': event_us(lambda: integ.render_mk_stats(frame, *scratch, 12, 1)),
        }
        print(name, json.dumps(res[f'{name}_{W}x{H}']), flush=True)
        del integ, hist, fresh, out, out2, guides, scratch
        torch.cuda.empty_cache()
    return res


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def slide_quality(tmp):
    """The sliding sphere, by the renderer: tests/test_gpu_validate.py's quality test, the figures kept."""
    q = vh.quality_case()
    out = {}
    for name, centre in (('moved', mh.SLIDE_TO), ('control', mh.SLIDE_FROM)):
        _, _, truth, changed = q[name]
        random.seed(1234)
        cam = mh.slide_camera_object()
        r = MI355XRenderer(mh.slide_world(mh.SLIDE_FROM), cam, os.path.join(tmp, 'slide.png'))
        r.background_color = vh.BACKGROUND
        r.render_adaptive(target_error=0.0, min_spp=vh.HISTORY_SAMPLES, max_spp=vh.HISTORY_SAMPLES)
        ball = core.Sphere.stationary(core.vec3(*centre), mh.SLIDE_RADIUS, r.primitives['spheres'][1].material)
        r.update_primitives(spheres={1: ball}, keep_history=True, max_history=vh.MAX_HISTORY)
        hist = (host(r.accum).copy(), host(r.stats).copy())
        plain = (r.accum.clone(), r.stats.clone())
        r.integrator.render_mk_stats(r.frame, *plain, vh.FRESH_BEGIN, vh.FRESH_SPP)
        per_radius = {}
        for radius in (3, 2):
            rr = (torch.empty_like(r.accum), torch.empty_like(r.stats))
            fresh = (torch.zeros_like(r.accum), torch.zeros_like(r.stats))
            r.integrator.render_mk_stats(r.frame, *fresh, vh.FRESH_BEGIN, vh.FRESH_SPP)
            w = torch.empty_like(r.stats[..., 0].contiguous())
            r.integrator.validate_history(r.accum, r.stats, *fresh, out=rr, weight=w, radius=radius)
            n_h = hist[1][..., 0].astype(np.float64)
            kept = float(np.round(host(w).astype(np.float64) * n_h).sum() / n_h.sum())
            per_radius[radius] = vh.orderings(hist, tuple(host(t) for t in fresh), tuple(host(t) for t in plain),
                                              tuple(host(t) for t in rr), kept, truth, changed)
        out[name] = {'radius_3': per_radius[3], 'radius_2': per_radius[2],
                     'equals_numpy': json.dumps(per_radius[3]) == json.dumps(vh.reference_orderings(q[name]))}
    vh.check_orderings(out['moved']['radius_3'], out['control']['radius_3'])
    return out


def orbit_quality(name='cornell_box', deltas=((4, 2), (40, 20)), caps=(8.0, 32.0, 64.0)):
    """§15's quality case with and without the validation: MSE of linear rgb against 1024 spp over the finite pixels."""
    sa, cam_obj, bg = rh.scene(name, 48)
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    out = {}
    for delta in deltas:
        prev, cur = rh.orbit(cam_obj, 0, 0), rh.orbit(cam_obj, *delta)
        W, H = prev['width'], prev['height']
        f0, f1 = device.make_frame(prev, bg, 50, 0, W, H), device.make_frame(cur, bg, 50, 0, W, H)
        zeros = lambda c: torch.zeros((H, W, c), dtype=torch.float32, device='cuda')  # noqa: E731
        a0, s0 = zeros(3), zeros(4)
        integ.render_mk_stats(f0, a0, s0, 0, 64)
        g0, g1 = integ.trace_guides(f0), integ.trace_guides(f1)
        ref = zeros(3)
        integ.render_mk(f1, ref, 10000, 1024)
        ref = host(ref) / f32(1024)
        fresh = (zeros(3), zeros(4))
        integ.render_mk_stats(f1, *fresh, 64, 4)
        imgs = {'alone': host(fresh[0]) / f32(4)}
        kept = {}
        for cap in caps:
            a, s = integ.reproject(cur, prev, g1, g0, a0, s0, max_history=cap)
            w = torch.empty((H, W), dtype=torch.float32, device='cuda')
            va, vs = integ.validate_history(a, s, *fresh, weight=w)
            n_h = host(s)[..., 0].astype(np.float64)
            kept[cap] = float(np.round(host(w).astype(np.float64) * n_h).sum() / n_h.sum())
            integ.render_mk_stats(f1, a, s, 64, 4)
            imgs[f'plain_cap{cap:g}'] = vh.image(host(a), host(s))
            imgs[f'validated_cap{cap:g}'] = vh.image(host(va), host(vs))
        ok = np.isfinite(ref).all(-1)
        for img in imgs.values():
            ok &= np.isfinite(img).all(-1)
        row = {k: float(np.mean((img[ok].astype(np.float64) - ref[ok]) ** 2)) for k, img in imgs.items()}
        row['history_kept'] = {f'cap{cap:g}': v for cap, v in kept.items()}
        row['finite_pixels'] = float(ok.mean())
        out[f'delta_{delta[0]}_{delta[1]}'] = row
        print(name, delta, json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:  # the renderer writes its image there
        quality = {'slide': slide_quality(tmp), 'cornell_box_orbit': orbit_quality()}
    with open(os.path.join(args.out, 'quality.json'), 'w') as f:
        json.dump(quality, f, indent=1)
    with open(os.path.join(args.out, 'timing.json'), 'w') as f:
        json.dump(timing(), f, indent=1)


if __name__ == '__main__':
    main()
