"""The HIP integrators against the reference's own kernel text, directly.

tests/golden/kernel_paths_<scene>.npz hold the colour and the counters of every
path of tiny frames as the reference's kernels.py computed them over the Taichi
stand-in (tests/golden/gen_kernel_paths.py). Each frame is rendered here one
sample per call with the megakernel and the wavefront; `accum` must equal, bit
for bit, the f32 sum of the recorded path colours in sample order, and the
kernels' segment / medium-exit / RR / depth-cap counters the recorded totals.
pt_oracle.c takes no part in this check, and nothing here reads the reference.
"""
import numpy as np
import pytest

from kernel_path_fixtures import SCENES, VARIANTS, frame_args, load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('name', SCENES)
def test_gpu_equals_reference_text(name, variant):
    import torch
    from ptmi import device
    z, sa, cam = load(name)
    Wd, Ht, spp = cam['width'], cam['height'], int(z['spp'])
    cam_, bg, max_depth, seed, _, _, traversal = frame_args(z, cam)
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    fr = device.make_frame(cam_, bg, max_depth, seed, Wd, Ht, traversal=traversal)
    acc = torch.zeros((Ht, Wd, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    for s in range(spp):
        (integ.render_mk if variant == 'mk' else integ.render_wf)(fr, acc, s, 1)
    torch.cuda.synchronize()
    got, counters = acc.cpu().numpy(), integ.read_counters()

    color = z[f'{variant}_color'].reshape(spp, Ht, Wd, 3)
    want = np.zeros((Ht, Wd, 3), np.float32)
    for s in range(spp):
        want = want + color[s]   # f32, sample order: render_sample's accum_buffer += color
    differ = np.argwhere(np.any(got.view(np.uint32) != want.view(np.uint32), axis=-1))
    print(f'{name} {variant}: {len(differ)} of {Ht * Wd} pixels differ; counters {counters}')
    assert len(differ) == 0, (f'{name} {variant}: pixel (x, y) = ({differ[0][1]}, {differ[0][0]}): '
                              f'GPU {got[tuple(differ[0])]!r}, reference text {want[tuple(differ[0])]!r}')
    recorded = {'segments': int(z[f'{variant}_nseg'].sum()), 'medium': int(z[f'{variant}_medium'].sum()),
                'paths': spp * Ht * Wd, 'rr': int(z[f'{variant}_rr'].sum()),
                'depth_cap': int(z[f'{variant}_cap'].sum())}
    assert counters == recorded
