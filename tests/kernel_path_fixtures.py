"""Loading of the tests/golden/kernel_paths_<scene>.npz fixtures (gen_kernel_paths.py):
what the reference's own kernel text computed, path by path, for tiny frames.
Shared by test_kernel_paths.py (oracle) and test_gpu_kernel_paths.py (HIP)."""
import glob
import json
import os

import numpy as np

from ptmi import scene_data as sd

GOLDEN = sd.golden_dir()
FIXTURES = sorted(os.path.basename(p)[len('kernel_paths_'):-len('.npz')]
                  for p in glob.glob(os.path.join(GOLDEN, 'kernel_paths_*.npz')))
SCENES = ('chainx', 'coincident', 'depthcap', 'materials', 'media', 'stackless')
VARIANTS = ('mk', 'wf')

_cache = {}


def load(name):
    """(npz, SceneArrays, camera upload dict) of a kernel-path fixture."""
    if name not in _cache:
        path = os.path.join(GOLDEN, f'kernel_paths_{name}.npz')
        z = np.load(path)
        names = json.loads(str(z['images']))   # one per image texture; the earthmap is the only image
        assert all(n == 'earthmap' for n in names), names
        images = [sd.load_earthmap() for _ in names]
        sa = sd.SceneArrays.from_npz(path, images=images)
        cam = {k: np.asarray(z['cam_' + k], np.float32) for k in
               ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
        cam['defocus_angle'] = float(z['cam_defocus_angle'])
        cam['width'], cam['height'] = (int(v) for v in z['cam_size'])
        _cache[name] = (z, sa, cam)
    return _cache[name]


def frame_args(z, cam):
    return (cam, tuple(float(x) for x in z['bg']), int(z['max_depth']), int(z['seed']), cam['width'], cam['height'],
            str(z['traversal']))
