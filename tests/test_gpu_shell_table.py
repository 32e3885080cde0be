"""GPU: the SHELL megakernels with the wave-resident shell table
(pt_megakernel.hip: ShellTable, built in the prologue, read by v_readlane in
converged code; pt_shell_chain.hpp) against the CPU oracle: every pixel
bit-identical and all five counters equal.

Scenes: the synthetic shells of tests/shell_scenes.py at R = 100 (the shell is
shaded as a surface) and R = 5000 (exit search, passthrough, escape), and a
64x64 window of vol2; 64x64 pixels at 4 spp; direct, staged and tile-listed
calls. One case moves primitives, the shell among them, and refits on the
device between two calls: the table is built per launch from the node array,
so the second call must equal the oracle on the updated scene. Two cases
shade with fewer than 64 live lanes (a frame narrower than a tile, a 1-spp
drain): the table is read across lanes, which is only right in converged code
(DESIGN.md §4). The last test runs all of the above in a child process with
the register-stress build (another register allocation of the same kernels)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shell_scenes as ss
import update_helpers as uh
from parity_helpers import BG, fixture

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
STRESS = os.path.join(ROOT, 'path-tracer-python_amd', 'ptmi', '_lib', 'libptmi_stress.so')
SPP = 4
MODES = ('direct', 'staged', 'listed')

_scenes = {}


def scene(name):
    """(SceneArrays, camera, background, window) of a case: 64x64 pixels."""
    from ptmi import scene_data as sd
    if name not in _scenes:
        if name == 'vol2':
            sa, cam = fixture('vol2_final_scene'), sd.fixture_camera('vol2_final_scene', 800)
            _scenes[name] = (sa, cam, BG['vol2_final_scene'], (368, 368, 64, 64))
        else:
            R = float(name[1:])
            _scenes[name] = (ss.shell_arrays(R), ss.shell_camera(R, 'inside', 64), ss.BG, (0, 0, 64, 64))
    return _scenes[name]


_oracle = {}


def oracle_render(key, sa, cam, bg, window, spp):
    import oracle
    if key not in _oracle:
        W, H = cam['width'], cam['height']
        o = np.zeros((H, W, 3), f32)
        st = oracle.render(oracle.OracleScene(sa), oracle.make_frame(cam, bg, 50, 7, W, H), 'mk', o, window, 0, spp)
        o.setflags(write=False)
        _oracle[key] = (o, {k: int(st[k]) for k in ss.COUNTERS})
    return _oracle[key]


def gpu_render(ds, cam, bg, window, spp, mode):
    import torch
    from ptmi import device
    W, H = cam['width'], cam['height']
    integ = device.Integrator(ds)
    assert ds.view.shell != 0
    fr = device.make_frame(cam, bg, 50, 7, W, H, window)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    if mode == 'listed':
        tiles = integ.new_tiles(fr)
        integ.render_mk_stats(fr, acc, integ.new_stats(fr), 0, spp, tiles=(tiles['list'], tiles['n']))
    else:
        integ.render_mk(fr, acc, 0, spp, staged=mode == 'staged')
    torch.cuda.synchronize()
    st = integ.read_counters()
    return acc.cpu().numpy(), {k: int(st[k]) for k in ss.COUNTERS}


def check(name, mode, window=None, spp=SPP):
    from ptmi import device
    sa, cam, bg, win = scene(name)
    window = window or win
    g, gst = gpu_render(device.DeviceScene.from_arrays(sa), cam, bg, window, spp, mode)
    o, ost = oracle_render((name, window, spp), sa, cam, bg, window, spp)
    print(f'{name} {mode} {window} spp={spp}: gpu={gst} oracle={ost}')
    assert gst == ost
    assert ss.same_bits(g, o)
    assert gst['paths'] == window[2] * window[3] * spp
    return gst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['R100', 'R5000', 'vol2'])
def test_table_kernels_equal_the_oracle(name, mode):
    st = check(name, mode)
    assert st['medium'] > 0


@pytest.mark.parametrize('mode', ['direct', 'staged'])
def test_frame_narrower_than_a_tile(mode):
    """5 of a tile's 8 columns and 13 rows: no wave ever has 64 live lanes."""
    check('R5000', mode, window=(0, 0, 5, 13))
    check('vol2', mode, window=(397, 380, 5, 13))


@pytest.mark.parametrize('name', ['R5000', 'vol2'])
def test_one_spp_drain(name):
    """1 spp, staged: each persistent wave takes its units and drains, shading with ever fewer live lanes."""
    check(name, 'staged', spp=1)


@pytest.mark.parametrize('mode', ['staged', 'direct'])
def test_table_follows_a_device_refit(mode):
    """Two calls around update_primitives: the shell moves by 0.05 R (its box,
    every ancestor's box, its sphere and the gate change) and an inner sphere
    moves; the second call equals the oracle on the updated scene."""
    from ptmi import device, scene_data as sd
    sa, cam, bg, win = scene('R5000')
    R = f32(5000.0)
    shell = int(np.argmax(sa.sphere_data[:, 3]))
    assert sa.sphere_data[shell, 3] == R
    inner = next(i for i in range(sa.num_spheres) if i != shell)
    edit = uh.sphere_edit([inner, shell],
                          [sa.sphere_data[inner, 0:3] + np.array([40.0, 25.0, -30.0], f32),
                           sa.sphere_data[shell, 0:3] + f32(0.05) * R * np.array([1.0, -0.5, 0.25], f32)],
                          [sa.sphere_data[inner, 3], R])
    ref = uh.refit(sa, {'spheres': edit})
    assert sd.pack_device(ref).shell != 0  # the moved shell still encloses the scene
    ds = device.DeviceScene.from_arrays(sa)
    g0, st0 = gpu_render(ds, cam, bg, win, SPP, mode)
    o0, ost0 = oracle_render(('R5000', win, SPP), sa, cam, bg, win, SPP)
    assert st0 == ost0 and ss.same_bits(g0, o0)
    ds.update_primitives(spheres=edit)
    assert ds.view.shell != 0
    g1, st1 = gpu_render(ds, cam, bg, win, SPP, mode)
    o1, ost1 = oracle_render(('R5000 moved', win, SPP), ref, cam, bg, win, SPP)
    print(f'refit {mode}: gpu={st1} oracle={ost1}')
    assert st1 == ost1 and ss.same_bits(g1, o1)
    assert not ss.same_bits(o0, o1)


def test_stress_build():
    """Every case above with libptmi_stress.so (the library is loaded once per
    process, so in a child): another register allocation changes no result."""
    assert os.path.exists(STRESS), 'libptmi_stress.so missing: run __graft_entry__.build()'
    p = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider',
                        '-k', 'not stress_build'], env=dict(os.environ, PTMI_LIB=STRESS), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert '15 passed' in p.stdout, p.stdout[-2000:]
