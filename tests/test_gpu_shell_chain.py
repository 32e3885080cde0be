"""GPU: the megakernel's expanded segment begin over the shell's ancestor chain
(SHELL kernels, pt_megakernel.hip; pt_shell_chain.hpp) against the CPU oracle,
which pops every chain node and the shell's leaf in every traversal:
accumulators bit-identical and all five counters equal, on 32x32 frames at 8
spp and on two 64x64 windows of vol2 at 4 spp.

The scenes (tests/shell_chain_helpers.py): chains of 1, 3 and 5 levels, one of
8 (longer than kShellChainMax: six levels expanded at most, the rest of the
chain pushed as a node), and one of 5 under leaf depth 17, where the 20-slot
kernel has room for 3. R = 100 shades the shell as a surface, R = 5000 passes
through and escapes (tests/shell_scenes.py)."""
import numpy as np
import pytest

import shell_chain_helpers as ch
import shell_scenes as ss
from parity_helpers import BG, fixture

pytestmark = pytest.mark.gpu

SPP = 8


def check(name, R, cam, max_depth, mode, shell=None):
    g, gst = ch.gpu_accum(name, R, cam, SPP, max_depth, mode, shell)
    o, ost = ch.oracle_accum(name, R, cam, SPP, max_depth)
    print(f'{name} R={R} {cam} depth={max_depth} {mode}: gpu={gst} oracle={ost}')
    assert gst == ost
    assert ss.same_bits(g, o)
    return g, gst


@pytest.mark.parametrize('mode', ['staged', 'overlapped', 'direct', 'listed'])
@pytest.mark.parametrize('name', ['c1', 'c3', 'c8', 'sah5'])
def test_chain_scene(name, mode):
    _, st = check(name, 5000.0, 'inside', 50, mode)
    assert st['medium'] > 0


@pytest.mark.parametrize('name', ['c1', 'c3', 'c8', 'sah5'])
def test_chain_scene_surface_shell(name):
    check(name, 100.0, 'inside', 50, 'staged')


@pytest.mark.parametrize('mode', ['staged', 'direct'])
@pytest.mark.parametrize('max_depth', [2, 3])
@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_depth_cap(R, max_depth, mode):
    _, st = check('c3', R, 'inside', max_depth, mode)
    assert st['depth_cap'] > 0


@pytest.mark.parametrize('cam', ['gate', 'pole+x', 'pole-y', 'pole+z'])
@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_cameras(R, cam):
    check('c3', R, cam, 50, 'staged')


@pytest.mark.parametrize('mode', ['staged', 'direct'])
def test_fewer_levels_than_found(mode):
    """Leaf depth 17: the 20-slot kernel expands 3 of the 5 levels and pushes the rest."""
    check('deep', 5000.0, 'inside', 50, mode)


@pytest.mark.parametrize('name', ['c3', 'c8'])
def test_without_the_hint_same_bits(name):
    g, gst = check(name, 5000.0, 'inside', 50, 'staged')
    g0, gst0 = check(name, 5000.0, 'inside', 50, 'staged', shell=0)
    assert gst == gst0 and ss.same_bits(g, g0)


@pytest.mark.parametrize('staged', [True, False])
@pytest.mark.parametrize('window', [(368, 368, 64, 64), (100, 600, 64, 64)])
def test_vol2_windows(window, staged):
    import oracle
    import torch
    from ptmi import device, scene_data as sd
    name, spp = 'vol2_final_scene', 4
    sa, cam = fixture(name), sd.fixture_camera(name, 800)
    W, H = cam['width'], cam['height']
    ofr = oracle.make_frame(cam, BG[name], 50, 0, W, H)
    o = np.zeros((H, W, 3), np.float32)
    ost = oracle.render(oracle.OracleScene(sa), ofr, 'mk', o, window, 0, spp)
    integ = device.Integrator(device.DeviceScene.from_arrays(sa))
    fr = device.make_frame(cam, BG[name], 50, 0, W, H, window)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    integ.reset_counters()
    integ.render_mk(fr, acc, 0, spp, staged=staged)
    torch.cuda.synchronize()
    gst = integ.read_counters()
    assert {k: int(gst[k]) for k in ss.COUNTERS} == {k: int(ost[k]) for k in ss.COUNTERS}
    assert ss.same_bits(acc.cpu().numpy(), o)
