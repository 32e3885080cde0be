"""GPU: the megakernel's inline enclosing-medium-shell shortcut (SHELL kernels,
pt_megakernel.hip) against the CPU oracle, which traces every exit search and
every escape segment through the BVH: accumulators bit-identical (L-inf 0) and
all five counters equal, on 32x32 frames at 8 spp.

R = 100 is the shell whose exit searches all fall back to shading the shell as
a surface (t_entry + 1e-4 > t_entry), R = 5000 the one that passes through and
escapes, as vol2's fog does (tests/shell_scenes.py); max_depth 2 and 3 put the
depth cap on the passthrough and on the escape segment."""
import pytest

import shell_scenes as ss

pytestmark = pytest.mark.gpu

SPP = 8


def check(R, cam, max_depth, mode, traversal='stack', shell=None):
    g, gst = ss.gpu_accum(R, cam, SPP, max_depth, mode, traversal, shell)
    o, ost = ss.oracle_accum(R, cam, SPP, max_depth, 'wf' if mode == 'wf' else 'mk', traversal)
    print(f'R={R} {cam} depth={max_depth} {mode} {traversal}: gpu={gst} oracle={ost}')
    assert gst == ost
    assert ss.same_bits(g, o)
    return g, gst


@pytest.mark.parametrize('mode', ['staged', 'overlapped', 'direct', 'listed'])
@pytest.mark.parametrize('max_depth', [50, 2, 3])
@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_shell_scene(R, max_depth, mode):
    _, st = check(R, 'inside', max_depth, mode)
    assert st['medium'] > 0 and (max_depth == 50 or st['depth_cap'] > 0)


@pytest.mark.parametrize('cam', ['pole+x', 'pole-y', 'pole+z'])
@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_poles(R, cam):
    _, st = check(R, cam, 50, 'staged')
    assert st['medium'] >= st['paths']  # every camera ray ends on the shell


@pytest.mark.parametrize('mode', ['staged', 'direct'])
def test_small_shell_falls_back_to_surface_shading(mode):
    check(1.0, 'inside', 50, mode)


@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_failed_gate_takes_the_ordinary_path(R):
    check(R, 'gate', 50, 'staged')


@pytest.mark.parametrize('R', [100.0, 5000.0])
def test_without_the_hint_same_bits(R):
    g, gst = check(R, 'inside', 50, 'staged')
    g0, gst0 = check(R, 'inside', 50, 'staged', shell=0)
    assert gst == gst0 and ss.same_bits(g, g0)


@pytest.mark.parametrize('mode,traversal', [('staged', 'stackless'), ('direct', 'stackless'), ('wf', 'stack')])
def test_other_kernels_ignore_the_hint(mode, traversal):
    check(5000.0, 'inside', 50, mode, traversal)
