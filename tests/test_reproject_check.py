"""CPU: the temporal reprojection's shared arithmetic (csrc/pt_reproject_math.hpp,
run on the CPU by csrc/reproject_check.cpp) equals the numpy reference
(reproject_helpers) bit for bit, on guides from the numpy guide trace over the
oracle and on tiny synthetic frames, and the same program built with
-fsanitize=address,undefined exits clean. Plus what the reference itself must
do to be worth matching."""
import os
import subprocess

import numpy as np
import pytest

import reproject_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32


@pytest.fixture(scope='module')
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('rp') / 'reproject_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'reproject_check', f'REPROJECT_CHECK={exe}'], check=True)
    return exe


@pytest.fixture(scope='module')
def san_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('rp_san') / 'reproject_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'reproject_check', f'REPROJECT_CHECK={exe}',
                    'REPROJECT_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    return exe


def run_check(exe, tmp_path, cur, prev, gc, gp, accum, stats, prm):
    h, w = stats.shape[:2]
    paths = [str(tmp_path / n) for n in ('in.f32', 'accum.f32', 'stats.f32')]
    rh.pack_input(cur, prev, prm, gc, gp, accum, stats).tofile(paths[0])
    r = subprocess.run([exe, str(w), str(h)] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(paths[1], f32).reshape(h, w, 3), np.fromfile(paths[2], f32).reshape(h, w, 4)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def both(check_exe, san_exe, tmp_path, case, prm=rh.DEFAULTS):
    """The case through the check program and, a second time, through its
    sanitizer build; both bit for bit the numpy reference, whose details are returned."""
    ref_a, ref_s, det = rh.reproject(*case, details=True, **prm)
    for exe in (check_exe, san_exe):
        a, s = run_check(exe, tmp_path, *case, prm)
        assert same(s, ref_s)
        assert same(a, ref_a)
        rh.check_properties(a, s, det, prm['max_history'])
    return ref_a, ref_s, det


@pytest.mark.parametrize('name,width,delta', rh.ORACLE_CASES)
def test_check_program_equals_numpy_reference_on_oracle_guides(check_exe, san_exe, tmp_path, name, width, delta):
    case = rh.oracle_case(name, width, delta)
    _, ref_s, det = both(check_exe, san_exe, tmp_path, case)
    frac = float((ref_s[..., 0] > 0).mean())
    print(f'{name} {width} px delta {delta}: history on {100 * frac:.1f} % of the pixels')
    if delta == (600, 0):  # from the other side: the points are in the old frame, but a wall shows its back
        assert det['valid'].any() and frac == 0.0
    elif delta == (40, 20):
        assert 0.3 < frac < 0.98  # part of the frame is new, part is disoccluded
    else:
        assert frac > 0.8


@pytest.mark.parametrize('width,height', rh.FLAT_CASES)
def test_check_program_equals_numpy_reference_on_tiny_frames(check_exe, san_exe, tmp_path, width, height):
    _, ref_s, _ = both(check_exe, san_exe, tmp_path, rh.flat_case(width, height))
    assert (ref_s[..., 0] > 0).any()


def test_points_behind_the_previous_camera_have_no_history(check_exe, san_exe, tmp_path):
    """lam <= 0: the previous camera stood past the wall the current one sees
    (hits), and looked the other way for the one miss pixel."""
    cur, prev, gc, gp, accum, stats = rh.flat_case(3, 2)
    prev = rh.flat_camera(3, 2, (0.0, 0.0, -5.0))  # the wall is at z = -3
    ref_a, ref_s, det = both(check_exe, san_exe, tmp_path, (cur, prev, gc, gp, accum, stats))
    hit = gc[..., 7] != 0
    assert (det['lam'][hit] < 0).all() and not det['valid'][hit].any()
    assert not ref_s[hit].any() and not ref_a[hit].any()


@pytest.mark.parametrize('prm', [dict(max_history=1.0, sigma_z=0.0, normal_min=1.0, sigma_a=0.0),
                                 dict(max_history=8.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2),
                                 dict(max_history=float(1 << 24), sigma_z=10.0, normal_min=-1.0, sigma_a=10.0)])
def test_check_program_equals_numpy_reference_at_other_parameters(check_exe, san_exe, tmp_path, prm):
    _, ref_s, _ = both(check_exe, san_exe, tmp_path, rh.oracle_case('cornell_smoke', 33, (4, 2)), prm)
    assert (ref_s[..., 0] <= prm['max_history']).all()


def test_a_previous_camera_without_delta_u_leaves_no_history(check_exe, san_exe, tmp_path):
    cur, prev, gc, gp, accum, stats = rh.oracle_case('cornell_box', 33, (4, 2))
    prev = dict(prev, delta_u=np.zeros(3, f32))  # a = x / 0: NaN or infinite
    ref_a, ref_s, det = both(check_exe, san_exe, tmp_path, (cur, prev, gc, gp, accum, stats))
    assert not det['valid'].any()
    assert not ref_a.any() and not ref_s.any()


def test_reference_with_the_camera_not_moved_keeps_every_countable_pixel():
    """What the helper must do to be a reference worth matching: with the same
    camera and the same guides a surface point lands on its own pixel up to
    rounding, so every hit or miss pixel whose own history is countable has
    history, and a pixel deep inside a flat region gets its own colour back."""
    cur, prev, gc, gp, accum, stats = rh.oracle_case('cornell_box', 48, (0, 0))
    a, s, det = rh.reproject(cur, prev, gc, gp, accum, stats, details=True, **rh.DEFAULTS)
    ok = rh.countable(accum, stats) & np.isfinite(gc[..., 3]) & np.isfinite(gp[..., 3])
    assert ok.mean() > 0.95
    assert (s[..., 0][ok] > 0).all()
    assert np.abs(det['ab'][ok] - np.stack(np.meshgrid(np.arange(48), np.arange(48)), -1)[ok]).max() < 1e-2
    # the cap: no count above max_history, and counts below it are carried as they are
    n0 = stats[..., 0]
    assert (s[..., 0] <= 32).all() and (s[..., 0][ok & (n0 == 16)] >= 15).all()
    with np.errstate(all='ignore'):
        back = a / s[..., 0:1]
        own = accum / n0[..., None]
    near = ok & (np.abs(back - own).max(-1) <= 1e-3 * np.abs(own).max(-1))
    assert near.mean() > 0.5


def test_reference_rejects_another_surface():
    """A tap is counted only on the same surface: moving the previous frame's
    depth, turning its normals or changing its albedo beyond the tolerances
    leaves no history on hit pixels; misses keep theirs."""
    cur, prev, gc, gp, accum, stats = rh.oracle_case('cornell_box', 33, (0, 0))
    hit = gc[..., 7] != 0
    base = rh.reproject(cur, prev, gc, gp, accum, stats)[1][..., 0] > 0
    assert base[hit].mean() > 0.9
    for ch, edit in ((3, lambda x: x * f32(1.5)), (slice(0, 3), lambda x: -x), (4, lambda x: x + f32(0.5))):
        g2 = gp.copy()
        g2[..., ch] = edit(g2[..., ch])
        has = rh.reproject(cur, prev, gc, g2, accum, stats)[1][..., 0] > 0
        assert not has[hit].any(), ch
        assert np.array_equal(has[~hit], base[~hit])
