"""CPU tests of the post-processing ABI (include/ptmi_post.h): its symbols are
in the library and in ptmi.post's own table and nowhere in ptmi.h's, every
rejected argument of ptmi_denoise returns before a HIP call with its message,
the workspace formula, and the denoiser's shared arithmetic
(csrc/pt_denoise_math.hpp, run on the CPU by csrc/denoise_check.cpp) against the
numpy reference (denoise_helpers) bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_helpers as dh
from ptmi import _lib, post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_post_header_symbols_are_exported_and_bound():
    txt = header('ptmi_post.h')
    syms = sorted(set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error', 'ptmi_tonemap'})
    assert 'ptmi_denoise' in syms and 'ptmi_denoise_workspace_bytes' in syms
    assert set(syms) == set(post.EXPORTS)
    lib = post.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert int(re.search(r'#define PTMI_POST_VERSION (\d+)', txt).group(1)) == post.POST_VERSION == 1
    # the integrator's ABI does not know them
    assert not set(syms) & set(_lib.EXPORTS)
    assert 'denoise' not in header('ptmi.h')


def call(lib, accum=64, stats=64, width=16, height=8, iterations=5, sigma=4.0, ws=256, ws_bytes=1 << 20, out=1 << 16,
         var=None):
    return lib.ptmi_denoise(C.c_void_p(accum), C.c_void_p(stats), width, height, iterations, sigma, C.c_void_p(ws),
                            ws_bytes, C.c_void_p(out), C.c_void_p(var), None)


@pytest.mark.parametrize('kw,msg', [
    (dict(accum=None), 'accum is NULL'),
    (dict(stats=None), 'stats NULL/misaligned'),
    (dict(stats=72), 'stats NULL/misaligned'),
    (dict(ws=None), 'workspace NULL/misaligned'),
    (dict(ws=264), 'workspace NULL/misaligned'),
    (dict(out=None), 'out_rgb is NULL'),
    (dict(width=0), 'bad image size'),
    (dict(height=-3), 'bad image size'),
    (dict(width=65536, height=32768, ws_bytes=1 << 40), 'bad image size'),  # 2^31 pixels
    (dict(iterations=-1), 'iterations'),
    (dict(iterations=9), 'iterations'),
    (dict(sigma=-0.5), 'sigma'),
    (dict(sigma=float('nan')), 'sigma'),
    (dict(ws_bytes=2 * 16 * 16 * 8 - 1), 'workspace too small'),
    (dict(out=64), 'out_rgb aliases accum'),
    (dict(out=64 + 12 * 16 * 8 - 4), 'out_rgb aliases accum'),
])
def test_denoise_rejects_bad_arguments_before_touching_device(kw, msg):
    lib = post.load()
    assert call(lib, **kw) == _lib.PTMI_EINVAL
    assert msg in lib.ptmi_last_error().decode()


def test_workspace_bytes():
    lib = post.load()
    for w, h in ((1, 1), (13, 11), (70, 37), (800, 800), (3840, 2160), (46340, 46340)):
        assert lib.ptmi_denoise_workspace_bytes(w, h) == (2 * 16 * w * h + 255) // 256 * 256
        assert post.workspace_bytes(w, h) == lib.ptmi_denoise_workspace_bytes(w, h)
    assert lib.ptmi_denoise_workspace_bytes(2 ** 31 - 1, 1) == (32 * (2 ** 31 - 1) + 255) // 256 * 256
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
        assert lib.ptmi_denoise_workspace_bytes(w, h) == 0
        assert 'bad image size' in lib.ptmi_last_error().decode()
    with pytest.raises(_lib.PtmiError):
        post.workspace_bytes(0, 4)


def test_lds_switch_validates():
    assert post.set_lds_max_step(2) == 2  # the default
    lib = post.load()
    assert lib.ptmi_denoise_set_lds_max_step(3) == _lib.PTMI_EINVAL
    assert lib.ptmi_denoise_set_lds_max_step(-1) == _lib.PTMI_EINVAL
    assert post.set_lds_max_step(2) == 2


# ------------------------------------------------- the shared arithmetic on the CPU
@pytest.fixture(scope='module')
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('dn') / 'denoise_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'denoise_check', f'DENOISE_CHECK={exe}'], check=True)
    return exe


def run_check(exe, tmp_path, accum, stats, iterations, sigma):
    h, w = stats.shape[:2]
    paths = [str(tmp_path / n) for n in ('accum.f32', 'stats.f32', 'rgb.f32', 'var.f32')]
    accum.tofile(paths[0])
    stats.tofile(paths[1])
    r = subprocess.run([exe, str(w), str(h), str(iterations), repr(float(sigma))] + paths, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(paths[2], np.float32).reshape(h, w, 3), np.fromfile(paths[3], np.float32).reshape(h, w)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('w,h,iterations,sigma', [
    (13, 11, 5, 4.0), (70, 37, 5, 4.0), (64, 64, 5, 4.0), (300, 200, 8, 4.0),
    (13, 11, 0, 4.0), (70, 37, 3, 0.0), (1, 1, 2, 4.0), (5, 1, 4, 1.5),
])
def test_check_program_equals_numpy_reference(check_exe, tmp_path, w, h, iterations, sigma):
    accum, stats, invalid = dh.synthetic(w, h, seed=w * 1000 + h)
    rgb, var = run_check(check_exe, tmp_path, accum, stats, iterations, sigma)
    ref_rgb, ref_var = dh.denoise(accum, stats, iterations, sigma)
    assert same(rgb, ref_rgb)
    assert same(var, ref_var)
    # the invalid pixels pass through as loaded and poison nobody
    c0, v0 = dh.load(accum, stats)
    bad = np.zeros((h, w), bool)
    for p in invalid:
        bad[p] = True
        assert same(rgb[p], c0[p]) and same(var[p], v0[p])
    if w * h > 2:
        assert not bad.all()
        assert np.isfinite(rgb[~bad]).all() and np.isfinite(var[~bad]).all()


def test_reference_filters_and_keeps_the_edge():
    """What the helper itself must do to be a reference worth matching: noise
    goes down inside the flat halves, the hard edge stays, the variance it
    claims shrinks."""
    accum, stats, _ = dh.synthetic(64, 64, seed=7)
    for y, x in zip(*np.nonzero(stats[..., 0] < 2)):  # an unknown variance (1e10f) spreads to all it reaches:
        accum[y, x], stats[y, x] = accum[y, x - 1], stats[y, x - 1]  # measured here without the n = 0, 1 pixels
    c0, v0 = dh.load(accum, stats)
    c, v = dh.denoise(accum, stats, 5, 4.0)
    flat = (slice(2, 24), slice(40, 62))  # right of the edge, away from the special pixels
    assert c[flat].std(axis=(0, 1)).max() < 0.5 * c0[flat].std(axis=(0, 1)).max()
    assert np.median(v[flat]) < 0.2 * np.median(v0[flat])
    left, right = c[2:24, 20:30].mean(axis=(0, 1)), c[2:24, 34:44].mean(axis=(0, 1))
    assert abs(left[2] - 0.2) < 0.05 and abs(right[2] - 0.9) < 0.05


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the 13x11 case."""
    exe = str(tmp_path / 'denoise_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'denoise_check', f'DENOISE_CHECK={exe}',
                    'DENOISE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    accum, stats, _ = dh.synthetic(13, 11, seed=13011)
    rgb, var = run_check(exe, tmp_path, accum, stats, 5, 4.0)
    ref_rgb, ref_var = dh.denoise(accum, stats, 5, 4.0)
    assert same(rgb, ref_rgb) and same(var, ref_var)
