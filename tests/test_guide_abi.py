"""CPU tests of the guide ABI (include/ptmi_guide.h): its symbols are in the
library and in ptmi.guide's own table and in neither of the other two ABIs',
every rejected argument returns before a HIP call with its message, and the
guided denoiser's shared arithmetic (csrc/pt_denoise_math.hpp, run on the CPU by
csrc/denoise_check.cpp, which `make guide_check` builds too) equals the numpy
reference (guide_helpers) bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_helpers as dh
import guide_helpers as gh
from ptmi import _lib, guide, post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_guide_header_symbols_are_exported_and_bound():
    txt = header('ptmi_guide.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert {'ptmi_guide_trace', 'ptmi_denoise_guided'} <= syms
    assert syms == set(guide.EXPORTS)
    lib = guide.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert int(re.search(r'#define PTMI_GUIDE_VERSION (\d+)', txt).group(1)) == guide.GUIDE_VERSION == 1
    assert int(re.search(r'#define PTMI_DN_DEMODULATE (\d+)', txt).group(1)) == guide.DN_DEMODULATE
    # the other two ABIs do not know them, and stay at their versions
    assert not syms & set(_lib.EXPORTS) and not syms & set(post.EXPORTS)
    for other in ('ptmi.h', 'ptmi_post.h'):
        assert 'ptmi_guide' not in header(other) and 'denoise_guided' not in header(other)
    assert post.POST_VERSION == 1
    assert C.sizeof(guide.GuidedParams) == 24


# ------------------------------------------------- rejected arguments: the filter
def call(lib, accum=64, stats=1 << 12, guides=1 << 14, width=16, height=8, ws=256, ws_bytes=1 << 20, out=1 << 16,
         var=None, null_params=False, **prm):
    p = guide.params(**prm)
    return lib.ptmi_denoise_guided(C.c_void_p(accum), C.c_void_p(stats), C.c_void_p(guides), width, height,
                                   None if null_params else C.byref(p), C.c_void_p(ws), ws_bytes, C.c_void_p(out),
                                   C.c_void_p(var), None)


N = 16 * 8


@pytest.mark.parametrize('kw,msg', [
    # every case ptmi_denoise rejects
    (dict(accum=None), 'accum is NULL'),
    (dict(stats=None), 'stats NULL/misaligned'),
    (dict(stats=(1 << 12) + 8), 'stats NULL/misaligned'),
    (dict(ws=None), 'workspace NULL/misaligned'),
    (dict(ws=264), 'workspace NULL/misaligned'),
    (dict(out=None), 'out_rgb is NULL'),
    (dict(width=0), 'bad image size'),
    (dict(height=-3), 'bad image size'),
    (dict(width=65536, height=32768, ws_bytes=1 << 40), 'bad image size'),  # 2^31 pixels
    (dict(iterations=-1), 'iterations'),
    (dict(iterations=9), 'iterations'),
    (dict(sigma=-0.5), 'sigma must'),
    (dict(sigma=float('nan')), 'sigma must'),
    (dict(ws_bytes=2 * 16 * N - 1), 'workspace too small'),
    (dict(out=64), 'out_rgb aliases accum'),
    (dict(out=64 + 12 * N - 4), 'out_rgb aliases accum'),
    # the guided call's own
    (dict(guides=None), 'guides NULL/misaligned'),
    (dict(guides=(1 << 14) + 4), 'guides NULL/misaligned'),
    (dict(null_params=True), 'params is NULL'),
    (dict(out=(1 << 12) + 16 * N - 4), 'out_rgb aliases stats'),
    (dict(out=(1 << 14) + 32 * N - 4), 'guides aliases out_rgb'),
    (dict(guides=(1 << 16) + 12 * N - 16), 'guides aliases out_rgb'),
    (dict(var=(1 << 14) - 4 * N + 4), 'guides aliases out_var'),
    (dict(sigma_z=-1.0), 'sigma_z'),
    (dict(sigma_z=float('nan')), 'sigma_z'),
    (dict(sigma_a=-1e-3), 'sigma_a'),
    (dict(sigma_a=float('nan')), 'sigma_a'),
    (dict(normal_power_log2=-1), 'normal_power_log2'),
    (dict(normal_power_log2=8), 'normal_power_log2'),
])
def test_denoise_guided_rejects_bad_arguments_before_touching_device(kw, msg):
    lib = guide.load()
    assert call(lib, **kw) == _lib.PTMI_EINVAL
    assert msg in lib.ptmi_last_error().decode()
    assert lib.ptmi_last_error().decode().startswith('denoise_guided: ')


@pytest.mark.parametrize('flags', [2, 3, -2, 1 << 30])
def test_unknown_flag_bits_are_rejected(flags):
    lib = guide.load()
    p = guide.params()
    p.flags = flags
    rc = lib.ptmi_denoise_guided(C.c_void_p(64), C.c_void_p(1 << 12), C.c_void_p(1 << 14), 16, 8, C.byref(p),
                                 C.c_void_p(256), 1 << 20, C.c_void_p(1 << 16), None, None)
    assert rc == _lib.PTMI_EINVAL and 'unknown flag bits' in lib.ptmi_last_error().decode()


def test_lds_switch_validates():
    assert guide.set_lds_max_step(2) == 2  # the default
    lib = guide.load()
    assert lib.ptmi_denoise_guided_set_lds_max_step(3) == _lib.PTMI_EINVAL
    assert lib.ptmi_denoise_guided_set_lds_max_step(-1) == _lib.PTMI_EINVAL
    assert guide.set_lds_max_step(2) == 2
    assert post.set_lds_max_step(2) == 2  # ptmi_denoise's own switch is another


# ------------------------------------------------- rejected arguments: the trace
def _scene_and_frame():
    """An empty scene's view (no device memory is touched before the checks) and a whole 16 x 8 frame."""
    v = _lib.SceneView()
    v.perlin_vec, v.perlin_perm = 256, 256
    f = _lib.Frame()
    f.width, f.height, f.x0, f.y0, f.w, f.h = 16, 8, 0, 0, 16, 8
    f.band_rows, f.band_stride, f.band_offset = 1, 1, 0
    f.max_depth = 50
    f.traversal = _lib.TRAVERSALS['stack']
    return v, f


@pytest.mark.parametrize('edit,msg', [
    (lambda v, f: dict(guides=None), 'guides NULL/misaligned'),
    (lambda v, f: dict(guides=(1 << 14) + 8), 'guides NULL/misaligned'),
    (lambda v, f: setattr(f, 'w', 8), 'windowed'),
    (lambda v, f: (setattr(f, 'y0', 2), setattr(f, 'h', 6)), 'windowed'),
    (lambda v, f: (setattr(f, 'band_stride', 2), setattr(f, 'band_offset', 1)), 'banded'),
    (lambda v, f: setattr(f, 'traversal', 7), 'unknown traversal'),
    (lambda v, f: setattr(f, 'width', 0), 'bad window'),
    (lambda v, f: setattr(v, 'num_spheres', -1), 'negative scene counts'),
    (lambda v, f: dict(scene=None), 'scene is NULL'),
    (lambda v, f: dict(frame=None), 'frame is NULL'),
])
def test_guide_trace_rejects_bad_arguments_before_touching_device(edit, msg):
    lib = guide.load()
    v, f = _scene_and_frame()
    kw = edit(v, f)
    kw = kw if isinstance(kw, dict) else {}
    scene = None if 'scene' in kw else C.byref(v)
    frame = None if 'frame' in kw else C.byref(f)
    rc = lib.ptmi_guide_trace(scene, frame, C.c_void_p(kw.get('guides', 1 << 14)), None)
    assert rc == _lib.PTMI_EINVAL
    assert msg in lib.ptmi_last_error().decode()


# ------------------------------------------------- the shared arithmetic on the CPU
@pytest.fixture(scope='module')
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('dng') / 'guide_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'guide_check', f'GUIDE_CHECK={exe}'], check=True)
    return exe


def run_check(exe, tmp_path, accum, stats, guides, iterations, sigma, sigma_z, sigma_a, npow, demodulate):
    h, w = stats.shape[:2]
    paths = [str(tmp_path / n) for n in ('accum.f32', 'stats.f32', 'guides.f32', 'rgb.f32', 'var.f32')]
    accum.tofile(paths[0])
    stats.tofile(paths[1])
    guides.tofile(paths[2])
    args = [str(w), str(h), str(iterations)] + [repr(float(np.float32(s))) for s in (sigma, sigma_z, sigma_a)]
    r = subprocess.run([exe] + args + [str(npow), str(int(demodulate))] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(paths[3], np.float32).reshape(h, w, 3), np.fromfile(paths[4], np.float32).reshape(h, w)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def inputs(w, h):
    accum, stats, invalid = dh.synthetic(w, h, seed=w * 1000 + h)
    return accum, stats, gh.synthetic_guides(w, h, seed=w * 1000 + h), invalid


# (w, h, iterations, sigma, sigma_z, sigma_a, normal_power_log2, demodulate)
CASES = [
    (13, 11, 5, 4.0, 0.1, 0.2, 5, True), (13, 11, 5, 4.0, 0.1, 0.2, 5, False),
    (70, 37, 5, 4.0, 0.1, 0.2, 5, True), (70, 37, 3, 4.0, 0.1, 0.2, 0, False),
    (64, 64, 5, 4.0, 0.1, 0.2, 7, True), (64, 64, 8, 8.0, 0.1, 0.2, 5, False),
    (70, 37, 8, 4.0, 0.1, 0.2, 7, True), (70, 37, 5, 4.0, 0.0, 0.0, 5, True),
    (13, 11, 0, 4.0, 0.1, 0.2, 5, True), (13, 11, 0, 4.0, 0.1, 0.2, 5, False),
    (13, 11, 3, 0.0, 0.0, 0.0, 0, False),
    (1, 1, 3, 4.0, 0.1, 0.2, 5, True), (1, 1, 0, 4.0, 0.1, 0.2, 7, False),
    (5, 1, 5, 1.5, 0.1, 0.2, 0, True), (5, 1, 8, 4.0, 0.0, 0.0, 7, False),
]


@pytest.mark.parametrize('w,h,iterations,sigma,sigma_z,sigma_a,npow,demodulate', CASES)
def test_check_program_equals_numpy_reference(check_exe, tmp_path, w, h, iterations, sigma, sigma_z, sigma_a, npow,
                                              demodulate):
    accum, stats, guides, invalid = inputs(w, h)
    rgb, var = run_check(check_exe, tmp_path, accum, stats, guides, iterations, sigma, sigma_z, sigma_a, npow,
                         demodulate)
    ref_rgb, ref_var = gh.denoise_guided(accum, stats, guides, iterations, sigma, sigma_z, sigma_a, npow, demodulate)
    assert same(rgb, ref_rgb)
    assert same(var, ref_var)
    bad = np.zeros((h, w), bool)
    for p in invalid:
        bad[p] = True
    if w * h > 2:  # the invalid pixels poison nobody
        assert not bad.all()
        assert np.isfinite(rgb[~bad]).all() and np.isfinite(var[~bad]).all()


def test_reference_with_neutral_guides_is_the_unguided_filter():
    """What ties the two references together: with one flat surface everywhere
    (equal depth, albedo and unit normal) and no demodulation every guide
    factor is exactly 1, so the guided filter is ptmi_denoise's."""
    accum, stats, _ = dh.synthetic(70, 37, seed=70037)
    g = np.zeros((37, 70, 8), np.float32)
    g[...] = (0, 0, 1, 2.5, 0.5, 0.5, 0.5, 1)
    rgb, var = gh.denoise_guided(accum, stats, g, 5, 4.0, 0.1, 0.2, 5, False)
    ref_rgb, ref_var = dh.denoise(accum, stats, 5, 4.0)
    assert same(rgb, ref_rgb) and same(var, ref_var)


def test_reference_stops_at_guide_edges():
    """What the helper itself must do to be a reference worth matching. Where a
    guide term is exactly 0 across a line (a depth step, an albedo step, hit
    against miss, perpendicular normals) no tap crosses it: changing the input
    on one side leaves the output on the other side bit for bit as it was.
    With flat guides the change leaks across, and a crease leaks less the more
    often the normal term is squared."""
    h, w = 24, 32
    accum, stats, _ = dh.synthetic(w, h, seed=11)
    accum[:], stats[..., 0], stats[..., 2] = 16 * 0.5, 16, 0.02 * 15  # flat, equally bright, all valid
    stats[..., 1] = 0.5
    other = accum.copy()
    other[:, w // 2:] += np.float32(16 * 0.01)  # inside the noise estimate: no luminance edge
    flat = np.zeros((h, w, 8), np.float32)
    flat[...] = (0, 0, 1, 2.0, 0.5, 0.5, 0.5, 1)

    def leak(guides, **kw):
        c0, v0 = gh.denoise_guided(accum, stats, guides, 5, 4.0, demodulate=False, **kw)
        c1, v1 = gh.denoise_guided(other, stats, guides, 5, 4.0, demodulate=False, **kw)
        assert np.isfinite(c0).all() and np.isfinite(c1).all()
        return float(np.abs(c1[:, :w // 2] - c0[:, :w // 2]).max())

    assert leak(flat) > 1e-3
    for ch, val in ((3, 4.0), (4, 0.9), (7, 0.0), (slice(0, 3), (1, 0, 0))):
        g = flat.copy()
        g[:, w // 2:, ch] = val
        assert leak(g) == 0.0, ch
    g = flat.copy()
    g[:, w // 2:, 0:3] = (0.6, 0, 0.8)  # a crease: dot 0.8, 0.8 ** 32 after five squarings
    assert 0.0 < leak(g, normal_power_log2=5) < 0.01 * leak(g, normal_power_log2=0)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the 13x11 case."""
    exe = str(tmp_path / 'guide_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'guide_check', f'GUIDE_CHECK={exe}',
                    'GUIDE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    accum, stats, guides, _ = inputs(13, 11)
    rgb, var = run_check(exe, tmp_path, accum, stats, guides, 5, 4.0, 0.1, 0.2, 5, True)
    ref_rgb, ref_var = gh.denoise_guided(accum, stats, guides, 5, 4.0, 0.1, 0.2, 5, True)
    assert same(rgb, ref_rgb) and same(var, ref_var)
