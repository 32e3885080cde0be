"""CPU: the shapes of tests/test_gpu_frame_scale.py (its SHAPES table, and the
frame it relies on in validate_helpers.FRAMES) against the constants they are
meant to lie beyond, read out of the source text: kBlock (pt_device.hpp),
kImgTile and capped_grid's 4096 blocks (pt_image.hpp), the 2048 blocks of
launch_stats_resolve and kScanBlock (pt_adaptive.hip), kVdMaxRadius
(pt_validate_math.hpp). A raised cap or a changed block fails here, so that the
GPU cases do not quietly run on the first trip of every loop; so does a
constant that is no longer where it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_frame_scale as fs
import validate_helpers as vh
from ptmi import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
SHAPES = fs.SHAPES


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def find(name, pattern):
    """The integer group(s) of the one match of ``pattern`` in csrc/``name``."""
    found = re.findall(pattern, source(name))
    assert len(found) == 1, f'{name}: {pattern!r} matches {len(found)} times'
    groups = found[0] if isinstance(found[0], tuple) else (found[0],)
    return tuple(int(g) for g in groups)


def constants():
    k = {'kBlock': find('pt_device.hpp', r'constexpr int kBlock = (\d+);')[0],
         'kImgTile': find('pt_image.hpp', r'constexpr int kImgTile = (\d+);')[0],
         'kScanBlock': find('pt_adaptive.hip', r'constexpr int kScanBlock = (\d+);')[0],
         'kVdMaxRadius': find('pt_validate_math.hpp', r'constexpr int32_t kVdMaxRadius = (\d+);')[0]}
    # capped_grid: return dim3((unsigned)(g > 4096 ? 4096 : g));
    cap = find('pt_image.hpp', r'inline dim3 capped_grid\(int64_t n, int block\) \{[^}]*?g > (\d+) \? (\d+) : g')
    assert cap[0] == cap[1]
    k['flat_cap'] = cap[0]
    # launch_stats_resolve: if (gr > 2048) gr = 2048;
    cap = find('pt_adaptive.hip', r'hipError_t launch_stats_resolve\([^{]*\{[^}]*?if \(gr > (\d+)\) gr = (\d+);')
    assert cap[0] == cap[1]
    k['resolve_cap'] = cap[0]
    assert len(re.findall(r'constexpr int kImgBlock = kImgTile \* kImgTile;', source('pt_image.hpp'))) == 1
    k['kImgBlock'] = k['kImgTile'] ** 2
    return k


K = constants()


def test_every_constant_is_found_and_a_missing_one_fails():
    assert K == {'kBlock': 256, 'kImgTile': 16, 'kImgBlock': 256, 'kScanBlock': 1024, 'kVdMaxRadius': 7,
                 'flat_cap': 4096, 'resolve_cap': 2048}
    with pytest.raises(AssertionError, match='matches 0 times'):
        find('pt_device.hpp', r'constexpr int kBlok = (\d+);')
    with pytest.raises(AssertionError, match='matches 0 times'):
        find('pt_adaptive.hip', r'hipError_t launch_stats_resolve\([^{]*\{[^}]*?if \(gr > (\d+)\) gr = (\d+) ;')


def test_the_kernels_are_launched_on_the_grids_the_shapes_assume():
    abi, dn, ad = source('pt_abi.hip'), source('pt_denoise.hip'), source('pt_adaptive.hip')
    assert 'const dim3 grid = capped_grid(npix, kBlock);' in abi  # the clears
    assert 'const dim3 grid = capped_grid(n, kBlock);' in abi  # the tone maps
    assert 'const int64_t n = (int64_t)width * height * 3;' in abi
    assert 'const dim3 flat = capped_grid(npix, kImgBlock), block(kImgBlock);' in dn
    assert dn.count('hipLaunchKernelGGL(dn_load<GUIDED>, flat, block,') == 1
    assert dn.count('hipLaunchKernelGGL(dn_store<GUIDED>, flat, block,') == 1
    assert 'unsigned gr = (unsigned)((nitems + kBlock - 1) / kBlock);' in ad
    assert 'const int64_t nitems = tile_list ? 64ll * n_tiles : (int64_t)npix;' in ad
    assert 'hipLaunchKernelGGL(tile_compact, dim3(1), dim3(kScanBlock),' in ad
    assert 'const int32_t per = (ntiles + kScanBlock - 1) / kScanBlock;' in ad


def frame(width, height, window=None, band=(1, 1, 0)):
    cam = {k: np.zeros(3, np.float32) for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = 0.0
    return device.make_frame(cam, (0, 0, 0), 50, 0, width, height, window, band)


def grid(f):
    """ptmi_mk_tile_grid: it returns before any HIP call."""
    v = [C.c_int32() for _ in range(4)]
    assert _lib.load().ptmi_mk_tile_grid(C.byref(f), *[C.byref(x) for x in v]) == _lib.PTMI_OK
    return tuple(x.value for x in v)


def owned_pixels(f):
    return f.w * len(device.frame_pixel_rows(f))


# ---------------------------------------------------------------- 1
def test_tile_update_shapes_straddle_one_tile_per_thread():
    scan = K['kScanBlock']
    per = {}
    for (w, h), (tx, ty) in SHAPES['tile_update'].items():
        assert grid(frame(w, h)) == (8, 8, tx, ty)
        nt = tx * ty
        per[w, h], first = fs.compact_runs(nt, scan)
        assert per[w, h] == -(-nt // scan) and first[-1] == nt
    assert per == {(256, 256): 1, (197, 325): 2, (264, 250): 2, (509, 261): 3}
    assert 32 * 32 == scan  # every thread used, one tile each
    assert 25 * 41 == scan + 1 and 197 % 8 and 325 % 8  # the first count past it, on a ragged grid
    _, first = fs.compact_runs(25 * 41, scan)
    assert first[513] - first[512] == 1 and first[513] == first[1024]  # owner 512 holds one tile, the rest none
    assert (33 * 32) % 2 == 0  # whole runs only
    assert 64 * 32 == 2 * scan and 64 * 33 > 2 * scan  # one tile row past per = 2
    _, first = fs.compact_runs(64 * 33, scan)
    assert (np.diff(first) == 0).sum() == scan - 64 * 33 // 3 > 0  # empty owner threads at the end


# ---------------------------------------------------------------- 2
def test_flat_kernel_shapes_reach_the_second_trip():
    threads = K['flat_cap'] * K['kBlock']
    w, h = SHAPES['clear_whole']
    assert (w - 1) * h <= threads < w * h == owned_pixels(frame(w, h))  # one column less stays on the first trip
    b = SHAPES['clear_band']
    f = frame(*b['image'], b['window'], b['band'])
    assert owned_pixels(f) > threads
    assert f.x0 > 0 and f.x0 + f.w <= f.width and f.band_stride > 1  # a window, inside the image, and banded
    assert (w * h) // 2 < threads  # why no band frame of that size fits the whole-frame case's image
    w, h = SHAPES['tonemap']
    assert w * h <= threads < 3 * w * h  # past it by the three elements alone
    assert threads % 3  # a pixel straddles the trips
    w, h = SHAPES['denoise']
    threads = K['flat_cap'] * K['kImgBlock']
    assert (w - 1) * h <= threads < w * h
    lo, hi = fs.trip_band(w, h)
    assert lo <= threads // w < hi  # the band holds the pixel where the first trip ends


# ---------------------------------------------------------------- 3
def test_resolve_shapes_are_past_the_stats_resolve_grid():
    threads = K['resolve_cap'] * K['kBlock']
    w = SHAPES['resolve_width']
    tx, ty = SHAPES['resolve_tiles']
    assert grid(frame(w, w)) == (8, 8, tx, ty) and w % 8 == 4  # a partial right column and bottom row
    assert w * w > threads
    ids = fs.listed_ids(tx * ty, tx)
    assert 64 * len(ids) > threads and len(ids) > 8192 == threads // 64
    assert len(ids) < tx * ty and len(set(ids.tolist())) == len(ids)
    prm = SHAPES['adaptive']
    assert (prm['pass_spp'], prm['min_spp'], prm['max_spp']) == (2, 2, 6)
    assert -(-tx * ty // K['kScanBlock']) == 10  # tile_compact's per in the adaptive loop


# ---------------------------------------------------------------- 4
def unclipped_tiles(w, h, radius, tile):
    """(tx, ty) of the tiles whose halo of ``radius`` lies wholly inside a w x h image."""
    return [(tx, ty) for ty in range(-(-h // tile)) for tx in range(-(-w // tile))
            if tx * tile - radius >= 0 and ty * tile - radius >= 0
            and (tx + 1) * tile + radius <= w and (ty + 1) * tile + radius <= h]


def test_validation_frames_hold_tiles_with_unclipped_halos():
    tile, r = K['kImgTile'], K['kVdMaxRadius']
    assert max(vh.RADII) == r
    assert (80, 50) in vh.FRAMES and 50 % tile and -(-50 // tile) == 4  # a ragged bottom row below two middle rows
    assert unclipped_tiles(80, 50, r, tile) == [(1, 1), (2, 1), (3, 1)]
    assert not unclipped_tiles(48, 27, r, tile)  # the largest frame before it had none
