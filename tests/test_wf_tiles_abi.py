"""CPU tests of the tile-listed wavefront ABI (include/ptmi_wf_tiles.h): its
symbol is in the library and in ptmi.wf_tiles's own table and in none of the
other four ABIs', and every rejected argument returns PTMI_EINVAL before a HIP
call with its message. No device is needed: the pointers are never
dereferenced."""
import ctypes as C
import os
import re

import numpy as np

from ptmi import _lib, device, guide, post, temporal, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def make_frame(**kw):
    cam = {k: np.zeros(3, np.float32) for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = 0.0
    args = dict(cam=cam, bg=(0, 0, 0), max_depth=50, seed=0, width=16, height=8)
    args.update(kw)
    return device.make_frame(**args)


def empty_scene():
    v = _lib.SceneView()
    v.perlin_vec = v.perlin_perm = 16
    return v


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_wf_tiles.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_wf_render_tiles_stats'} == set(wf_tiles.EXPORTS) == set(wf_tiles.SIGNATURES)
    lib = wf_tiles.load()
    assert hasattr(lib, 'ptmi_wf_render_tiles_stats')
    assert int(re.search(r'#define PTMI_WF_TILES_VERSION (\d+)', txt).group(1)) == wf_tiles.WF_TILES_VERSION == 1
    # the four existing signature tables do not know it, nor do their headers
    for other in (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES):
        assert 'ptmi_wf_render_tiles_stats' not in other
    for other in ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h'):
        assert 'ptmi_wf_render_tiles_stats' not in header(other) and 'ptmi_wf_tiles' not in header(other)
    restype, argtypes = wf_tiles.SIGNATURES['ptmi_wf_render_tiles_stats']
    assert restype is C.c_int and len(argtypes) == 12
    # ptmi_wf_render_stats with (tile_list, n_tiles) after stats
    base = _lib.SIGNATURES['ptmi_wf_render_stats'][1]
    assert argtypes == base[:6] + [C.c_void_p, C.c_int32] + base[6:]


def test_render_tiles_stats_rejects_bad_arguments_before_touching_device():
    lib = wf_tiles.load()
    f, v = make_frame(), empty_scene()  # 16 x 8: 2 tiles, 128 pixels

    def call(ws=256, ws_bytes=1 << 40, acc=16, st=32, tl=64, nt=1, s0=0, sc=1, scene=v, frame=f):
        return lib.ptmi_wf_render_tiles_stats(C.byref(scene) if scene is not None else None,
                                              C.byref(frame) if frame is not None else None,
                                              C.c_void_p(ws) if ws else None, ws_bytes,
                                              C.c_void_p(acc) if acc else None, C.c_void_p(st) if st else None,
                                              C.c_void_p(tl) if tl else None, nt, s0, sc, None, None)

    E = _lib.PTMI_EINVAL
    # the list
    assert call(nt=-1) == E and 'n_tiles -1 outside [0, 2]' in err()
    assert call(nt=3) == E and 'n_tiles 3 outside [0, 2]' in err()  # the grid has 2 tiles
    assert call(nt=1 << 30) == E and 'n_tiles' in err()
    assert call(tl=None, nt=1) == E and 'tile_list NULL/misaligned' in err()
    assert call(tl=None, nt=2) == E and 'tile_list NULL/misaligned' in err()
    assert call(tl=66) == E and 'tile_list NULL/misaligned' in err()
    # ptmi_wf_render_stats's own prologue, in its order: scene, frame, accum, stats, before the list
    assert call(scene=None, nt=-1) == E and 'scene is NULL' in err()
    assert call(frame=None, nt=-1) == E and 'frame is NULL' in err()
    assert call(frame=make_frame(max_depth=300), nt=-1) == E and 'max_depth' in err()
    assert call(frame=make_frame(window=(0, 0, 17, 8)), nt=-1) == E and 'bad window' in err()
    assert call(frame=make_frame(band=(2, 2, 2))) == E and 'band' in err()
    assert call(acc=None, nt=-1) == E and 'accum is NULL' in err()
    assert call(st=None, nt=-1) == E and 'stats NULL/misaligned' in err()
    assert call(st=36) == E and 'stats NULL/misaligned' in err()
    # and what follows the list
    assert call(sc=-1) == E and 'bad sample range' in err()
    assert call(s0=-1) == E and 'bad sample range' in err()
    assert call(ws=None) == E and 'workspace' in err()
    assert call(ws=264) == E and 'workspace' in err()
    assert call(ws_bytes=64) == E and 'workspace' in err()
    # a banded frame's grid: 16 x 8 in one-row bands of 2 ranks is 4 rows of 64 x 1 tiles
    banded = make_frame(band=(1, 2, 1))
    assert call(frame=banded, nt=4, sc=0) == _lib.PTMI_OK
    assert call(frame=banded, nt=5) == E and 'n_tiles 5 outside [0, 4]' in err()
    # no-ops: an empty list (with or without a pointer), no samples
    assert call(nt=0, tl=None) == _lib.PTMI_OK
    assert call(nt=0) == _lib.PTMI_OK
    assert call(sc=0) == _lib.PTMI_OK
