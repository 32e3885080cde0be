"""CPU tests of the adaptive-sampling entry points (ABI v8): the tile grid of
a frame and the argument validation, which happens before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from ptmi import _lib, device


def make_frame(**kw):
    cam = {k: np.zeros(3, np.float32) for k in ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = 0.0
    args = dict(cam=cam, bg=(0, 0, 0), max_depth=50, seed=0, width=16, height=8)
    args.update(kw)
    return device.make_frame(**args)


def grid(f):
    v = [C.c_int32() for _ in range(4)]
    rc = _lib.load().ptmi_mk_tile_grid(C.byref(f), *[C.byref(x) for x in v])
    assert rc == _lib.PTMI_OK
    return tuple(x.value for x in v)


def empty_scene():
    v = _lib.SceneView()
    v.perlin_vec = v.perlin_perm = 16
    return v


def err():
    return _lib.load().ptmi_last_error().decode()


def test_tile_grid_shapes():
    assert grid(make_frame())[:2] == (8, 8)
    assert grid(make_frame(width=400, height=225)) == (8, 8, 50, 29)
    assert grid(make_frame(width=800, height=800, band=(4, 2, 1)))[:2] == (16, 4)
    assert grid(make_frame(width=800, height=800, band=(1, 8, 3)))[:2] == (64, 1)
    assert grid(make_frame(width=800, height=800, band=(2, 4, 0)))[:2] == (32, 2)
    assert grid(make_frame(width=800, height=800, band=(8, 2, 0)))[:2] == (8, 8)


def test_tile_grid_of_a_window():
    # 200 x 136 window: 25 x 17 tiles of 8 x 8
    assert grid(make_frame(width=800, height=800, window=(96, 200, 200, 136))) == (8, 8, 25, 17)
    # 4-row bands of 2 ranks: 68 local rows in 16 x 4 tiles, 13 x 17 (200 = 12.5 x 16)
    assert grid(make_frame(width=800, height=800, window=(96, 200, 200, 136), band=(4, 2, 1))) == (16, 4, 13, 17)
    # one-row bands of 8 ranks: rows 3, 11, .. of 136: 17 rows of 64 x 1 tiles
    assert grid(make_frame(width=800, height=800, window=(96, 200, 200, 136), band=(1, 8, 3))) == (64, 1, 4, 17)


def test_tile_grid_rejects_bad_arguments():
    lib = _lib.load()
    f = make_frame()
    v = [C.c_int32() for _ in range(4)]
    assert lib.ptmi_mk_tile_grid(None, *[C.byref(x) for x in v]) == _lib.PTMI_EINVAL
    assert lib.ptmi_mk_tile_grid(C.byref(f), None, C.byref(v[1]), C.byref(v[2]), C.byref(v[3])) == _lib.PTMI_EINVAL
    assert lib.ptmi_mk_tile_grid(C.byref(make_frame(band=(0, 1, 0))), *[C.byref(x) for x in v]) == _lib.PTMI_EINVAL


def test_stats_clear_rejects_bad_arguments():
    lib = _lib.load()
    f = make_frame()
    assert lib.ptmi_stats_clear(C.byref(f), None, None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert lib.ptmi_stats_clear(C.byref(f), C.c_void_p(24), None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert lib.ptmi_stats_clear(C.byref(make_frame(window=(0, 0, 17, 8))), C.c_void_p(16), None) == _lib.PTMI_EINVAL
    assert 'bad window' in err()


def test_trace_tiles_rejects_bad_arguments():
    lib = _lib.load()
    f, v = make_frame(), empty_scene()  # 16 x 8: 2 tiles, 128 pixels
    big = 1 << 20

    def call(ws=256, ws_bytes=big, tl=64, nt=1, s0=0, sc=2, scene=v, frame=f):
        return lib.ptmi_mk_trace_tiles_ws(C.byref(scene) if scene is not None else None, C.byref(frame),
                                          C.c_void_p(ws) if ws else None, ws_bytes, C.c_void_p(tl) if tl else None,
                                          nt, s0, sc, None, None)

    assert call(scene=None) == _lib.PTMI_EINVAL and 'scene' in err()
    assert call(frame=make_frame(max_depth=300)) == _lib.PTMI_EINVAL and 'max_depth' in err()
    assert call(sc=0) == _lib.PTMI_EINVAL and 'sample range' in err()
    assert call(s0=-1) == _lib.PTMI_EINVAL and 'sample range' in err()
    assert call(nt=-1) == _lib.PTMI_EINVAL and 'n_tiles' in err()
    assert call(nt=3) == _lib.PTMI_EINVAL and 'n_tiles' in err()  # the grid has 2 tiles
    assert call(tl=None) == _lib.PTMI_EINVAL and 'tile_list' in err()
    assert call(tl=66) == _lib.PTMI_EINVAL and 'tile_list' in err()
    assert call(ws=None) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(ws=264) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(ws_bytes=lib.ptmi_mk_workspace_bytes(C.byref(f), 2) - 1) == _lib.PTMI_EINVAL and 'workspace' in err()
    # an empty list is a no-op, with or without a list pointer, and one sample is accepted
    assert call(nt=0, tl=None) == _lib.PTMI_OK
    assert call(nt=0, sc=1) == _lib.PTMI_OK


def test_resolve_stats_rejects_bad_arguments():
    lib = _lib.load()
    f = make_frame()
    big = 1 << 20

    def call(ws=256, ws_bytes=big, acc=16, st=32, tl=None, nt=0, sc=2, frame=f):
        return lib.ptmi_mk_resolve_stats_ws(C.byref(frame), C.c_void_p(ws) if ws else None, ws_bytes,
                                            C.c_void_p(acc) if acc else None, C.c_void_p(st) if st else None,
                                            C.c_void_p(tl) if tl else None, nt, sc, None)

    assert call(frame=make_frame(band=(2, 2, 2))) == _lib.PTMI_EINVAL and 'band' in err()
    assert call(acc=None) == _lib.PTMI_EINVAL and 'accum' in err()
    assert call(st=None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(st=40) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(sc=0) == _lib.PTMI_EINVAL and 'sample_count' in err()
    assert call(tl=66, nt=1) == _lib.PTMI_EINVAL and 'tile_list' in err()
    assert call(tl=64, nt=-1) == _lib.PTMI_EINVAL and 'n_tiles' in err()
    assert call(tl=64, nt=3) == _lib.PTMI_EINVAL and 'n_tiles' in err()
    assert call(ws=None) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(ws_bytes=64) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(tl=64, nt=0) == _lib.PTMI_OK  # an empty list resolves nothing


def test_wf_render_stats_rejects_bad_arguments():
    lib = _lib.load()
    f, v = make_frame(), empty_scene()

    def call(ws=256, ws_bytes=1 << 40, acc=16, st=32, s0=0, sc=1, scene=v):
        return lib.ptmi_wf_render_stats(C.byref(scene) if scene is not None else None, C.byref(f),
                                        C.c_void_p(ws) if ws else None, ws_bytes, C.c_void_p(acc) if acc else None,
                                        C.c_void_p(st) if st else None, s0, sc, None, None)

    assert call(scene=None) == _lib.PTMI_EINVAL and 'scene' in err()
    assert call(acc=None) == _lib.PTMI_EINVAL and 'accum' in err()
    assert call(st=None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(st=36) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(sc=-1) == _lib.PTMI_EINVAL and 'sample range' in err()
    assert call(ws=None) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(ws_bytes=64) == _lib.PTMI_EINVAL and 'workspace' in err()
    assert call(sc=0) == _lib.PTMI_OK


def test_tile_update_rejects_bad_arguments():
    lib = _lib.load()
    f = make_frame()

    def call(st=32, thr=0.05, lo=4, hi=16, state=64, terr=128, tl=192, na=256, frame=f):
        p = [C.c_void_p(x) if x else None for x in (state, terr, tl, na)]
        return lib.ptmi_tile_update(C.byref(frame), C.c_void_p(st) if st else None, thr, lo, hi, *p, None)

    assert call(frame=make_frame(window=(4, 4, 4, 5))) == _lib.PTMI_EINVAL and 'bad window' in err()
    assert call(st=None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(st=24) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(thr=-0.5) == _lib.PTMI_EINVAL and 'threshold' in err()
    assert call(thr=float('nan')) == _lib.PTMI_EINVAL and 'threshold' in err()
    assert call(lo=-1) == _lib.PTMI_EINVAL and 'spp' in err()
    assert call(lo=8, hi=4) == _lib.PTMI_EINVAL and 'spp' in err()
    for k in ('state', 'terr', 'tl', 'na'):
        assert call(**{k: None}) == _lib.PTMI_EINVAL and 'tile buffers' in err()
        assert call(**{k: 66}) == _lib.PTMI_EINVAL and 'tile buffers' in err()


def test_tonemap_stats_rejects_bad_arguments():
    lib = _lib.load()

    def call(acc=16, st=32, out=48, w=4, h=4):
        return lib.ptmi_tonemap_stats(C.c_void_p(acc) if acc else None, C.c_void_p(st) if st else None,
                                      C.c_void_p(out) if out else None, w, h, None)

    assert call(acc=None) == _lib.PTMI_EINVAL
    assert call(out=None) == _lib.PTMI_EINVAL
    assert call(w=0) == _lib.PTMI_EINVAL
    assert call(h=-1) == _lib.PTMI_EINVAL
    assert call(st=None) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(st=8) == _lib.PTMI_EINVAL and 'stats' in err()
    assert call(w=40000, h=40000) == _lib.PTMI_ECAPACITY
