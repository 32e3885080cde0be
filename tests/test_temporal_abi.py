"""CPU tests of the temporal ABI (include/ptmi_temporal.h): its symbol is in the
library and in ptmi.temporal's own table and in none of the other three ABIs',
and every rejected argument returns PTMI_EINVAL before a HIP call with its
message. No device is needed: the pointers are never dereferenced."""
import ctypes as C
import os
import re

import pytest

from ptmi import _lib, guide, post, temporal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_temporal_header_symbols_are_exported_and_bound():
    txt = header('ptmi_temporal.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_reproject'} == set(temporal.EXPORTS) == set(temporal.SIGNATURES)
    lib = temporal.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert int(re.search(r'#define PTMI_TEMPORAL_VERSION (\d+)', txt).group(1)) == temporal.TEMPORAL_VERSION == 1
    # the other three ABIs do not know it, and stay at their versions
    for other in (_lib.EXPORTS, post.EXPORTS, guide.EXPORTS):
        assert not syms & set(other)
    for other in ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h'):
        assert 'ptmi_reproject' not in header(other) and 'ptmi_temporal' not in header(other)
    assert post.POST_VERSION == 1 and guide.GUIDE_VERSION == 1
    assert C.sizeof(temporal.ReprojectParams) == 20
    assert [f[0] for f in temporal.ReprojectParams._fields_] == ['max_history', 'sigma_z', 'normal_min', 'sigma_a',
                                                                 'flags']
    # the contract's assumption about the previous camera is stated
    assert 'perpendicular' in txt


def test_default_parameters():
    p = temporal.params()
    assert (p.max_history, p.flags) == (32.0, 0)
    assert abs(p.sigma_z - 0.1) < 1e-7 and abs(p.normal_min - 0.9) < 1e-7 and abs(p.sigma_a - 0.2) < 1e-7


W, H = 16, 8
N = W * H
# addresses far apart: guides 32 N = 4096 B, stats 16 N = 2048 B, accum 12 N = 1536 B
GC, GP, AP, SP, AO, SO = 1 << 16, 2 << 16, 3 << 16, 4 << 16, 5 << 16, 6 << 16


def call(lib, cur=True, prev=True, gc=GC, gp=GP, ap=AP, sp=SP, width=W, height=H, ao=AO, so=SO, null_params=False,
         flags=0, **prm):
    p = temporal.params(**prm)
    p.flags = flags
    cams = _lib.Camera(), _lib.Camera()
    return lib.ptmi_reproject(C.byref(cams[0]) if cur else None, C.byref(cams[1]) if prev else None, C.c_void_p(gc),
                              C.c_void_p(gp), C.c_void_p(ap), C.c_void_p(sp), width, height,
                              None if null_params else C.byref(p), C.c_void_p(ao), C.c_void_p(so), None)


nan = float('nan')


@pytest.mark.parametrize('kw,msg', [
    # a NULL pointer
    (dict(cur=False), 'a camera is NULL'),
    (dict(prev=False), 'a camera is NULL'),
    (dict(gc=None), 'guides_cur NULL/misaligned'),
    (dict(gp=None), 'guides_prev NULL/misaligned'),
    (dict(ap=None), 'accum_prev is NULL'),
    (dict(sp=None), 'stats_prev NULL/misaligned'),
    (dict(null_params=True), 'params is NULL'),
    (dict(ao=None), 'accum_out is NULL'),
    (dict(so=None), 'stats_out NULL/misaligned'),
    # the size
    (dict(width=0), 'bad image size'),
    (dict(height=0), 'bad image size'),
    (dict(width=-16), 'bad image size'),
    (dict(height=-3), 'bad image size'),
    (dict(width=65536, height=32768), 'bad image size'),  # 2^31 pixels
    # guides or stats pointers not 16-byte aligned
    (dict(gc=GC + 4), 'guides_cur NULL/misaligned'),
    (dict(gp=GP + 8), 'guides_prev NULL/misaligned'),
    (dict(sp=SP + 12), 'stats_prev NULL/misaligned'),
    (dict(so=SO + 8), 'stats_out NULL/misaligned'),
    # an output overlapping any input
    (dict(ao=GC), 'accum_out aliases guides_cur'),
    (dict(ao=GC + 32 * N - 4), 'accum_out aliases guides_cur'),
    (dict(ao=GP - 12 * N + 4), 'accum_out aliases guides_prev'),
    (dict(ao=AP), 'accum_out aliases accum_prev'),
    (dict(ao=AP + 12 * N - 4), 'accum_out aliases accum_prev'),
    (dict(ao=SP + 16), 'accum_out aliases stats_prev'),
    (dict(so=GC + 16), 'stats_out aliases guides_cur'),
    (dict(so=GP + 32 * N - 16), 'stats_out aliases guides_prev'),
    (dict(so=AP - 16 * N + 16), 'stats_out aliases accum_prev'),
    (dict(so=SP), 'stats_out aliases stats_prev'),
    (dict(so=SP + 16 * N - 16), 'stats_out aliases stats_prev'),
    # or the other output
    (dict(so=AO), 'accum_out aliases stats_out'),
    (dict(ao=SO + 16 * N - 4), 'accum_out aliases stats_out'),
    # the parameters
    (dict(max_history=nan), 'max_history'),
    (dict(max_history=0.5), 'max_history'),
    (dict(max_history=-1.0), 'max_history'),
    (dict(max_history=float((1 << 24) + 2)), 'max_history'),
    (dict(max_history=float('inf')), 'max_history'),
    (dict(sigma_z=-1e-3), 'sigma_z'),
    (dict(sigma_z=nan), 'sigma_z'),
    (dict(sigma_a=-1.0), 'sigma_a'),
    (dict(sigma_a=nan), 'sigma_a'),
    (dict(normal_min=nan), 'normal_min'),
    (dict(normal_min=-1.5), 'normal_min'),
    (dict(normal_min=1.0000001), 'normal_min'),
    (dict(flags=1), 'flags must be 0'),
    (dict(flags=-1), 'flags must be 0'),
    (dict(flags=1 << 30), 'flags must be 0'),
])
def test_reproject_rejects_bad_arguments_before_touching_device(kw, msg):
    lib = temporal.load()
    assert call(lib, **kw) == _lib.PTMI_EINVAL
    err = lib.ptmi_last_error().decode()
    assert msg in err and err.startswith('reproject: ')


def test_adjacent_buffers_do_not_count_as_overlapping():
    """The overlap test is exact to the byte: buffers that touch are told apart
    from buffers that share one. Checked through the first parameter test that
    follows the overlap tests, so that no launch happens."""
    lib = temporal.load()
    for kw in (dict(ao=GC + 32 * N), dict(ao=AP - 12 * N), dict(so=SP + 16 * N), dict(so=AO + 12 * N)):
        assert call(lib, flags=1, **kw) == _lib.PTMI_EINVAL
        assert 'flags must be 0' in lib.ptmi_last_error().decode(), kw
