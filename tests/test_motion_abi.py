"""CPU tests of the motion ABI (include/ptmi_motion.h): its symbols are in the
library and in ptmi.motion's own table and in none of the other ABIs'; every
rejected argument returns PTMI_EINVAL before a HIP call with its message (no
device is needed: the pointers are never dereferenced); the shared arithmetic
(csrc/pt_motion_math.hpp, run on the CPU by csrc/motion_check.cpp) equals the
numpy reference (motion_helpers) bit for bit, also built with
-fsanitize=address,undefined; and what the reference itself must do to be
worth matching: with unmoved rows it is reproject_helpers.reproject, and a
sphere that slides across a fixed view takes its history along."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_helpers as mh
import reproject_helpers as rh
from ptmi import _lib, guide, motion, post, temporal, update, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


# ---------------------------------------------------------------- the ABI table
def test_motion_header_symbols_are_exported_and_bound():
    txt = header('ptmi_motion.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == {'ptmi_guide_trace_ids', 'ptmi_reproject_moved'} == set(motion.EXPORTS) == set(motion.SIGNATURES)
    lib = motion.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert int(re.search(r'#define PTMI_MOTION_VERSION (\d+)', txt).group(1)) == motion.MOTION_VERSION == 1
    assert int(re.search(r'#define PTMI_RPM_MATCH_IDS (\d+)', txt).group(1)) == motion.RPM_MATCH_IDS == 1
    # a table of its own: the other six know neither symbol, and their headers do not name this one
    for other in (_lib, post, guide, temporal, wf_tiles, update):
        assert not syms & set(other.EXPORTS), other.__name__
    for other in ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h'):
        assert 'ptmi_motion' not in header(other) and not any(s in header(other) for s in syms)
    assert temporal.TEMPORAL_VERSION == 1 and guide.GUIDE_VERSION == 1 and update.UPDATE_VERSION == 1
    assert _lib.ABI_VERSION == 9
    assert C.sizeof(motion.ReprojectMovedParams) == 24
    assert [f[0] for f in motion.ReprojectMovedParams._fields_] == ['base', 'flags']
    # the two consequences the contract must state
    assert 'normal turned' in txt and 'is not detected' in txt and 'max_history bounds' in txt


def test_default_parameters():
    p = motion.params()
    assert (p.base.max_history, p.base.flags, p.flags) == (32.0, 0, motion.RPM_MATCH_IDS)
    assert motion.params(match_ids=False).flags == 0


# ---------------------------------------------------------------- rejected arguments: the reprojection
W, H = 16, 8
N = W * H
NS, NQ, NT = 4, 2, 2  # 64, 128 and 96 bytes of rows
(GC, GP, AP, SP, IC, IP, AO, SO, RS, RQ, RT, PS, PQ, PT) = (k << 16 for k in range(1, 15))
nan = float('nan')


def call(lib, cur=True, prev=True, gc=GC, gp=GP, ap=AP, sp=SP, ic=IC, ip=IP, scene=True, counts=(NS, NQ, NT),
         rows=(RS, RQ, RT), prows=(PS, PQ, PT), width=W, height=H, ao=AO, so=SO, null_params=False, flags=0,
         base_flags=0, **prm):
    p = motion.params(**prm)
    p.flags, p.base.flags = flags, base_flags
    cams = _lib.Camera(), _lib.Camera()
    v = _lib.SceneView()
    v.spheres, v.quads, v.tris = rows
    v.num_spheres, v.num_quads, v.num_triangles = counts
    P = C.c_void_p
    return lib.ptmi_reproject_moved(C.byref(cams[0]) if cur else None, C.byref(cams[1]) if prev else None, P(gc),
                                    P(gp), P(ap), P(sp), P(ic), P(ip), C.byref(v) if scene else None, P(prows[0]),
                                    P(prows[1]), P(prows[2]), width, height, None if null_params else C.byref(p),
                                    P(ao), P(so), None)


@pytest.mark.parametrize('kw,msg', [
    # everything ptmi_reproject rejects
    (dict(cur=False), 'a camera is NULL'),
    (dict(prev=False), 'a camera is NULL'),
    (dict(gc=None), 'guides_cur NULL/misaligned'),
    (dict(gp=GP + 8), 'guides_prev NULL/misaligned'),
    (dict(ap=None), 'accum_prev is NULL'),
    (dict(sp=SP + 12), 'stats_prev NULL/misaligned'),
    (dict(null_params=True), 'params is NULL'),
    (dict(ao=None), 'accum_out is NULL'),
    (dict(so=SO + 8), 'stats_out NULL/misaligned'),
    (dict(width=0), 'bad image size'),
    (dict(height=-3), 'bad image size'),
    (dict(width=65536, height=32768), 'bad image size'),
    (dict(ao=GC + 32 * N - 4), 'accum_out aliases guides_cur'),
    (dict(ao=GP - 12 * N + 4), 'accum_out aliases guides_prev'),
    (dict(ao=AP), 'accum_out aliases accum_prev'),
    (dict(so=SP + 16 * N - 16), 'stats_out aliases stats_prev'),
    (dict(so=AO), 'accum_out aliases stats_out'),
    (dict(max_history=nan), 'max_history'),
    (dict(max_history=0.5), 'max_history'),
    (dict(max_history=float((1 << 24) + 2)), 'max_history'),
    (dict(sigma_z=-1e-3), 'sigma_z'),
    (dict(sigma_a=nan), 'sigma_a'),
    (dict(normal_min=1.0000001), 'normal_min'),
    (dict(base_flags=1), 'base.flags must be 0'),
    # NULL or misaligned id images
    (dict(ic=None), 'ids_cur NULL/misaligned'),
    (dict(ic=IC + 2), 'ids_cur NULL/misaligned'),
    (dict(ip=None), 'ids_prev NULL/misaligned'),
    (dict(ip=IP + 1), 'ids_prev NULL/misaligned'),
    # the scene and its rows
    (dict(scene=False), 'scene is NULL'),
    (dict(counts=(-1, NQ, NT)), 'count of spheres'),
    (dict(counts=(NS, NQ, (1 << 25) + 1)), 'count of tris'),
    (dict(rows=(None, RQ, RT)), "the scene's spheres NULL/misaligned"),
    (dict(rows=(RS, RQ + 4, RT)), "the scene's quads NULL/misaligned"),
    # a previous-row pointer that is NULL while its count is > 0
    (dict(prows=(None, PQ, PT)), 'prev_spheres NULL/misaligned'),
    (dict(prows=(PS, None, PT)), 'prev_quads NULL/misaligned'),
    (dict(prows=(PS, PQ, None)), 'prev_tris NULL/misaligned'),
    (dict(prows=(PS, PQ, PT + 8)), 'prev_tris NULL/misaligned'),
    # an output overlapping the id images or the row arrays
    (dict(ao=IC + 4 * N - 4), 'accum_out aliases ids_cur'),
    (dict(so=IP), 'stats_out aliases ids_prev'),
    (dict(ao=RS + 16 * NS - 4), 'accum_out aliases spheres'),
    (dict(so=RQ + 64 * NQ - 16), 'stats_out aliases quads'),
    (dict(ao=RT - 12 * N + 4), 'accum_out aliases tris'),
    (dict(so=PS), 'stats_out aliases prev_spheres'),
    (dict(ao=PQ + 64), 'accum_out aliases prev_quads'),
    (dict(so=PT + 48 * NT - 16), 'stats_out aliases prev_tris'),
    # unknown flag bits
    (dict(flags=2), 'unknown flag bits'),
    (dict(flags=-1), 'unknown flag bits'),
    (dict(flags=1 << 30 | 1), 'unknown flag bits'),
])
def test_reproject_moved_rejects_bad_arguments_before_touching_device(kw, msg):
    lib = motion.load()
    assert call(lib, **kw) == _lib.PTMI_EINVAL
    err = lib.ptmi_last_error().decode()
    assert msg in err and err.startswith('reproject_moved: ')


def test_adjacent_buffers_and_empty_types_are_accepted_by_the_checks():
    """Buffers that touch do not overlap, and a type with count 0 may have NULL
    rows. Checked through the flag test, the last one, so that no launch happens."""
    lib = motion.load()
    for kw in (dict(ao=IC + 4 * N), dict(so=RS + 16 * NS), dict(ao=PT - 12 * N), dict(so=PQ + 64 * NQ),
               dict(counts=(NS, 0, NT), rows=(RS, None, RT), prows=(PS, None, PT)),
               dict(counts=(0, 0, 0), rows=(None, None, None), prows=(None, None, None)),
               dict(counts=(NS, 0, NT), so=RQ)):  # nothing of the empty type is read: no overlap to find
        assert call(lib, flags=2, **kw) == _lib.PTMI_EINVAL
        assert 'unknown flag bits' in lib.ptmi_last_error().decode(), kw


# ---------------------------------------------------------------- rejected arguments: the id trace
def _scene_and_frame():
    """An empty scene's view (no device memory is touched before the checks) and a whole 16 x 8 frame."""
    v = _lib.SceneView()
    v.perlin_vec, v.perlin_perm = 1 << 20, 2 << 20
    f = _lib.Frame()
    f.width, f.height, f.x0, f.y0, f.w, f.h = 16, 8, 0, 0, 16, 8
    f.band_rows, f.band_stride, f.band_offset = 1, 1, 0
    f.max_depth = 50
    f.traversal = _lib.TRAVERSALS['stack']
    return v, f


@pytest.mark.parametrize('edit,msg', [
    # ptmi_guide_trace's
    (lambda v, f: dict(guides=None), 'guides NULL/misaligned'),
    (lambda v, f: dict(guides=(1 << 14) + 8), 'guides NULL/misaligned'),
    (lambda v, f: setattr(f, 'w', 8), 'windowed'),
    (lambda v, f: (setattr(f, 'band_stride', 2), setattr(f, 'band_offset', 1)), 'banded'),
    (lambda v, f: setattr(f, 'traversal', 7), 'unknown traversal'),
    (lambda v, f: setattr(v, 'num_spheres', -1), 'negative scene counts'),
    (lambda v, f: dict(scene=None), 'scene is NULL'),
    (lambda v, f: dict(frame=None), 'frame is NULL'),
    # the id image
    (lambda v, f: dict(ids=None), 'ids NULL/misaligned'),
    (lambda v, f: dict(ids=(1 << 15) + 2), 'ids NULL/misaligned'),
    (lambda v, f: dict(ids=(1 << 14) + 32 * N - 4), 'ids aliases guides'),
    (lambda v, f: dict(ids=(1 << 14) - 4 * N + 4), 'ids aliases guides'),
    (lambda v, f: dict(ids=(1 << 20) + 4092), "ids aliases the scene's perlin_vec"),
    (lambda v, f: dict(ids=(2 << 20) - 4 * N + 4), "ids aliases the scene's perlin_perm"),
])
def test_guide_trace_ids_rejects_bad_arguments_before_touching_device(edit, msg):
    lib = motion.load()
    v, f = _scene_and_frame()
    kw = edit(v, f)
    kw = kw if isinstance(kw, dict) else {}
    scene = None if 'scene' in kw else C.byref(v)
    frame = None if 'frame' in kw else C.byref(f)
    rc = lib.ptmi_guide_trace_ids(scene, frame, C.c_void_p(kw.get('guides', 1 << 14)),
                                  C.c_void_p(kw.get('ids', 1 << 15)), None)
    assert rc == _lib.PTMI_EINVAL
    assert msg in lib.ptmi_last_error().decode()


# ---------------------------------------------------------------- the shared arithmetic on the CPU
@pytest.fixture(scope='module')
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('mv') / 'motion_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'motion_check', f'MOTION_CHECK={exe}'], check=True)
    return exe


@pytest.fixture(scope='module')
def san_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('mv_san') / 'motion_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'motion_check', f'MOTION_CHECK={exe}',
                    'MOTION_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    return exe


def run_check(exe, tmp_path, case, match_ids, prm):
    h, w = case['stats'].shape[:2]
    paths = [str(tmp_path / n) for n in ('in.f32', 'ids.i32', 'accum.f32', 'stats.f32')]
    mh.pack_input(case['cur'], case['prev'], prm, case['guides_cur'], case['guides_prev'], case['accum'],
                  case['stats'], case['rows_cur'], case['rows_prev']).tofile(paths[0])
    mh.pack_ids(case['ids_cur'], case['ids_prev']).tofile(paths[1])
    counts = [str(len(case['rows_cur'][t])) for t in (mh.SPHERE, mh.QUAD, mh.TRIANGLE)]
    r = subprocess.run([exe, str(w), str(h)] + counts + [str(int(match_ids))] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(paths[2], f32).reshape(h, w, 3), np.fromfile(paths[3], f32).reshape(h, w, 4)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def both(check_exe, san_exe, tmp_path, case, match_ids, prm=rh.DEFAULTS):
    """The case through the check program and through its sanitizer build; both
    bit for bit the numpy reference, whose outputs and details are returned."""
    ref_a, ref_s, det = mh.reference(case, match_ids=match_ids, details=True, **prm)
    for exe in (check_exe, san_exe):
        a, s = run_check(exe, tmp_path, case, match_ids, prm)
        assert same(s, ref_s)
        assert same(a, ref_a)
        rh.check_properties(a, s, det, prm['max_history'])
    return ref_a, ref_s, det


@pytest.mark.parametrize('match_ids', [True, False])
@pytest.mark.parametrize('kind', mh.SYNTHETIC_KINDS)
def test_check_program_equals_numpy_reference(check_exe, san_exe, tmp_path, kind, match_ids):
    case = mh.synthetic_case(kind)
    _, ref_s, _ = both(check_exe, san_exe, tmp_path, case, match_ids)
    has = ref_s[..., 0] > 0
    hit = case['guides_cur'][..., 7] != 0
    named = hit & (case['ids_cur'] >= 0)
    assert not has[hit & ~named].any()  # a hit pixel without an id has no history
    if kind == 'nan_row':  # P_prev is NaN: step 4 is false
        assert not has[hit].any()
    else:
        assert has[named].mean() > 0.8
    moved = any(not same(case['rows_cur'][t], case['rows_prev'][t]) for t in case['rows_cur'])
    assert moved
    if kind != 'nan_row':  # the move shows: not what unmoved rows give
        still = mh.reference(dict(case, rows_prev=case['rows_cur']), match_ids=match_ids)
        assert not same(still[0], mh.reference(case, match_ids=match_ids)[0])


@pytest.mark.parametrize('moved', [True, False])
def test_check_program_equals_numpy_reference_on_oracle_guides(check_exe, san_exe, tmp_path, moved):
    """`coverage` traced by the CPU oracle, the camera orbited one degree, with
    and without the update of a sphere, a quad and a triangle: the GPU tests' case."""
    case = mh.coverage_case(moved)
    for match_ids in (True, False):
        _, ref_s, _ = both(check_exe, san_exe, tmp_path, case, match_ids)
        assert (ref_s[..., 0] > 0).mean() > 0.9
    if moved:  # each moved primitive is in view, and keeps history on most of its pixels
        has = mh.reference(case)[1][..., 0] > 0
        ok, ptype, prim = mh.decode(case['ids_cur'], {t: len(r) for t, r in case['rows_cur'].items()})
        for t in (mh.SPHERE, mh.QUAD, mh.TRIANGLE):
            changed = (case['rows_cur'][t].view(np.uint32) != case['rows_prev'][t].view(np.uint32)).any(-1)
            assert changed.sum() == 1
            px = ok & (ptype == t)
            px[px] = changed[prim[px]]
            assert px.sum() >= 15 and has[px].mean() > 0.8, (t, int(px.sum()), float(has[px].mean()))


def test_other_parameters_and_hostile_ids(check_exe, san_exe, tmp_path):
    """The id decode on the CPU, under the sanitizers: a prim equal to the
    count, type nibble 7, INT32_MIN and -1 on hit pixels, and in the previous
    id image; and the other corner of the parameter ranges."""
    case = dict(mh.synthetic_case('tris'))
    ids_cur, ids_prev = case['ids_cur'].copy(), case['ids_prev'].copy()
    hostile = [mh.make_id(mh.TRIANGLE, 6), np.int32(7 << 28 | 1), np.int32(-2 ** 31), np.int32(-1),
               mh.make_id(mh.SPHERE, 0), mh.make_id(mh.QUAD, 0), np.int32(3 << 28), np.int32(0x0fffffff)]
    for k, v in enumerate(hostile):
        ids_cur[3 + 2 * k, 5:9] = v
        ids_prev[4 + 2 * k, 20:24] = v
    case.update(ids_cur=ids_cur, ids_prev=ids_prev)
    for prm in (rh.DEFAULTS, dict(max_history=1.0, sigma_z=0.0, normal_min=1.0, sigma_a=0.0),
                dict(max_history=float(1 << 24), sigma_z=10.0, normal_min=-1.0, sigma_a=10.0)):
        for match_ids in (True, False):
            ref_a, ref_s, _ = both(check_exe, san_exe, tmp_path, case, match_ids, prm)
            for k in range(len(hostile)):
                assert not ref_a[3 + 2 * k, 5:9].any() and not ref_s[3 + 2 * k, 5:9].any()


# ---------------------------------------------------------------- what the reference must do
@pytest.mark.parametrize('name', ['coverage', 'synthetic'])
def test_reference_with_unmoved_rows_is_the_static_reprojection(name):
    """Previous rows bitwise the current rows, flags 0, the camera moved: the
    reference equals reproject_helpers.reproject on the same inputs, bit for bit."""
    case = mh.coverage_case(False) if name == 'coverage' else mh.synthetic_case('quads')
    case = dict(case, rows_prev=case['rows_cur'])
    if name == 'synthetic':  # every hit pixel named: a hit pixel without an id has no history in either form
        hit = case['guides_cur'][..., 7] != 0
        case['ids_cur'] = np.where(hit & (case['ids_cur'] < 0), mh.make_id(mh.QUAD, 0), case['ids_cur'])
    assert not all(np.array_equal(case['cur'][k], case['prev'][k]) for k in ('center', 'pixel00'))
    a, s = mh.reference(case, match_ids=False)
    pa, ps = rh.reproject(case['cur'], case['prev'], case['guides_cur'], case['guides_prev'], case['accum'],
                          case['stats'], **rh.DEFAULTS)
    assert same(a, pa) and same(s, ps)
    assert (s[..., 0] > 0).mean() > 0.8


def test_a_sliding_sphere_takes_its_history_along():
    """The property that shows the feature, on the reference. A fixed camera; an
    opaque sphere moves parallel to the image plane by 2.0, more than its
    diameter 1.6; the history is colour A on the sphere's old pixels, B
    elsewhere, n = 8. The move was chosen so that, on the reference alone, the
    interior set (all four taps on the old sphere) holds 75 of the sphere's 113
    current pixels: not empty, and more than half."""
    case = mh.slide_case()
    sid = case['sphere_id']
    old, new = case['ids_prev'] == sid, case['ids_cur'] == sid
    assert old.sum() > 100 and not (old & new).any()  # moved by more than its projected diameter
    a, s, det = mh.reference(case, details=True)
    pa, ps = rh.reproject(case['cur'], case['prev'], case['guides_cur'], case['guides_prev'], case['accum'],
                          case['stats'], **rh.DEFAULTS)
    sphere, interior = mh.check_slide(case, a, s, pa, ps, det)
    assert (sphere, interior) == (mh.SLIDE_SPHERE_PIXELS, mh.SLIDE_INTERIOR_PIXELS) == (113, 75)
    assert 2 * interior >= sphere
    # an implementation that forwards to ptmi_reproject fails check_slide
    with pytest.raises(AssertionError):
        mh.check_slide(case, pa, ps, pa, ps, det)


def test_trace_ids_names_the_device_rows():
    """trace_ids gives device indices: the row an id names is the primitive the
    oracle hit, for every type `coverage` has."""
    case = mh.coverage_case(False)
    sa, ids = case['sa_prev'], case['ids_prev']
    ok, ptype, prim = mh.decode(ids, {t: len(r) for t, r in case['rows_prev'].items()})
    assert np.array_equal(ok, ids >= 0) and {int(t) for t in np.unique(ptype[ok])} == {0, 1, 2}
    g = case['guides_prev']
    sph = ok & (ptype == mh.SPHERE)
    row = case['rows_prev'][mh.SPHERE][prim[sph]]
    # a sphere pixel's surface point lies on the sphere its id names
    P = mh.surface_points(case['prev'], g)[sph]
    r = np.linalg.norm(P.astype(np.float64) - row[:, 0:3], axis=1)
    assert np.abs(r - row[:, 3]).max() < 1e-2 * row[:, 3].max()
    assert sa.num_spheres == len(case['rows_prev'][mh.SPHERE])
