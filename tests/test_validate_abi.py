"""CPU tests of the history-validation ABI (include/ptmi_validate.h): its symbol
is in the library and in ptmi.validate's own table and in none of the other
eight; every rejected argument returns PTMI_EINVAL with its message before a HIP
call (no device is needed: the pointers are never dereferenced); the arithmetic
the kernel calls, run on the CPU by csrc/validate_check.cpp, equals the numpy
reference (validate_helpers) bit for bit, also under the sanitizers; an empty
history gives the fresh pair back and an empty fresh pair the history; and on
the sliding-sphere scene, through the CPU oracle, the validated image beats both
today's merge and the fresh samples alone where the light changed, and costs
nothing where nothing moved."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import validate_helpers as vh
from ptmi import _lib, guide, motion, post, temporal, tree, update, validate, wf_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
OTHER_HEADERS = ('ptmi.h', 'ptmi_post.h', 'ptmi_guide.h', 'ptmi_temporal.h', 'ptmi_wf_tiles.h', 'ptmi_update.h',
                 'ptmi_motion.h', 'ptmi_tree.h')
NAMES = {'ptmi_history_validate'}


def header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def err():
    return _lib.load().ptmi_last_error().decode()


def test_header_symbol_is_exported_and_bound_apart_from_the_other_abis():
    txt = header('ptmi_validate.h')
    syms = set(re.findall(r'\b(ptmi_[a-z_0-9]+)\s*\(', txt)) - {'ptmi_last_error'}
    assert syms == NAMES == set(validate.EXPORTS) == set(validate.SIGNATURES)
    lib = validate.load()
    assert all(hasattr(lib, s) for s in NAMES)
    assert int(re.search(r'#define PTMI_VALIDATE_VERSION (\d+)', txt).group(1)) == validate.VALIDATE_VERSION == 1
    assert int(re.search(r'#define PTMI_VALIDATE_MAX_RADIUS (\d+)', txt).group(1)) == validate.MAX_RADIUS == 7
    others = (_lib.SIGNATURES, post.SIGNATURES, guide.SIGNATURES, temporal.SIGNATURES, wf_tiles.SIGNATURES,
              update.SIGNATURES, motion.SIGNATURES, tree.SIGNATURES)
    assert len(others) == 8 and not any(NAMES & set(o) for o in others)
    for other in OTHER_HEADERS:
        assert not any(word in header(other) for word in ('ptmi_validate', 'PTMI_VALIDATE', 'history_validate'))
    assert int(re.search(r'#define PTMI_ABI_VERSION (\d+)', header('ptmi.h')).group(1)) == _lib.ABI_VERSION == 9
    assert len(validate.SIGNATURES['ptmi_history_validate'][1]) == 11
    assert C.sizeof(validate.ValidateParams) == 12
    p = validate.params()
    assert (p.radius, p.k_lo, p.k_hi) == (3, 2.0, 4.0) == tuple(vh.DEFAULTS[k] for k in ('radius', 'k_lo', 'k_hi'))
    with pytest.raises(ValueError, match='whole number'):
        validate.params(radius=2.5)


def test_history_validate_rejects_bad_arguments_before_touching_device():
    lib = validate.load()
    E = _lib.PTMI_EINVAL
    W, H = 48, 27
    n = W * H
    # fake device pointers, far enough apart for a 48 x 27 frame: 16 * n bytes is the largest image
    base = {'ha': 1 << 20, 'hs': 2 << 20, 'fa': 3 << 20, 'fs': 4 << 20, 'oa': 5 << 20, 'os': 6 << 20, 'w': 7 << 20}

    def call(width=W, height=H, prm=(3, 2.0, 4.0), null_params=False, **ptr):
        a = dict(base, **ptr)
        p = validate.ValidateParams(*prm)
        return lib.ptmi_history_validate(a['ha'], a['hs'], a['fa'], a['fs'], width, height,
                                         None if null_params else C.byref(p), a['oa'], a['os'], a['w'], None)

    for key, name, align in (('ha', 'hist_accum', 4), ('hs', 'hist_stats', 16), ('fa', 'fresh_accum', 4),
                             ('fs', 'fresh_stats', 16), ('oa', 'out_accum', 4), ('os', 'out_stats', 16)):
        assert call(**{key: None}) == E and f'history_validate: {name} NULL/misaligned' in err()
        assert call(**{key: base[key] + align // 2}) == E and f'history_validate: {name} NULL/misaligned' in err()
    assert call(w=base['w'] + 2) == E and 'history_validate: weight_out misaligned' in err()
    assert call(null_params=True) == E and 'history_validate: params is NULL' in err()
    for size in ((0, H), (W, 0), (-1, H), (W, -5), (1 << 16, 1 << 15)):
        assert call(*size) == E and 'history_validate: bad image size' in err()
    for radius in (-1, 8, 100):
        assert call(prm=(radius, 2.0, 4.0)) == E and 'history_validate: radius must be in [0, 7]' in err()
    for k in ((np.nan, 4.0), (2.0, np.nan), (2.0, np.inf), (-np.inf, 4.0)):
        assert call(prm=(3,) + k) == E and 'history_validate: k_lo and k_hi must be finite' in err()
    assert call(prm=(3, -0.5, 4.0)) == E and 'history_validate: k_lo must be >= 0' in err()
    for k in ((2.0, 2.0), (4.0, 2.0)):
        assert call(prm=(3,) + k) == E and 'history_validate: k_hi must be above k_lo' in err()
    # not in place: every output against every input, and against the other outputs
    sizes = {'ha': 12 * n, 'hs': 16 * n, 'fa': 12 * n, 'fs': 16 * n}
    names = {'ha': 'hist_accum', 'hs': 'hist_stats', 'fa': 'fresh_accum', 'fs': 'fresh_stats'}
    for out, out_name in (('oa', 'out_accum'), ('os', 'out_stats'), ('w', 'weight_out')):
        for key in sizes:
            assert call(**{out: base[key]}) == E and f'history_validate: {out_name} aliases {names[key]}' in err()
            assert call(**{out: base[key] + sizes[key] - 16}) == E and f'{out_name} aliases {names[key]}' in err()
    assert call(**{'os': base['oa'] + 16}) == E and 'out_stats aliases out_accum' in err()
    assert call(w=base['os'] + 16 * n - 4) == E and 'weight_out aliases out_stats' in err()
    assert call(w=base['oa']) == E and 'weight_out aliases out_accum' in err()


# ------------------------------------------------------------------ the check program against numpy
def check_cases():
    """(width, height, radius, k_lo, k_hi, the four input images) of every frame of FRAMES at every radius of
    RADII with the default k, and the 48 x 27 frame with another pair of k."""
    out = [(w, h, r, 2.0, 4.0) + vh.synthetic(w, h) for w, h in vh.FRAMES for r in vh.RADII]
    out.append((48, 27, 2, 0.0, 0.75) + vh.synthetic(48, 27, seed=1))
    return out


def test_synthetic_inputs_reach_what_they_are_for():
    seen_branches, seen_lam = set(), set()
    for w, h, r, k_lo, k_hi, *images in check_cases():
        ha, hs, fa, fs = (a.reshape(h * w, -1) for a in images)
        at = vh.planted_pixels(w, h)
        assert len(set(at.values())) == len(vh.PLANTED) <= w * h
        assert [hs[at[k], 0] for k in ('n_h0', 'n_h1', 'n_h2', 'n_h32')] == [0, 1, 2, 32]
        assert [fs[at[k], 0] for k in ('n_f0', 'n_f1', 'n_f4')] == [0, 1, 4]
        for k in ('flat_equal', 'flat_unequal'):
            assert hs[at[k], 2] == 0 and fs[at[k], 2] == 0
        assert hs[at['flat_equal'], 1] == fs[at['flat_equal'], 1] and hs[at['flat_unequal'], 1] != fs[at['flat_unequal'], 1]
        assert np.isnan(ha[at['nan_hist']]).any() and np.isfinite(hs[at['nan_hist']]).all()
        assert np.isinf(hs[at['inf_hist'], 2]) and np.isnan(fa[at['nan_fresh']]).all()
        oa, os_, wt, det = vh.validate(*images, radius=r, k_lo=k_lo, k_hi=k_hi, details=True)
        lam, branch = det['lam'].reshape(-1), det['branch'].reshape(-1)
        assert ((lam >= 0) & (lam <= 1)).all()
        if r == 0:  # the window is the pixel itself: each planted pixel takes its own branch
            assert branch[at['flat_equal']] == 'flat_equal' and lam[at['flat_equal']] == 0
            assert branch[at['flat_unequal']] == 'flat_unequal' and lam[at['flat_unequal']] == 1
            for k in ('n_h0', 'n_h1', 'n_f0', 'n_f1', 'inf_hist', 'nan_fresh'):
                assert branch[at[k]] == 'empty' and lam[at[k]] == 0, k
            assert branch[at['nan_hist']] == 'ratio'  # judged by its finite stats, emptied by its accum
        seen_branches |= set(branch.tolist())
        seen_lam |= {'zero'} if (lam == 0).any() else set()
        seen_lam |= {'one'} if (lam == 1).any() else set()
        seen_lam |= {'between'} if ((lam > 0) & (lam < 1)).any() else set()
        if (w, h, k_lo) == (48, 27, 2.0):  # at the default k every radius meets all three
            assert (lam == 0).any() and (lam == 1).any() and ((lam > 0) & (lam < 1)).any(), r
        # a bad pixel stays in its own output pixel: everything else is finite
        own = np.zeros(w * h, bool)
        own[[at['nan_hist'], at['inf_hist'], at['nan_fresh']]] = True
        assert np.isfinite(oa.reshape(w * h, -1)[~own]).all() and np.isfinite(os_.reshape(w * h, -1)[~own]).all()
        assert np.isfinite(wt).all() and ((wt >= 0) & (wt <= 1)).all()
        n_out = os_[..., 0].reshape(-1)
        assert np.array_equal(n_out[~own], np.floor(n_out[~own]))  # counts stay whole numbers
        # the emptied history pixels are their fresh pixels, the NaN fresh pixel passes through
        for k in ('nan_hist', 'inf_hist', 'n_h0'):
            assert oa.reshape(-1, 3)[at[k]].tobytes() == fa[at[k]].tobytes()
            assert os_.reshape(-1, 4)[at[k]].tobytes() == fs[at[k]].tobytes() and wt.reshape(-1)[at[k]] == 0
        assert np.isnan(oa.reshape(-1, 3)[at['nan_fresh']]).all()
    assert {'empty', 'ratio', 'flat_equal', 'flat_unequal'} <= seen_branches
    assert seen_lam == {'zero', 'one', 'between'}


def test_reference_branches_of_step_3_that_no_plausible_image_takes():
    D = np.array([np.nan, 1, np.inf, 1, 0, 1, 1, 3], f32)
    V = np.array([1, np.nan, np.inf, -1, 0, 0, np.inf, 1], f32)
    m = np.array([1, 1, 1, 1, 1, 1, 1, 0])
    lam, branch = vh.stale_fraction(D, V, m, 2.0, 4.0)
    assert branch.tolist() == ['nan_sum', 'nan_sum', 'nan_z', 'negative', 'flat_equal', 'flat_unequal', 'ratio', 'empty']
    assert lam.tolist() == [1, 1, 1, 1, 0, 1, 0, 0]
    lam, _ = vh.stale_fraction(np.array([4, 6, 8, 10], f32), np.full(4, 4, f32), np.ones(4), 2.0, 4.0)
    assert lam.tolist() == [0, 0.5, 1, 1]  # z = 2, 3, 4, 5


def run_check(exe, tmp_path, case, tag):
    w, h, r, k_lo, k_hi, *images = case
    src, *dst = (str(tmp_path / f'{tag}.{k}') for k in ('in', 'accum', 'stats', 'weight'))
    vh.pack_input(r, k_lo, k_hi, *images).tofile(src)
    subprocess.run([exe, str(w), str(h), src] + dst, check=True, timeout=60)
    return tuple(np.fromfile(p, f32).reshape(shape) for p, shape in zip(dst, ((h, w, 3), (h, w, 4), (h, w))))


def _run_check(exe, tmp_path):
    for k, case in enumerate(check_cases()):
        w, h, r, k_lo, k_hi, *images = case
        got = run_check(exe, tmp_path, case, f'c{k}')
        want = vh.validate(*images, radius=r, k_lo=k_lo, k_hi=k_hi)
        for g, x, what in zip(got, want, ('accum', 'stats', 'weight')):
            assert vh.same_bits(g, x), (w, h, r, what)
    # hostile statistics: negative and huge M2, negative and fractional counts, infinities everywhere
    rng = np.random.default_rng(11)
    w, h = 19, 7
    pool = np.array([0, -0.0, 1, 2, 3.5, -4, 32, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan, 1e-40], f32)
    images = [rng.choice(pool, (h, w, c)).astype(f32) for c in (3, 4, 3, 4)]
    got = run_check(exe, tmp_path, (w, h, 1, 2.0, 4.0, *images), 'hostile')
    want = vh.validate(*images, radius=1)
    assert all(vh.same_bits(g, x) for g, x in zip(got, want))
    # a short input file, a radius of 8, k_hi == k_lo
    src, dst = str(tmp_path / 'bad.in'), [str(tmp_path / f'bad.{k}') for k in 'asw']
    np.zeros(3 + 14 * 6 - 1, f32).tofile(src)
    assert subprocess.run([exe, '3', '2', src] + dst, capture_output=True).returncode == 2
    for head in ((8, 2, 4), (3, 2, 2), (1.5, 2, 4), (3, -1, 4)):
        np.concatenate([np.array(head, f32), np.zeros(14 * 6, f32)]).tofile(src)
        assert subprocess.run([exe, '3', '2', src] + dst, capture_output=True).returncode == 2, head
    assert subprocess.run([exe, '0', '2', src] + dst, capture_output=True).returncode == 2


def test_check_program_equals_numpy(tmp_path):
    exe = str(tmp_path / 'validate_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'validate_check', f'VALIDATE_CHECK={exe}'], check=True)
    _run_check(exe, tmp_path)


def test_check_program_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same inputs."""
    exe = str(tmp_path / 'validate_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'validate_check', f'VALIDATE_CHECK={exe}',
                    'VALIDATE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    _run_check(exe, tmp_path)


# ------------------------------------------------------------------ identities
@pytest.mark.parametrize('radius', vh.RADII)
def test_an_empty_history_gives_the_fresh_pair_and_an_empty_fresh_pair_the_history(radius):
    ha, hs, fa, fs = vh.synthetic(37, 21)
    oa, os_, wt = vh.validate(np.zeros_like(ha), np.zeros_like(hs), fa, fs, radius=radius)
    assert oa.tobytes() == fa.tobytes() and os_.tobytes() == fs.tobytes() and not wt.any()
    # a history as the reprojection leaves it: accum = colour * n, M2 = s2 * (n - 1), whole counts of every size
    rng = np.random.default_rng(5)
    n = rng.integers(0, 40, (21, 37)).astype(f32)
    colour, s2 = rng.uniform(0, 2, (21, 37, 3)).astype(f32), rng.uniform(0, 0.1, (21, 37)).astype(f32)
    hs = np.stack([n, np.where(n > 0, vh.ah.luminance(colour), 0), np.where(n > 0, s2 * (n - f32(1)), 0),
                   np.zeros_like(n)], -1).astype(f32)
    ha = (colour * n[..., None]).astype(f32)
    oa, os_, wt = vh.validate(ha, hs, np.zeros_like(ha), np.zeros_like(hs), radius=radius)
    assert oa.tobytes() == ha.tobytes() and os_.tobytes() == hs.tobytes()
    assert np.array_equal(wt, (n >= 1).astype(f32))


# ------------------------------------------------------------------ the quality case
def test_validation_beats_todays_merge_where_the_light_changed_and_costs_nothing_where_it_did_not():
    """The sliding sphere through the CPU oracle: 64 samples before the move
    carried by the numpy reproject_moved and capped at 32, four fresh samples
    after it, against a 512-sample truth. Orderings and one cap, no recorded
    numbers (validate_helpers.check_orderings)."""
    q = vh.quality_case()
    vh.check_orderings(vh.reference_orderings(q['moved']), vh.reference_orderings(q['control']))
