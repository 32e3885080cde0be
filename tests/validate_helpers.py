"""numpy f32 reference of the history-validation ABI (include/ptmi_validate.h),
and the inputs the CPU and GPU tests share.

``validate`` restates steps 1 - 6 in numpy f32, one rounding per operation in
the header's order. ``synthetic`` makes a frame of plausible history and fresh
pixels with one pixel per property the contract names. ``quality_case`` is the
case that shows the feature: the sliding sphere of motion_helpers, its history
rendered by the CPU oracle and carried by the numpy ``reproject_moved``, judged
by four fresh oracle samples against a 512-sample truth."""
import numpy as np

import adaptive_helpers as ah
import motion_helpers as mh
import reproject_helpers as rh

f32 = np.float32
DEFAULTS = dict(radius=3, k_lo=2.0, k_hi=4.0)
# (width, height); 5 x 3 is smaller than any window but r = 0; 80 x 50 is 5 x 4 tiles of 16 x 16 with a ragged bottom
# row, the one frame with tiles (row 1, columns 1 - 3) whose halo of the largest radius lies wholly inside the image
FRAMES = [(48, 27), (37, 21), (16, 16), (17, 1), (5, 3), (80, 50)]
RADII = [0, 3, 7]


def same_bits(a, b):
    """Equal bit for bit, except that a NaN equals a NaN of any payload."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _finite3(s):
    return np.isfinite(s[..., 0]) & np.isfinite(s[..., 1]) & np.isfinite(s[..., 2])


def entries(hist_stats, fresh_stats):
    """Step 1: (d, v, usable) per pixel."""
    hs, fs = np.asarray(hist_stats, f32), np.asarray(fresh_stats, f32)
    one = f32(1)
    with np.errstate(all='ignore'):
        usable = (hs[..., 0] >= 2) & (fs[..., 0] >= 2) & _finite3(hs) & _finite3(fs)
        d = fs[..., 1] - hs[..., 1]
        v = (hs[..., 2] / (hs[..., 0] - one)) / hs[..., 0] + (fs[..., 2] / (fs[..., 0] - one)) / fs[..., 0]
    zero = np.zeros(usable.shape, f32)
    return np.where(usable, d, zero).astype(f32), np.where(usable, v, zero).astype(f32), usable


def window_sums(d, v, usable, radius):
    """Step 2: (D, V, m), j outer and i inner, both ascending; pixels outside the image add 0.0f."""
    H, W = d.shape
    r = int(radius)
    pad = lambda a: np.pad(a, r)  # noqa: E731
    dp, vp, up = pad(d), pad(v), pad(usable.astype(np.int64))
    D, V, m = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), np.int64)
    with np.errstate(all='ignore'):
        for j in range(2 * r + 1):
            for i in range(2 * r + 1):
                D = D + dp[j:j + H, i:i + W]
                V = V + vp[j:j + H, i:i + W]
                m = m + up[j:j + H, i:i + W]
    assert D.dtype == f32 and V.dtype == f32
    return D, V, m


def stale_fraction(D, V, m, k_lo, k_hi):
    """Step 3: (lam, branch); branch names the case each pixel took."""
    k_lo, k_hi = f32(k_lo), f32(k_hi)
    with np.errstate(all='ignore'):
        z = np.abs(D) / np.sqrt(V)
        lin = np.fmin(np.fmax((z - k_lo) / (k_hi - k_lo), f32(0)), f32(1)).astype(f32)
    nan_sum = np.isnan(D) | np.isnan(V)
    conds = [m == 0, nan_sum, (V > 0) & np.isnan(z), V > 0, (V == 0) & (D == 0), V == 0]
    names = ['empty', 'nan_sum', 'nan_z', 'ratio', 'flat_equal', 'flat_unequal', 'negative']
    lam = np.select(conds, [f32(0), f32(1), f32(1), lin, f32(0), f32(1)], default=f32(1)).astype(f32)
    branch = np.select(conds, list(range(6)), default=6)
    return lam, np.array(names)[branch]


def validate(hist_accum, hist_stats, fresh_accum, fresh_stats, radius=3, k_lo=2.0, k_hi=4.0, details=False):
    """(accum_out, stats_out, weight[, details]) of ptmi_history_validate. details: lam, branch, n_v, n_h
    (step 4's), usable, m."""
    ha, hs = np.array(hist_accum, f32), np.array(hist_stats, f32)
    fa, fs = np.asarray(fresh_accum, f32), np.asarray(fresh_stats, f32)
    d, v, usable = entries(hs, fs)
    D, V, m = window_sums(d, v, usable, radius)
    lam, branch = stale_fraction(D, V, m, k_lo, k_hi)
    one, zero = f32(1), f32(0)
    # 4.
    bad = ~(np.isfinite(ha).all(-1) & _finite3(hs))
    ha[bad] = 0
    hs[bad] = 0
    n_h, mean_h, m2_h = hs[..., 0], hs[..., 1], hs[..., 2]
    n_f, mean_f, m2_f = fs[..., 0], fs[..., 1], fs[..., 2]
    with np.errstate(all='ignore'):
        n_v = np.floor(n_h * (one - lam)).astype(f32)
        weight = np.where(n_h >= 1, n_v / n_h, zero).astype(f32)  # 6.
        # 5.
        scale = (1.0 / np.maximum(n_h, one).astype(np.float64)).astype(f32)
        av = ((ha * scale[..., None]) * n_v[..., None]).astype(f32)
        m2_v = np.where(n_h >= 2, (m2_h / (n_h - one)) * (n_v - one), zero).astype(f32)
        same = n_v == n_h
        av = np.where(same[..., None], ha, av)
        m2_v = np.where(same, m2_h, m2_v)
        delta = mean_f - mean_h
        n = n_v + n_f
        merged_accum = av + fa
        merged_stats = np.stack([n, mean_h + delta * (n_f / n), (m2_v + m2_f) + (delta * delta) * ((n_v * n_f) / n),
                                 np.zeros_like(n)], -1)
    assert merged_accum.dtype == f32 and merged_stats.dtype == f32 and av.dtype == f32 and m2_v.dtype == f32
    alone_stats = np.stack([n_v, mean_h, m2_v, np.zeros_like(n_v)], -1)
    fresh_only, no_fresh = ~(n_v >= 1), n_f == 0
    out_accum = np.where(fresh_only[..., None], fa, np.where(no_fresh[..., None], av, merged_accum))
    out_stats = np.where(fresh_only[..., None], fs, np.where(no_fresh[..., None], alone_stats, merged_stats))
    res = (out_accum.astype(f32), out_stats.astype(f32), weight)
    if details:
        res += (dict(lam=lam, branch=branch, n_v=n_v, n_h=n_h.copy(), usable=usable, m=m),)
    return res


def kept_fraction(n_v, n_h):
    """sum(n_v) / sum(n_h) of step 4's counts, 1.0 for an empty history: MI355XRenderer.render_validated's value."""
    total = float(np.asarray(n_h, np.float64).sum())
    return float(np.asarray(n_v, np.float64).sum()) / total if total > 0 else 1.0


# ---------------------------------------------------------------- synthetic inputs
PLANTED = ('n_h0', 'n_h1', 'n_h2', 'n_h32', 'n_f0', 'n_f1', 'n_f4', 'flat_equal', 'flat_unequal', 'nan_hist',
           'inf_hist', 'nan_fresh')


def planted_pixels(width, height):
    """name -> flat pixel index of the PLANTED pixels: spread over the frame, all different."""
    step = max(1, (width * height) // len(PLANTED))
    return {name: k * step for k, name in enumerate(PLANTED)}


def synthetic(width, height, seed=0):
    """(hist_accum, hist_stats, fresh_accum, fresh_stats) of a width x height
    frame: a history of 32 samples with M2 = s2 * 31 and four fresh samples
    whose mean is the history's plus the noise four samples have; in the right
    half of the frame the fresh mean is 0.5 higher (the light changed), in a
    band of two columns beside it 0.12 higher. On top, one pixel per name of
    PLANTED (``planted_pixels``): histories of 0, 1, 2 and 32 samples; fresh
    pixels of 0, 1 and 4 samples; M2 = 0 on both sides with equal and with
    unequal means; a history pixel with a NaN accum value (its stats stay
    finite) and one with an infinite M2; a NaN fresh pixel."""
    rng = np.random.default_rng(7000 + 100 * width + height + seed)
    H, W = height, width
    colour = rng.uniform(0.2, 0.8, (H, W, 3)).astype(f32)
    s2 = rng.uniform(0.01, 0.03, (H, W)).astype(f32)
    hs = np.zeros((H, W, 4), f32)
    hs[..., 0], hs[..., 1], hs[..., 2] = 32, ah.luminance(colour), s2 * f32(31)
    ha = (colour * f32(32)).astype(f32)
    shift = (rng.standard_normal((H, W)) * np.sqrt(s2 / 4)).astype(f32)
    xs = np.arange(W)[None, :]
    shift = shift + np.where(xs >= W // 2, f32(0.5), np.where(xs >= W // 2 - 2, f32(0.12), f32(0))).astype(f32)
    cf = (colour + shift[..., None]).astype(f32)
    fs = np.zeros((H, W, 4), f32)
    fs[..., 0], fs[..., 1], fs[..., 2] = 4, ah.luminance(cf), rng.uniform(0.01, 0.03, (H, W)).astype(f32) * f32(3)
    fa = (cf * f32(4)).astype(f32)
    ha, hs, fa, fs = (a.reshape(H * W, -1) for a in (ha, hs, fa, fs))
    at = planted_pixels(W, H)
    ha[at['n_h0']], hs[at['n_h0']] = 0, 0
    p = at['n_h1']
    ha[p], hs[p] = colour.reshape(-1, 3)[p], (1, hs[p, 1], 0, 0)
    p = at['n_h2']
    ha[p], hs[p] = colour.reshape(-1, 3)[p] * f32(2), (2, hs[p, 1], s2.reshape(-1)[p], 0)
    fa[at['n_f0']], fs[at['n_f0']] = 0, 0
    p = at['n_f1']
    fa[p], fs[p] = cf.reshape(-1, 3)[p], (1, fs[p, 1], 0, 0)
    p = at['flat_equal']
    hs[p, 2] = fs[p, 2] = 0
    fs[p, 1] = hs[p, 1]
    p = at['flat_unequal']
    hs[p, 2] = fs[p, 2] = 0
    fs[p, 1] = hs[p, 1] + f32(0.25)
    ha[at['nan_hist'], 1] = np.nan
    hs[at['inf_hist'], 2] = np.inf
    fa[at['nan_fresh']], fs[at['nan_fresh'], 1:3] = np.nan, np.nan
    return ha.reshape(H, W, 3), hs.reshape(H, W, 4), fa.reshape(H, W, 3), fs.reshape(H, W, 4)


def pack_input(radius, k_lo, k_hi, hist_accum, hist_stats, fresh_accum, fresh_stats):
    """The raw f32 input file of csrc/validate_check.cpp."""
    return np.concatenate([np.array([radius, k_lo, k_hi], f32)] +
                          [np.asarray(a, f32).reshape(-1) for a in (hist_accum, hist_stats, fresh_accum,
                                                                    fresh_stats)]).astype(f32)


# ---------------------------------------------------------------- the quality case
BACKGROUND = (0.7, 0.8, 1.0)
HISTORY_SAMPLES, MAX_HISTORY, FRESH_BEGIN, FRESH_SPP = 64, 32.0, 64, 4
TRUTH_BEGIN, TRUTH_SPP = 1000, 512
CHANGED_LIGHT = 0.03  # the change of the truth's luminance above which a pixel's light counts as changed
_oracle = {}


def oracle_frame(sa, cam, variant='mk', seed=0, max_depth=50):
    """(oracle scene, oracle frame) of scene arrays and a camera-upload dict, cached per scene object."""
    import oracle
    if id(sa) not in _oracle:
        _oracle[id(sa)] = (sa, oracle.OracleScene(sa))
    return _oracle[id(sa)][1], oracle.make_frame(cam, BACKGROUND, max_depth, seed, cam['width'], cam['height'])


def oracle_cols(sa, cam, s_begin, s_count, variant='mk'):
    """(s_count, H, W, 3) f32: the colours of samples [s_begin, s_begin + s_count) of every pixel, one oracle
    render of one sample into a zeroed accumulator each."""
    import oracle
    osc, fr = oracle_frame(sa, cam, variant)
    W, H = cam['width'], cam['height']
    out = np.zeros((s_count, H, W, 3), f32)
    for s in range(s_count):
        oracle.render(osc, fr, variant, out[s], (0, 0, W, H), s_begin + s, 1)
    return out


def oracle_mean(sa, cam, s_begin, s_count, variant='mk'):
    """(H, W, 3) f32: the mean colour of samples [s_begin, s_begin + s_count)."""
    import oracle
    osc, fr = oracle_frame(sa, cam, variant)
    W, H = cam['width'], cam['height']
    acc = np.zeros((H, W, 3), f32)
    oracle.render(osc, fr, variant, acc, (0, 0, W, H), s_begin, s_count)
    return acc / f32(s_count)


def stats_render(cols):
    """(accum, stats) of sample colours accumulated from cleared buffers in Welford order."""
    acc, st = np.zeros(cols.shape[1:], f32), np.zeros(cols.shape[1:3] + (4,), f32)
    ah.accumulate(acc, st, cols)
    return acc, st


def image(accum, stats):
    """The linear image: every pixel divided by its own count (0 where it has none)."""
    n = stats[..., 0:1]
    with np.errstate(all='ignore'):
        return np.where(n > 0, accum / n, f32(0)).astype(f32)


def mse(img, truth, mask):
    return float(((img.astype(np.float64) - truth.astype(np.float64))[mask] ** 2).mean())


def carried(case, hist, moved):
    """The history ``hist`` = (accum, stats) of the slide case's scene before the move carried by the numpy
    reproject_moved to the scene after it (``moved``) or to the same scene (the control), capped at MAX_HISTORY."""
    prm = dict(rh.DEFAULTS, max_history=MAX_HISTORY)
    cam = case['cur']
    if moved:
        return mh.reproject_moved(cam, cam, case['guides_cur'], case['guides_prev'], hist[0], hist[1],
                                  case['ids_cur'], case['ids_prev'], case['rows_cur'], case['rows_prev'], **prm)
    return mh.reproject_moved(cam, cam, case['guides_prev'], case['guides_prev'], hist[0], hist[1], case['ids_prev'],
                              case['ids_prev'], case['rows_prev'], case['rows_prev'], **prm)


def orderings(hist, fresh, plain, validated, kept, truth, changed):
    """The figures the quality assertions read, for one carried history
    ``hist``, the fresh pair, history + fresh as today's continuation adds them
    (``plain``: the fresh samples accumulated on top of the history, sample by
    sample) and the ``validated`` pair with its ``kept`` fraction: the MSE of
    linear rgb against ``truth`` of the fresh samples alone, of plain and of
    validated, over all pixels with history, over those of ``changed`` and
    over the rest."""
    has = hist[1][..., 0] > 0
    imgs = {'fresh': image(*fresh), 'plain': image(*plain), 'validated': image(*validated)}
    out = {'pixels': {'all': int(has.sum()), 'changed': int((has & changed).sum()),
                      'unchanged': int((has & ~changed).sum())}, 'kept': float(kept)}
    for name, mask in (('all', has), ('changed', has & changed), ('unchanged', has & ~changed)):
        out[name] = {k: mse(img, truth, mask) if mask.any() else float('nan') for k, img in imgs.items()}
    return out


def reference_orderings(entry, **params):
    """``orderings`` of one half of ``quality_case`` (hist, fresh colours, truth, changed), all in numpy."""
    hist, cols, truth, changed = entry
    fresh = stats_render(cols)
    plain = (hist[0].copy(), hist[1].copy())
    ah.accumulate(plain[0], plain[1], cols)
    va, vs, _, det = validate(*hist, *fresh, details=True, **dict(DEFAULTS, **params))
    return orderings(hist, fresh, plain, (va, vs), kept_fraction(det['n_v'], det['n_h']), truth, changed)


_quality = {}


def quality_case():
    """The slide case through the oracle (megakernel semantics, seed 0, depth
    50, background BACKGROUND): a dict with 'moved' and 'control', each
    (hist, fresh colours, truth, changed), the history being oracle samples
    0 - 63 of the scene before the move carried by ``carried``, the fresh
    colours samples 64 - 67 ((4, H, W, 3)) and the truth the mean of samples
    1000 - 1511 of the scene they are judged in; ``changed``
    marks the pixels whose truth luminance differs between the two scenes by
    more than CHANGED_LIGHT (nowhere, for the control)."""
    if not _quality:
        case = mh.slide_case()
        cam = case['cur']
        before, after = case['sa_prev'], case['sa_cur']
        rendered = stats_render(oracle_cols(before, cam, 0, HISTORY_SAMPLES))
        truth = {k: oracle_mean(sa, cam, TRUTH_BEGIN, TRUTH_SPP) for k, sa in (('before', before), ('after', after))}
        changed = np.abs(ah.luminance(truth['after']) - ah.luminance(truth['before'])) > f32(CHANGED_LIGHT)
        _quality['moved'] = (carried(case, rendered, True), oracle_cols(after, cam, FRESH_BEGIN, FRESH_SPP),
                             truth['after'], changed)
        _quality['control'] = (carried(case, rendered, False), oracle_cols(before, cam, FRESH_BEGIN, FRESH_SPP),
                               truth['before'], np.zeros_like(changed))
        _quality['case'] = case
    return _quality


def check_orderings(moved, control):
    """The assertions of the quality case on ``orderings`` of its two halves; prints the figures first."""
    for name, o in (('moved', moved), ('control', control)):
        print(f'{name}: pixels {o["pixels"]} kept {o["kept"]:.4f}')
        for k in ('all', 'changed', 'unchanged'):
            print(f'  {k:9s} ' + ' '.join(f'{m}={v:.5f}' for m, v in o[k].items()))
    # the premises: enough changed-light pixels with history, and today's merge worse there than no history at all
    assert moved['pixels']['changed'] >= 50
    assert moved['changed']['plain'] > moved['changed']['fresh']
    # where the light changed, the validated image beats both alternatives; over the frame it beats today's
    assert moved['changed']['validated'] < moved['changed']['plain']
    assert moved['changed']['validated'] < moved['changed']['fresh']
    assert moved['all']['validated'] < moved['all']['plain']
    # nothing moved: nearly all history kept, and no worse than today's merge where the light did not change
    assert control['kept'] >= 0.95
    assert control['all']['validated'] <= moved['unchanged']['plain']
