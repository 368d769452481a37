"""Float64 numpy reference of the ensemble mix and its step tails (npfn_mix_rows, include/npfn.h).

It restates the operations, not the kernels: per estimator a softmax of the fp16 logits times the
float32 inverse temperature, the cancelled bars of a translated estimator removed, the translation
of oracle.preprocess_oracle.translate_probs in float64, the arithmetic mean or softmax(mean of
logs), and then the bar distribution's inverse CDF, log density and CDF on the float32 borders
fma(bz, ystats[1], ystats[0]) (:func:`borders32`).  A translation table is the triple (idx [nb + 1], share
[nb + 1] with the flags folded in as -1 / 2, tcancel [nb]) the engine exports.

An estimator row with no finite logit has no mass to give (it adds nothing to the mean; under geo
the whole row loses its mass).  A row with no mass is all zeros here; its draw, density and CDF
are NaN.

The ``_flags_as_share`` and ``_cum_restart`` arguments of :func:`translate64` seed two defects for
tests/test_mix_host.py (which shows that the bars of tests/test_gpu_mix.py would see them); no
other caller sets them.
"""
import math

import numpy as np

from bar_cdf_ref import HM, bucket64, cdf_from_probs
from oracle.preprocess_oracle import cancel_broken_borders, translation_table, yeo_johnson_inverse


def inv_temperature(T) -> np.float32:
    return np.float32(1) / np.float32(T)


def softmax_rows64(x: np.ndarray) -> np.ndarray:
    """Row softmax in float64; a row with no finite value gives zeros."""
    m = x.max(-1, keepdims=True)
    live = np.isfinite(m)
    with np.errstate(invalid="ignore"):
        e = np.where(live, np.exp(x - np.where(live, m, 0.0)), 0.0)
    s = e.sum(-1, keepdims=True)
    return np.divide(e, s, out=np.zeros_like(e), where=s > 0)


def translate64(q: np.ndarray, idx, share, _flags_as_share=False, _cum_restart=None) -> np.ndarray:
    """q [R, nb] over the source bars -> [R, nb] over the common bars (translate_probs in float64):
    the CDF at every common border = exclusive prefix sum + share of the source bucket, 0 / 1
    where the flag says so and at the first / last border, differences clamped at 0."""
    nb = q.shape[1]
    cum = np.cumsum(q, axis=1) - q
    if _cum_restart is not None and _cum_restart < nb:
        cum[:, _cum_restart:] -= cum[:, _cum_restart:_cum_restart + 1]
    sh = np.asarray(share, dtype=np.float64)
    left = cum[:, idx] + q[:, idx] * sh[None, :]
    if not _flags_as_share:
        left = np.where(sh[None, :] < 0, 0.0, np.where(sh[None, :] > 1.5, 1.0, left))
    left = np.clip(left, 0.0, 1.0)
    left[:, 0] = 0.0
    left[:, nb] = 1.0
    return np.maximum(left[:, 1:] - left[:, :-1], 0.0)


def estimator_probs(logits16, invT, ett=None, table=None, **defect) -> np.ndarray:
    """[E, R, nb] float64: every estimator's bar probabilities over the common borders."""
    lg = np.asarray(logits16, dtype=np.float16).astype(np.float64) * np.float64(np.float32(invT))
    E = lg.shape[0]
    out = np.empty(lg.shape, dtype=np.float64)
    for e in range(E):
        if ett is not None and ett[e]:
            idx, share, tcancel = table
            x = np.where(np.asarray(tcancel, dtype=bool)[None, :], -np.inf, lg[e])
            q = softmax_rows64(x)
            empty = q.sum(-1) == 0
            out[e] = translate64(q, idx, share, **defect)
            out[e][empty] = 0.0
        else:
            out[e] = softmax_rows64(lg[e])
    return out


def geo_from_probs(q, logits16, invT, ett=None) -> np.ndarray:
    """softmax(mean_e log q_e) of q [E, R, nb] = :func:`estimator_probs`.  An untranslated
    estimator's log q_e is its log-softmax taken in the log domain, x - max - log sum exp(x - max):
    a bar 7e4 below the maximum (the +-65504 row) has a finite log probability there, while the
    exp of it underflows even in float64 and its log would be -inf."""
    lg = np.asarray(logits16, dtype=np.float16).astype(np.float64) * np.float64(np.float32(invT))
    with np.errstate(divide="ignore", invalid="ignore"):
        logq = np.log(q)
        for e in range(q.shape[0]):
            if ett is None or not ett[e]:
                m = lg[e].max(-1, keepdims=True)
                live = np.isfinite(m)
                s = np.where(live, np.exp(lg[e] - np.where(live, m, 0.0)), 0.0).sum(-1, keepdims=True)
                logq[e] = np.where(live, lg[e] - np.where(live, m, 0.0) - np.log(np.where(live, s, 1.0)), -np.inf)
        return softmax_rows64(logq.mean(0))


def mix_probs(logits16, invT, ett=None, table=None, geo=False, **defect) -> np.ndarray:
    """[R, nb] float64 mixture of logits16 [E, R, nb] (fp16)."""
    q = estimator_probs(logits16, invT, ett, table, **defect)
    if not geo:
        return q.mean(0)
    return geo_from_probs(q, logits16, invT, ett)


def borders32(bz, ystats) -> np.ndarray:
    """The common borders as the device forms them, float32: fma(bz, s, m) -- the compiler contracts
    every ``bz * s + m`` of the kernels (k_borders, the tails, and k_target_tf's __fadd_rn(__fmul_rn())
    too, which the HIP headers define as the plain operators) into one v_fma_f32, so the product is
    not rounded: here the exact float64 product plus m, rounded once to float64 and then to float32.
    oracle borders_of rounds the product first and may differ by one ulp."""
    bz = np.asarray(bz, dtype=np.float32).astype(np.float64)
    return (bz * np.float64(np.float32(ystats[1])) + np.float64(np.float32(ystats[0]))).astype(np.float32)


def sample_bucket(b64: np.ndarray, th: np.ndarray) -> np.ndarray:
    return bucket64(b64, th)


def cdf_linear(p: np.ndarray, borders, th) -> np.ndarray:
    """[R] float64: the CDF the sampler inverts -- linear inside every bar, the two end bars
    included -- of row r of p [R, nb] (divided by its sum) at th[r]."""
    b = np.asarray(borders, dtype=np.float64)
    th = np.asarray(th, dtype=np.float64)
    j = bucket64(b, th)
    out = np.empty(th.shape[0])
    for r in range(th.shape[0]):
        tot = math.fsum(p[r])
        w = b[j[r] + 1] - b[j[r]]
        frac = min(max((th[r] - b[j[r]]) / w, 0.0), 1.0) if w > 0 else 1.0
        out[r] = (math.fsum(p[r, :j[r]]) + p[r, j[r]] * frac) / tot if tot > 0 else np.nan
    return out


def icdf_linear(p: np.ndarray, borders, u) -> np.ndarray:
    """[R] float64 draws: the first bar with mass whose cumulative sum reaches u, linear inside."""
    b = np.asarray(borders, dtype=np.float64)
    out = np.full(len(u), np.nan)
    for r in range(len(u)):
        tot = math.fsum(p[r])
        if not tot > 0:
            continue
        c = np.cumsum(p[r]) / tot
        mass = np.nonzero(p[r] > 0)[0]
        hit = mass[c[mass] >= u[r]]
        j = hit[0] if hit.size else mass[-1]
        frac = min(max((u[r] - (c[j] - p[r, j] / tot)) / (p[r, j] / tot), 0.0), 1.0)
        out[r] = b[j] + (b[j + 1] - b[j]) * frac
    return out


def log_density(p: np.ndarray, borders, y) -> np.ndarray:
    """[R] float64: the full-support bar log density of y[r] under row r of p (npfn_bar_nll,
    negated): log(p_j / sum p) - log w_j in y's bucket j, plus the half-normal term in an end
    bar.  -inf for a bar without mass, NaN for a row without mass."""
    b = np.asarray(borders, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    nb = b.shape[0] - 1
    j = bucket64(b, np.nan_to_num(y, nan=0.0))
    out = np.empty(y.shape[0])

    def end(w, d):
        s = w / HM
        v = max(d, 1e-8)
        return math.log(math.sqrt(2.0 / math.pi) / s) - v * v / (2.0 * s * s) + math.log(w)

    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(y.shape[0]):
            tot = math.fsum(p[r])
            if not tot > 0:
                out[r] = np.nan
                continue
            k = int(j[r])
            w = b[k + 1] - b[k]
            lp = np.log(p[r, k] / tot) - np.log(w)
            if k == 0:
                lp += end(w, b[1] - y[r])
            if k == nb - 1:
                lp += end(w, y[r] - b[nb - 1])
            out[r] = lp
    return out


def cdf(p: np.ndarray, borders, y) -> np.ndarray:
    """[R] float64: npfn_bar_cdf's definition (tests/bar_cdf_ref.py) under the rows of p; NaN for
    a row without mass."""
    return cdf_from_probs(p, np.asarray(borders, dtype=np.float64), y)


def target_translation_host(bz, ylam, ystats):
    """k_target_tf's table from the oracle's functions, given the device's lambda and statistics
    (ystats [6]: common mean / std in [0], [1], the transformed target's in [3], [4]):
    (idx int32 [nb + 1], share float32 [nb + 1] with the flags folded in as -1 / 2, tcancel uint8
    [nb], frm float32 [nb + 1] the repaired source borders)."""
    bz = np.asarray(bz, dtype=np.float32)
    frm = yeo_johnson_inverse(bz.astype(np.float64) * np.float64(np.float32(ystats[4])) + np.float64(np.float32(ystats[3])),
                              float(ylam))
    frm, cancel = cancel_broken_borders(frm)
    frm32 = frm.astype(np.float32)
    idx, share, flag = translation_table(frm32, borders32(bz, ystats))
    share = np.where(flag < 0, np.float32(-1), np.where(flag > 0, np.float32(2), share)).astype(np.float32)
    return idx, share, cancel.astype(np.uint8), frm32


def oracle_table(y, bz):
    """The oracle's own fit of a target y on the standard borders bz: (table triple, ystats [6],
    lambda), as OracleTabPFN.fit computes them."""
    from oracle.preprocess_oracle import power_transform_vec, yj_fit
    from oracle.tabpfn_oracle import OracleTabPFN

    y = np.asarray(y, dtype=np.float32)
    m, s, z, _ = OracleTabPFN._ystats(y)
    lam = yj_fit(y)
    tm, ts, tz, _ = OracleTabPFN._ystats(power_transform_vec(y, lam))
    ystats = np.array([m, s, z, tm, ts, tz], dtype=np.float32)
    idx, share, tc, _ = target_translation_host(bz, lam, ystats)
    return (idx, share, tc), ystats, lam


def mix_bar(p_ref: np.ndarray, n_translated: int, E: int) -> np.ndarray:
    """The per-bar bound of tests/test_gpu_mix.py for the arithmetic mean: 2e-5 p_ref for the
    argument rounding of __expf over a logit range of ~20 and its last bits, plus, per translated
    estimator, the rounded additions on the way to the two prefix sums a translated bar is the
    difference of (the serial segment of ceil(nb / 256) bars, six wave steps, three wave bases,
    the share product: all sums <= 1, 2^-24 each)."""
    nb = p_ref.shape[-1]
    return 2e-5 * p_ref + delta_abs(nb) * n_translated / E


def delta_abs(nb: int) -> float:
    return 2.0 * (-(-nb // 256) + 16) * 2.0 ** -24


def rel_rows(lg16, invT) -> np.ndarray:
    """[R] the relative term of the bars: 2e-5, or 2^-23 x the row's scaled logit range where that
    is more (x * invT is rounded to float32 before the maximum is subtracted: half an ulp at
    |x| invT for each of the two values of a difference)."""
    x = np.asarray(lg16).astype(np.float64) * float(invT)
    fin = np.isfinite(x)
    hi = np.where(fin, x, -np.inf).max((0, 2))
    lo = np.where(fin, x, np.inf).min((0, 2))
    with np.errstate(invalid="ignore"):
        rng = np.where(np.isfinite(hi) & np.isfinite(lo), hi - lo, 0.0)
    return np.maximum(2e-5, 2.0 ** -23 * rng)


def arith_fraction(p, ref, lg16, invT, n_tr, E):
    """The arithmetic-mean bar applied to p [R, nb] against ref: (largest |p - ref| / bar, its
    (row, bar), whether every bar and row the reference leaves without mass and without a bar is
    exactly zero in p)."""
    nb = ref.shape[1]
    bar = rel_rows(lg16, invT)[:, None] * ref + delta_abs(nb) * n_tr / E
    # float32 has no relative precision below its smallest normal number (2^-126; the device's exp
    # flushes there): masses under 2^-120 are held to 2^-120 absolutely
    bar = np.where(ref > 0, np.maximum(bar, 2.0 ** -120), bar)
    d = np.abs(np.asarray(p, dtype=np.float64) - ref)
    zero = bar == 0
    dead = ref.sum(1) == 0
    zeros_ok = bool((p[zero] == 0).all() and (p[dead] == 0).all())
    frac = np.where(zero, 0.0, d / np.where(zero, 1.0, bar))
    return float(frac.max()), np.unravel_index(frac.argmax(), frac.shape), zeros_ok


def structural_zero(logits16, invT, ett=None, table=None) -> np.ndarray:
    """[R, nb] bool: bars that are zero by structure, whatever the rounding -- in some estimator
    the bar's logit is -inf (untranslated), the row is empty, or (translated) both of the bar's
    borders take the same CDF value without a rounded operation between them: both forced to 0
    (first border, flag -1, or a source bucket without mass and without mass before it) or both
    forced to 1 (last border, flag 2), or both inside the SAME source bucket without mass (one
    prefix sum, read twice).  A zero of the float64 reference that is the difference of two equal
    prefix sums read at DIFFERENT source buckets (a run of -inf logits in a translated row) is not
    structural: a float32 scan forms the two prefixes by different additions, equal to rounding
    only, and what is left of their difference (at most delta) is mass to the mean of logs.  The
    bar below the first border forced to 1 is of that kind too: it takes 1 - fl(prefix)."""
    lg = np.asarray(logits16, dtype=np.float16).astype(np.float64) * np.float64(np.float32(invT))
    E, R, nb = lg.shape
    out = np.zeros((R, nb), dtype=bool)
    for e in range(E):
        if ett is None or not ett[e]:
            out |= np.isneginf(lg[e]) | ~np.isfinite(lg[e]).any(-1, keepdims=True)
            continue
        idx, share, tcancel = table
        idx = np.asarray(idx)
        x = np.where(np.asarray(tcancel, dtype=bool)[None, :], -np.inf, lg[e])
        q = softmax_rows64(x)
        before = np.cumsum(q, axis=1) - q
        cls = np.full((R, nb + 1), -1, dtype=np.int64)          # -1: a rounded value; else a class id
        src0 = q[:, idx] == 0
        cls = np.where(src0, idx[None, :] + 2, cls)               # the bucket's own prefix, read as it is
        cls = np.where(src0 & (before[:, idx] == 0), 0, cls)      # sums of zeros are exact
        sh = np.asarray(share)
        cls = np.where(sh[None, :] < 0, 0, np.where(sh[None, :] > 1.5, 1, cls))
        cls[:, 0], cls[:, nb] = 0, 1
        out |= ((cls[:, 1:] == cls[:, :-1]) & (cls[:, 1:] >= 0)) | (q.sum(-1, keepdims=True) == 0)
    return out


def geo_fraction(p, ref, q, structural, ett, lg16, invT):
    """The geo bar (tests/test_gpu_mix.py) applied to p [R, nb] against ref = softmax(mean_e log
    q_e), q [E, R, nb]: (largest |log p - log ref - row median| / bar over the compared bars, the
    largest excused share of the bars with mass among the random rows, whether the reference's
    structural zeros (:func:`structural_zero`) are exact zeros in p, whether every compared bar
    kept its mass)."""
    E, R, nb = q.shape
    p = np.asarray(p)
    must0 = (ref == 0) & structural
    zeros_ok = bool((p[must0] == 0).all())
    tol = np.repeat(rel_rows(lg16, invT)[:, None], nb, 1)
    excused = np.zeros((R, nb), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(E):
            if ett is not None and ett[e]:
                t = delta_abs(nb) / q[e]
                excused |= ~(t <= 0.5)
                tol += np.where(np.isfinite(t), t, 0.0) / E
    live = ref > 2.0 ** -120
    worst, ex_share, kept = 0.0, 0.0, True
    for r in range(R):
        mass = live[r].sum()
        if mass == 0:
            continue
        if r < N_RANDOM:
            ex_share = max(ex_share, (excused[r] & live[r]).sum() / mass)
        cmp_ = live[r] & ~excused[r]
        if not cmp_.any():
            continue
        if not (p[r, cmp_] > 0).all():   # counted, and the rest of the row is still compared
            kept = False
            cmp_ &= p[r] > 0
            if not cmp_.any():
                continue
        d = np.log(p[r, cmp_].astype(np.float64)) - np.log(ref[r, cmp_])
        d -= np.median(d)
        worst = max(worst, float((np.abs(d) / tol[r, cmp_]).max()))
    return worst, float(ex_share), zeros_ok, kept


# ------------------------------------------------------------------ the test matrix's inputs
TARGETS = ("z", "exp", "-exp")
ETT_PATTERNS = ([0], [1], [0, 1], [1, 0], [0, 1, 0], [1, 1, 1], [0, 0, 1, 1, 0, 0, 1, 1])
N_ROWS = 16
ROW_ONE_BAR, ROW_CANCELLED, ROW_HUGE, ROW_THREE, ROW_EMPTY_EST, ROW_EMPTY_ALL = 10, 11, 12, 13, 14, 15
N_RANDOM = 10   # rows 0..9: N(0, scale^2) logits


def target_values(name: str, n: int = 64, seed: int = 0) -> np.ndarray:
    z = np.random.default_rng(seed).normal(size=n)
    return {"z": z, "exp": np.exp(1.5 * z), "-exp": -np.exp(1.5 * z)}[name].astype(np.float32)


def tables_for(nb: int):
    """{target: (table triple, ystats [6], lambda)} on synthetic_borders(nb), and the borders."""
    from npe_pfn.weights import synthetic_borders

    bz = synthetic_borders(nb)
    return {t: oracle_table(target_values(t), bz) for t in TARGETS}, bz


def case_logits(nb: int, E: int, tcancel, seed: int, scale: float = 1.0) -> np.ndarray:
    """fp16 [E, 16, nb]: ten N(0, scale^2) rows; a row with all its mass in one bar; a row with
    mass only in bars the table cancels (the last quarter of the bars when it cancels none); a
    row holding +-65504; a row that is -inf except for 3 bars; a row whose LAST estimator has no
    finite logit; a row where no estimator has one."""
    rng = np.random.default_rng(seed)
    lg = (scale * rng.normal(size=(E, N_ROWS, nb))).astype(np.float16)
    k = int(rng.integers(nb))
    lg[:, ROW_ONE_BAR] = np.float16(-40.0)
    lg[:, ROW_ONE_BAR, k] = np.float16(20.0)
    can = np.asarray(tcancel, dtype=bool)
    if not can.any():
        can = np.arange(nb) >= nb - max(nb // 4, 1)
    lg[:, ROW_CANCELLED] = np.where(can[None, :], lg[:, ROW_CANCELLED], np.float16(-np.inf))
    lg[:, ROW_HUGE, int(rng.integers(nb))] = np.float16(-65504.0)
    lg[:, ROW_HUGE, k] = np.float16(65504.0)
    three = rng.permutation(nb)[:3]
    keep = np.zeros(nb, dtype=bool)
    keep[three] = True
    lg[:, ROW_THREE] = np.where(keep[None, :], lg[:, ROW_THREE], np.float16(-np.inf))
    lg[E - 1, ROW_EMPTY_EST] = np.float16(-np.inf)
    lg[:, ROW_EMPTY_ALL] = np.float16(-np.inf)
    return lg
