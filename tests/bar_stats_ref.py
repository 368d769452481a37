"""fp64 numpy restatement of the bar distribution's summaries (npfn_bar_stats / npfn_predict_stats).

[ext: tabpfn 2.2.1 FullSupportBarDistribution.mean / .median / .mode / .icdf], restated the way
oracle/tabpfn_oracle.py restates ``sample`` and the NLL.  Inputs are fp32 logits [R, nb] and
fp32 borders [nb + 1]; everything is computed in fp64 on those values.

* :func:`ref_icdf` IS ``oracle.tabpfn_oracle.bar_sample(logits, borders, u=q)``.  That function
  takes ``searchsorted(cdf, u, 'left')``, which at u = 0 answers bar 0 even when bar 0 has no mass
  and then divides 0 by 0; those entries (and only those: the ones it returns non-finite) are
  filled from :func:`ref_icdf64`, the same definition with "the first bar WITH MASS whose
  cumulative sum reaches q" spelled out (tests/test_bar_stats_host.py pins the two to each other
  wherever the oracle is finite).  Its probabilities are an fp32 softmax, so it cannot place
  the last ~1e-3 of the mass (check_quantiles below has the figures); ref_icdf64 can.
* :func:`ref_cdf` is the piecewise-linear CDF that :func:`ref_icdf64` inverts.
"""
import numpy as np

from oracle.tabpfn_oracle import HALFNORMAL_MEDIAN, bar_sample

SQRT_2_OVER_PI = float(np.sqrt(2.0 / np.pi))


def probs64(logits: np.ndarray) -> np.ndarray:
    """softmax of the fp32 logits in fp64 (rows without a finite logit give NaN)."""
    lg = np.asarray(logits, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(lg - lg.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)


def bar_means(borders: np.ndarray) -> np.ndarray:
    """m_j: bar centres, and the half-normal means of the two tail bars."""
    b = np.asarray(borders, dtype=np.float32).astype(np.float64)
    w = np.diff(b)
    m = b[:-1] + w / 2
    m[0] = b[1] - (w[0] / HALFNORMAL_MEDIAN) * SQRT_2_OVER_PI
    m[-1] = b[-2] + (w[-1] / HALFNORMAL_MEDIAN) * SQRT_2_OVER_PI
    return m


def ref_mean(logits: np.ndarray, borders: np.ndarray) -> np.ndarray:
    return probs64(logits) @ bar_means(borders)


def ref_mode_density(logits: np.ndarray, borders: np.ndarray) -> np.ndarray:
    """p_j / w_j [R, nb]; bars of zero width are -inf (never the mode)."""
    w = np.diff(np.asarray(borders, dtype=np.float32).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = probs64(logits) / w
    return np.where(w > 0, d, -np.inf)


def _rowwise(q, R: int) -> np.ndarray:
    return np.broadcast_to(np.asarray(q, dtype=np.float64), (R,)).copy()


def ref_icdf64(logits: np.ndarray, borders: np.ndarray, q) -> np.ndarray:
    """icdf(q) per row in fp64 (q a scalar or one level per row): the first bar with mass whose
    cumulative sum reaches q (the last bar with mass if none does), linear inside it."""
    p = probs64(logits)
    R, nb = p.shape
    q = _rowwise(q, R)
    b = np.asarray(borders, dtype=np.float32).astype(np.float64)
    cdf = np.cumsum(p, axis=1)
    cdf0 = np.concatenate([np.zeros((R, 1)), cdf[:, :-1]], axis=1)
    out = np.empty(R)
    for i in range(R):
        ok = np.flatnonzero((p[i] > 0) & (cdf[i] >= q[i]))
        j = ok[0] if ok.size else np.flatnonzero(p[i] > 0)[-1]
        frac = min(max((q[i] - cdf0[i, j]) / p[i, j], 0.0), 1.0)
        out[i] = b[j] + (b[j + 1] - b[j]) * frac
    return out


def ref_icdf(logits: np.ndarray, borders: np.ndarray, q) -> np.ndarray:
    """oracle.tabpfn_oracle.bar_sample(logits, borders, u=q) (float32), its 0 / 0 entries -- a
    zero-mass bar picked at q = 0 -- filled from :func:`ref_icdf64`."""
    R = np.asarray(logits).shape[0]
    q = _rowwise(q, R)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = bar_sample(logits, borders, q)
    bad = ~np.isfinite(x)
    if bad.any():
        x = x.copy()
        x[bad] = ref_icdf64(np.asarray(logits)[bad], borders, q[bad]).astype(np.float32)
    return x


def ref_cdf(logits: np.ndarray, borders: np.ndarray, x) -> np.ndarray:
    """Piecewise-linear CDF per row at x (one point per row): mass of the bars left of x plus the
    linear share of x's bar; 0 / 1 outside the borders."""
    p = probs64(logits)
    R, nb = p.shape
    x = _rowwise(x, R)
    b = np.asarray(borders, dtype=np.float32).astype(np.float64)
    cdf0 = np.concatenate([np.zeros((R, 1)), np.cumsum(p, axis=1)], axis=1)
    j = np.clip(np.searchsorted(b, x, side="right") - 1, 0, nb - 1)
    rows = np.arange(R)
    w = b[j + 1] - b[j]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(w > 0, np.clip((x - b[j]) / w, 0.0, 1.0), 0.0)
    return cdf0[rows, j] + p[rows, j] * frac


# ------------------------------------------------- assertions shared by the GPU test files
def ulp32(x) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


ORACLE_MIN_TAIL = 1e-2   # the oracle's bar_sample is compared where 1 - q is at least this


def check_quantiles(x_dev: np.ndarray, logits: np.ndarray, borders: np.ndarray, qs, what: str = "") -> None:
    """x_dev [len(qs), R] (qs ascending): within 1e-4 of the border span -- what the project holds
    bar_sample to -- of the fp64 definition (ref_icdf64) at every q, and of the oracle's bar_sample
    (ref_icdf) wherever 1 - q >= ORACLE_MIN_TAIL; inside the borders; non-decreasing in q.

    Why the oracle is not asked about the last 1 % of the mass: it takes its probabilities from
    an fp32 softmax (each p and the normaliser rounded to 2^-24), so its CDF carries ~2^-23 of
    the total, and a position error is the CDF error over the density -- unbounded where the
    remaining mass is of that order.  On the inputs of test_gpu_bar_stats.py the oracle itself
    is 2.3e-2 (q = 1 - 1e-6) and 3.7e-2 (q = 1) away from the fp64 definition at 5000 bars and
    2.35e-3 at 1024, against bounds of 2.2e-3 and 1.9e-3; up to q = 0.99 it stays within 3e-5
    (measured on the CPU, no device involved).  At q = 1 it also depends on whether its rounded
    probabilities sum to 1, where the definition is plain: the right border of the last bar
    with mass."""
    b = np.asarray(borders, dtype=np.float32)
    span = float(b[-1]) - float(b[0])
    assert x_dev.shape == (len(qs), np.asarray(logits).shape[0]) and x_dev.dtype == np.float32
    for i, q in enumerate(qs):
        q = float(np.float32(q))   # the level the device is given: the ABI's quantiles are float32
        x = x_dev[i].astype(np.float64)
        err = np.abs(x - ref_icdf64(logits, borders, q))
        print(f"{what} q={q!r}: max |x - fp64 definition| = {err.max():.3e} (bound {1e-4 * span:.3e})")
        assert err.max() <= 1e-4 * span, (what, q, int(err.argmax()), err.max())
        if 1.0 - q >= ORACLE_MIN_TAIL:
            err = np.abs(x - ref_icdf(logits, borders, q).astype(np.float64))
            print(f"{what} q={q!r}: max |x - oracle bar_sample| = {err.max():.3e}")
            assert err.max() <= 1e-4 * span, (what, q, int(err.argmax()), err.max())
    assert (x_dev >= b[0]).all() and (x_dev <= b[-1]).all(), what
    assert (np.diff(x_dev, axis=0) >= 0).all(), what


def check_mean(mean_dev: np.ndarray, logits: np.ndarray, borders: np.ndarray, what: str = "") -> None:
    """|mean - ref| <= 2e-5 span + 4 ulp32(|ref|): __expf on arguments up to ~90 in magnitude has
    relative error eps <= 90 * 2^-24 + 2^-22 ~ 6e-6; the normalised mean then errs by at most
    2 eps E|m - mean| <= 2 eps span / 2, which leaves a margin of about 3x."""
    b = np.asarray(borders, dtype=np.float32)
    span = float(b[-1]) - float(b[0])
    ref = ref_mean(logits, borders)
    err = np.abs(mean_dev.astype(np.float64) - ref)
    bound = 2e-5 * span + 4 * ulp32(ref)
    print(f"{what} mean: max |mean - ref| = {err.max():.3e} (bound {bound.min():.3e})")
    assert mean_dev.dtype == np.float32 and (err <= bound).all(), (what, int((err - bound).argmax()), err.max())


def check_mode(mode_dev: np.ndarray, logits: np.ndarray, borders: np.ndarray, what: str = "") -> np.ndarray:
    """The bar recovered from the returned centre has (1 - 1e-5) of the largest reference density
    (near-ties may resolve either way) and the value is b[j] + w_j / 2 within 2 ulp; returns j."""
    b = np.asarray(borders, dtype=np.float32).astype(np.float64)
    centres = b[:-1] + np.diff(b) / 2
    dens = ref_mode_density(logits, borders)
    j = np.abs(centres[None, :] - mode_dev.astype(np.float64)[:, None]).argmin(1)
    rows = np.arange(len(j))
    assert (np.abs(mode_dev.astype(np.float64) - centres[j]) <= 2 * ulp32(centres[j])).all(), what
    ratio = dens[rows, j] / dens.max(1)
    print(f"{what} mode: min density ratio = {ratio.min():.8f}")
    assert (ratio >= 1 - 1e-5).all(), (what, int(ratio.argmin()), ratio.min())
    return j
