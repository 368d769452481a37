"""fp64 numpy restatement of npfn_bar_cdf (include/npfn.h): the CDF of the full-support bar
distribution, the integral of exactly the density whose negative log
oracle.tabpfn_oracle.bar_nll returns.  Written row by row with math.erf / math.erfc, apart from
the engine and from npe_pfn.diagnostics.bar_cdf, which the tests compare against it."""
import math

import numpy as np

HM = 0.6744897501960817  # the half-normal median: the tail bars' scale is width / HM


def cdf_row(p: np.ndarray, b: np.ndarray, j: int, y: float) -> float:
    """F(y) of one row: p [nb] normalized fp64 probabilities, b [nb + 1] fp64 borders, j the bucket
    of y.  Formed from the side with less mass (S_left <= S_right: from the left)."""
    nb = p.shape[0]
    if math.isnan(y) or not np.isfinite(p).all():
        return float("nan")
    if y == -math.inf:
        return 0.0
    if y == math.inf:
        return 1.0
    w = b[j + 1] - b[j]
    if w <= 0.0:
        frac, rest = 1.0, 0.0
    elif j == 0:
        z = max(b[1] - y, 0.0) / (w / HM * math.sqrt(2.0))
        frac, rest = math.erfc(z), math.erf(z)
    elif j == nb - 1:
        z = max(y - b[nb - 1], 0.0) / (w / HM * math.sqrt(2.0))
        frac, rest = math.erf(z), math.erfc(z)
    else:
        frac = min(max((y - b[j]) / w, 0.0), 1.0)
        rest = 1.0 - frac
    s_left = math.fsum(p[:j])
    s_right = math.fsum(p[j + 1:])
    if s_left <= s_right:
        return s_left + p[j] * frac
    return 1.0 - (s_right + p[j] * rest)


def softmax64(logits: np.ndarray) -> np.ndarray:
    lg = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(lg - lg.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def bucket64(b: np.ndarray, y: np.ndarray) -> np.ndarray:
    """The NLL's bucket rule (oracle bar_bucket: searchsorted left - 1, the two end-border
    fix-ups, clamped) on fp64 values, so that a y between two fp32 numbers keeps its place; on
    fp32-representable inputs it is bar_bucket itself (asserted in tests/test_bar_cdf_host.py)."""
    nb = b.shape[0] - 1
    idx = np.searchsorted(b, y, side="left") - 1
    idx = np.where(y == b[0], 0, idx)
    idx = np.where(y == b[-1], nb - 1, idx)
    return np.clip(idx, 0, nb - 1)


def cdf_from_probs(p: np.ndarray, borders: np.ndarray, y: np.ndarray) -> np.ndarray:
    """[N] fp64: F(y_i) under row i of the probabilities p [N, nb] (divided by their row sums)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        p = p / p.sum(-1, keepdims=True)
    b = np.asarray(borders, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    idx = bucket64(b, np.nan_to_num(yv, nan=0.0))
    return np.array([cdf_row(p[i], b, int(idx[i]), float(yv[i])) for i in range(p.shape[0])], dtype=np.float64)


def bar_cdf_ref(logits: np.ndarray, borders: np.ndarray, y: np.ndarray) -> np.ndarray:
    """[N] fp64: F(y_i) under softmax(row i of logits [N, nb]) on borders [nb + 1], every input
    taken at the precision it is given in."""
    return cdf_from_probs(softmax64(logits), borders, y)
