"""numpy fp64 references, derived error bounds and shared cases for the support kernels K9-K12
(csrc/npfn_support.hip).  Test infrastructure only.

K12 (``npfn_filter_stdeuclid``)
    The kernel rounds each column's mean and unbiased std (fp64 sums of the fp32 values) to fp32
    and evaluates the standardised distance in fp32.  :func:`filter_rank` restates that with the
    same rounded statistics and everything after them in fp64, and returns per row a bound on
    what the fp32 evaluation may move the distance d_i:

        bound_i = 4 * 2^-24 * ( sqrt(sum_j (|xs_ij| + |os_j|)^2) + (dim + 3) * d_i )

    Derivation (u = 2^-24, the fp32 unit roundoff).  xs_ij = fl(fl(x - m) / sd) and
    os_j = fl(fl(obs - m) / sd) carry two roundings each, so they are off by at most
    2u |xs_ij| and 2u |os_j|; the subtraction adds one more rounding of the difference, and the
    cancellation in it keeps the absolute, not the relative, error: |delta_ij| <=
    2u (|xs_ij| + |os_j|) + u |df_ij|.  A perturbation delta of the vector df moves its norm by at
    most |delta| (triangle inequality), which gives 2u sqrt(sum_j (|xs_ij| + |os_j|)^2) + u d_i.
    The dim squares, the dim accumulations and the root each add at most u relative to the sum
    of squares, i.e. (dim + 1) u d_i on the root after halving and one rounding of the root itself;
    together below (dim + 3) u d_i with the term before.  Times a 4x margin.

    :func:`check_filter` accepts an index list only if every order violation against the fp64
    distances is explained by that bound; :func:`filter_in_band` counts the rows that are within
    their bound of the k-th distance (the rows whose membership the bound leaves open), which the
    host test caps, so that the acceptance cannot go slack.

K11 (``npfn_sir_select``)
    The device and oracle/support_oracle.py form the same fp32 ``exp`` terms and add them in
    fp64.  Each ``expf`` is within 1 ulp on either side, so two evaluations of a term agree to
    2 * 2^-23 = 2^-22 relative, and so do the (all-positive) sums and every CDF step; with a 4x
    margin a pick may differ from the oracle's only where every CDF step between the two picks
    lies within 2^-20 * s of the target u * s (:func:`sir_mismatch_is_rounding`).
    :func:`sir_in_band` counts the groups in which that can happen at all.
"""
from __future__ import annotations

import numpy as np

from oracle.philox import uniforms
from oracle.support_oracle import log_ratios

U24 = 2.0 ** -24
SIR_BAND = 2.0 ** -20

# ------------------------------------------------------------------ K12 cases
# (n, dim, k, shift): standard-normal rows (+ shift on every column), obs = 0.5 * normal + shift
FILTER_SHAPES = [(257, 1, 100, 0.0), (1000, 4, 100, 0.0), (4097, 33, 1000, 0.0), (65537, 4, 5000, 0.0),
                 (3, 2, 2, 0.0), (2, 1, 1, 0.0), (1000, 4, 100, 1000.0)]
FILTER_SHAPES += [(n, 3, k, 0.0) for n in (255, 256, 257) for k in (1, n - 1, n)]
# cases whose first draw put a column statistic within 1e-9 of an fp32 rounding midpoint (a
# condition of tests/test_support_ref_host.py; with 66 statistics most draws of the 33-column
# case do) draw again
FILTER_RESEED = {(4097, 33, 1000): 100013, (255, 3, 255): 100000}


def filter_case(n: int, dim: int, k: int, shift: float = 0.0):
    """x [n, dim] float32, obs [dim] float32 of one FILTER_SHAPES entry."""
    rng = np.random.default_rng(7000 + 31 * n + 7 * dim + k + FILTER_RESEED.get((n, dim, k), 0))
    x = (rng.standard_normal((n, dim)) + shift).astype(np.float32)
    obs = (0.5 * rng.standard_normal(dim) + shift).astype(np.float32)
    return x, obs


def column_stats64(x: np.ndarray):
    """fp64 column mean and unbiased std (two passes) of the fp32 values."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x64.shape[0]
    mean = x64.sum(axis=0) / n
    std = np.sqrt(((x64 - mean) ** 2).sum(axis=0) / max(n - 1, 1))
    return mean, std


def midpoint_margin(v: np.ndarray) -> float:
    """Smallest relative distance of an fp64 value from the midpoint of its two fp32 neighbours."""
    v = np.asarray(v, dtype=np.float64).ravel()
    f = v.astype(np.float32)
    lo = np.where(f.astype(np.float64) <= v, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    return float(np.min(np.abs(v - mid) / np.abs(v)))


def filter_rank(x: np.ndarray, obs: np.ndarray):
    """(d [n] fp64, bound [n] fp64): the standardised distance from the fp32-rounded column
    statistics, evaluated in fp64, and the derived bound on its fp32 evaluation."""
    x = np.asarray(x, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32).reshape(-1)
    dim = x.shape[1]
    mean, std = column_stats64(x)
    m = mean.astype(np.float32).astype(np.float64)
    sd = std.astype(np.float32).astype(np.float64)
    xs = (x.astype(np.float64) - m) / sd
    os_ = (obs.astype(np.float64) - m) / sd
    d = np.sqrt(((xs - os_) ** 2).sum(axis=1))
    bound = 4.0 * U24 * (np.sqrt(((np.abs(xs) + np.abs(os_)) ** 2).sum(axis=1)) + (dim + 3) * d)
    return d, bound


def filter_emulate_fp32(x: np.ndarray, obs: np.ndarray) -> np.ndarray:
    """The kernel's arithmetic in numpy float32, every operation rounded on its own (no FMA)."""
    x = np.asarray(x, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32).reshape(-1)
    mean, std = column_stats64(x)
    m, sd = mean.astype(np.float32), std.astype(np.float32)
    acc = np.zeros(x.shape[0], np.float32)
    for j in range(x.shape[1]):
        df = (x[:, j] - m[j]) / sd[j] - (obs[j] - m[j]) / sd[j]
        acc = acc + df * df
    return np.sqrt(acc)


def filter_in_band(x: np.ndarray, obs: np.ndarray, k: int) -> int:
    """Rows within their bound of the k-th smallest distance (the k-th row itself included)."""
    d, bound = filter_rank(x, obs)
    dk = np.sort(d)[k - 1]
    return int(np.count_nonzero(np.abs(d - dk) <= bound))


def filter_band_cap(k: int) -> int:
    """At most 4 rows and at most 1 % of k; the k-th row itself always counts, hence at least 1."""
    return min(4, max(1, k // 100))


def check_filter(idx, x: np.ndarray, obs: np.ndarray, k: int) -> float:
    """Assert that ``idx`` is an acceptable answer of K12 and return the largest share of the
    bound that any order violation against the fp64 distances used (0 when the order is the
    fp64 order)."""
    idx = np.asarray(idx).astype(np.int64).ravel()
    n = x.shape[0]
    assert idx.shape == (k,), (idx.shape, k)
    assert k == 0 or (idx.min() >= 0 and idx.max() < n), "index out of range"
    assert np.unique(idx).size == k, "repeated index"
    if k == 0:
        return 0.0
    d, bound = filter_rank(x, obs)
    dk = np.sort(d)[k - 1]
    sel = np.zeros(n, bool)
    sel[idx] = True
    over = (d[sel] - dk) / bound[sel]            # selected rows may pass d_(k) by their bound
    use = max(0.0, float(over.max()))
    assert use <= 1.0, f"a selected row lies {use:.3g} bounds above the k-th distance"
    if k < n:
        under = (dk - d[~sel]) / bound[~sel]     # unselected rows may fall short of it likewise
        u2 = max(0.0, float(under.max()))
        assert u2 <= 1.0, f"an unselected row lies {u2:.3g} bounds below the k-th distance"
        use = max(use, u2)
    if k > 1:
        a, b = idx[:-1], idx[1:]
        inv = (d[a] - d[b]) / (bound[a] + bound[b])
        u3 = max(0.0, float(inv.max()))
        assert u3 <= 1.0, f"consecutive outputs are out of order by {u3:.3g} bounds"
        use = max(use, u3)
    return use


# ------------------------------------------------------------------ K11 cases
SIR_SHAPES = [(1000, 100), (257, 7), (64, 300), (50, 1), (33, 64), (20, 4096),
              (5, 63), (6, 65), (7, 129), (3, 127), (1, 64), (2, 128)]
SIR_SEED, SIR_COUNTER = 99, 5


def sir_case(G: int, k: int, seed: int, afn: float = 0.1, nan_every: int = 0, width: int = 3):
    """(theta [G k, width], lpr, lq [G k], thr) as torch tensors: random log densities with
    -inf priors, optional NaN ratios, and the threshold at the ``afn`` quantile of lq."""
    import torch

    g = torch.Generator().manual_seed(seed)
    lq = torch.randn(G * k, generator=g) * 4
    lpr = torch.randn(G * k, generator=g)
    lpr[::13] = -float("inf")
    if nan_every:
        lq[::nan_every] = -float("inf")
        lpr[::nan_every] = -float("inf")  # -inf - -inf = NaN -> -inf ratio
    thr = torch.quantile(lq[torch.isfinite(lq)], afn)
    th = torch.randn(G * k, width, generator=g)
    return th, lpr, lq, thr


def sir_shape_case(G: int, k: int):
    return sir_case(G, k, seed=G + k, nan_every=17 if k > 1 else 0)


def sir_steps(lpr, lq, thr: float, k: int, seed: int, counter: int, group_offset: int = 0):
    """(c [G, k], s [G], u [G]): the oracle's CDF steps, totals and uniforms per group (fp64).
    A group whose ratios are all -inf has s = 0."""
    lw = log_ratios(np.asarray(lpr), np.asarray(lq), thr).reshape(-1, k)
    m = lw.max(axis=1, keepdims=True).astype(np.float32)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        e = np.exp((lw - m).astype(np.float32)).astype(np.float64)
    e[np.isneginf(m[:, 0])] = 0.0
    c = np.cumsum(e, axis=1)
    u = uniforms(seed, counter, lw.shape[0], row_offset=group_offset).astype(np.float64)
    return c, c[:, -1].copy(), u


def sir_mismatch_is_rounding(c_g: np.ndarray, s_g: float, u_g: float, pick: int, ref: int) -> bool:
    """True if every CDF step between the two picks lies within 2^-20 * s of the target u * s."""
    lo, hi = min(int(pick), int(ref)), max(int(pick), int(ref))
    if not (0 <= lo and hi < c_g.shape[0]):
        return False
    return bool(np.all(np.abs(c_g[lo:hi] - u_g * s_g) <= SIR_BAND * s_g))


def sir_in_band(c: np.ndarray, s: np.ndarray, u: np.ndarray) -> int:
    """Groups whose target lies within 2^-20 * s of any CDF step."""
    hit = np.abs(c - (u * s)[:, None]) <= (SIR_BAND * s)[:, None]
    return int(np.count_nonzero(hit.any(axis=1) & (s > 0)))
