"""Calibration diagnostics of the autoregressive posterior, in torch (no scipy).

``bar_cdf`` is the host restatement (fp64) of the engine's ``npfn_bar_cdf`` (include/npfn.h): the
CDF of tabpfn's full-support bar distribution, the integral of exactly the density whose negative
log ``criterion(logits, y)`` returns.  ``NPE_PFN_Core.pit_batched`` uses it with every estimator
that has no fused ``ar_score`` (e.g. the CPU oracle).  ``pit_ks_statistic`` condenses the
per-dimension probability integral transform values ``u_k = F_k(theta_k | x, theta_<k)`` -- uniform
exactly when conditional k is calibrated -- into one Kolmogorov-Smirnov distance per dimension.

Coverage of the joint posterior (``NPE_PFN_Core.coverage_batched``): ``rank_accumulate_host`` is the
definition of the engine's ``npfn_rank_accumulate`` (and the path of estimators without an engine),
``CoverageRanks`` holds the simulation-based-calibration, HPD and TARP ranks it yields, and
``rank_ks_statistic`` / ``expected_coverage`` turn ranks into a uniformity distance and a coverage
curve.

Distance between two sets of draws (``mmd_batched``, ``NPE_PFN_Core.mmd_batched``): the reference
harness's MMD with a permutation null.  ``mmd_sums_host`` is the definition of the engine's
``npfn_mmd_sums``, ``permutation_labels`` the relabellings, ``TwoSampleResult`` what comes back.

Exact 2-Wasserstein distance between two equally sized sets of draws (``wasserstein_batched``,
``NPE_PFN_Core.wasserstein_batched``): the reference harness's ``sqrt(ot.emd2(...))`` as a linear
assignment problem on integer costs.  ``transport_costs_host`` and ``assignment_solve_host`` are
the definition of the engine's ``npfn_w2_assign``, ``TransportResult`` what comes back.

Classifier two-sample test (``c2st_batched``, ``NPE_PFN_Core.c2st_batched``): the reference
harness's C2ST, a small MLP per fold trained to tell the two sets apart, 0.5 = indistinguishable.
``c2st_folds``, ``c2st_order``, ``c2st_widths``, ``c2st_init`` and ``c2st_adam_table`` fix every
random and tabulated input on the host, ``c2st_fit_host`` is the definition of the engine's
``npfn_c2st_fit``, ``ClassifierTestResult`` what comes back.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .engine import (C2ST_BETAS, C2ST_EPS, C2ST_MAX_FOLDS, MMD_MAX_LABELLINGS, check_c2st_args, check_mmd_args,
                     check_transport_args)

HALFNORMAL_MEDIAN = 0.6744897501960817  # median of |N(0, 1)|: the tail bars' scale is width / this


def bar_cdf(logits, borders, y) -> Tensor:
    """F(y_i) under row i of ``logits`` [N, n_bars] on ``borders`` [n_bars + 1]; float64 [N] on
    the device of ``logits``.

    With p = softmax(logits row), w_j = b[j+1] - b[j] and j the bucket of y by the NLL's rule
    (searchsorted(b, y, left) - 1, the two end-border fix-ups, clamped): F = sum_{i<j} p_i +
    p_j frac, frac = clamp((y - b[j]) / w_j, 0, 1) in an inner bar, erfc(max(b[1] - y, 0) /
    (s0 sqrt 2)) in the left tail bar (a half-normal hanging left from b[1], s0 = w_0 /
    HALFNORMAL_MEDIAN), erf(max(y - b[n_bars-1], 0) / (s1 sqrt 2)) in the right one, 1 in a bar
    of width 0.  The result is formed from the side with less mass.  NaN for y = NaN or a row
    without a finite logit; 0 / 1 at y = -inf / +inf."""
    lg = torch.as_tensor(logits).detach().to(torch.float64)
    dev = lg.device
    b = torch.as_tensor(borders).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    yv = torch.as_tensor(y).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    if lg.ndim != 2 or b.shape[0] != lg.shape[1] + 1 or yv.shape[0] != lg.shape[0] or lg.shape[1] < 2:
        raise ValueError(f"bar_cdf: logits {tuple(lg.shape)}, borders {tuple(b.shape)} and y {tuple(yv.shape)} "
                         "do not match (n_bars >= 2)")
    nb = lg.shape[1]
    p = torch.softmax(lg, dim=-1)
    y_ok = torch.nan_to_num(yv, nan=0.0)   # NaN rows are answered at the end
    idx = torch.searchsorted(b, y_ok, right=False) - 1
    idx = torch.where(y_ok == b[0], torch.zeros_like(idx), idx)
    idx = torch.where(y_ok == b[-1], torch.full_like(idx, nb - 1), idx)
    idx = idx.clamp(0, nb - 1)
    zero = torch.zeros((lg.shape[0], 1), dtype=torch.float64, device=dev)
    left_mass = torch.cat([zero, torch.cumsum(p, 1)[:, :-1]], 1).gather(1, idx[:, None])[:, 0]
    right_mass = torch.cat([torch.cumsum(p.flip(1), 1).flip(1)[:, 1:], zero], 1).gather(1, idx[:, None])[:, 0]
    pj = p.gather(1, idx[:, None])[:, 0]
    left, right = b[idx], b[idx + 1]
    w = right - left
    pos = w > 0
    w_safe = torch.where(pos, w, torch.ones_like(w))
    scale = w_safe / HALFNORMAL_MEDIAN * math.sqrt(2.0)
    frac = ((y_ok - left) / w_safe).clamp(0.0, 1.0)
    rest = 1.0 - frac
    z0 = (right - y_ok).clamp(min=0.0) / scale
    z1 = (y_ok - left).clamp(min=0.0) / scale
    is_l, is_r = idx == 0, idx == nb - 1
    frac = torch.where(is_l, torch.erfc(z0), torch.where(is_r, torch.erf(z1), frac))
    rest = torch.where(is_l, torch.erf(z0), torch.where(is_r, torch.erfc(z1), rest))
    frac = torch.where(pos, frac, torch.ones_like(frac))
    rest = torch.where(pos, rest, torch.zeros_like(rest))
    out = torch.where(left_mass <= right_mass, left_mass + pj * frac, 1.0 - (right_mass + pj * rest))
    out = torch.where(yv == float("-inf"), torch.zeros_like(out), out)
    out = torch.where(yv == float("inf"), torch.ones_like(out), out)
    bad = torch.isnan(yv) | ~torch.isfinite(p.sum(1))
    return torch.where(bad, torch.full_like(out, float("nan")), out)


def pit_ks_statistic(pit: Tensor) -> Tensor:
    """Kolmogorov-Smirnov distance of each column of ``pit`` [n, d_theta] from the uniform
    distribution on [0, 1]: sup_u |ECDF(u) - u| per dimension, [d_theta] (the statistic of a
    one-sample KS test; no p-value).  Leading dimensions are flattened into n."""
    u = torch.as_tensor(pit)
    if u.ndim < 2 or u.shape[-1] < 1 or u.numel() == 0:
        raise ValueError(f"pit_ks_statistic: pit must be [n, d_theta] with n >= 1, got {tuple(u.shape)}")
    u = u.reshape(-1, u.shape[-1]).to(torch.float64)
    n = u.shape[0]
    s = torch.sort(u, dim=0).values
    i = torch.arange(1, n + 1, dtype=torch.float64, device=u.device)[:, None]
    d_plus = (i / n - s).max(dim=0).values
    d_minus = (s - (i - 1) / n).max(dim=0).values
    return torch.maximum(d_plus, d_minus)


# ------------------------------------------------------------------ coverage ranks
def rank_accumulate_host(theta, logp, take, n_obs: int, per: int, theta_true, logp_true, ref, inv_scale,
                         counts: Tensor) -> None:
    """Adds the rank counts of one sampler round to ``counts`` [n_obs, dim + 2, 2] (int64, in
    place; the caller zeroes it before the first round) -- the definition of the engine's
    ``npfn_rank_accumulate`` (``Engine.rank_accumulate``, same arguments), in torch on the device
    of ``counts``, every comparison in fp64 (exact for fp32 inputs).

    ``theta`` [n_obs * per, dim] is obs-major (row i belongs to observation i // per), ``logp``
    [n_obs * per]; a row takes part when ``take`` is None or ``take[i] != 0``.  For observation m
    and its rows s that take part, slot 0 counts "<" and slot 1 "==" of

    * column k < dim: ``theta[s, k]`` against ``theta_true[m, k]`` (simulation-based calibration);
    * column dim: ``logp_true[m]`` against ``logp[s]``, i.e. slot 0 counts the draws DENSER than
      the truth (HPD);
    * column dim + 1: ``d2(theta[s])`` against ``d2(theta_true[m])`` with d2(a) = sum over k
      ascending of t_k * t_k, t_k = (a_k - ref[m, k]) * inv_scale[k] in fp64, every multiply and
      add rounded on its own (TARP: the draws closer to the reference point than the truth).

    A NaN on either side counts in neither slot.  ``logp`` / ``logp_true`` may both be None (column
    dim is left alone), ``ref`` / ``inv_scale`` too (column dim + 1)."""
    n_obs, per = int(n_obs), int(per)
    dev = counts.device
    th = torch.as_tensor(theta).to(device=dev, dtype=torch.float64)
    if n_obs < 0 or per < 0 or th.ndim != 2 or th.shape[1] < 1 or th.shape[0] != n_obs * per:
        raise ValueError(f"rank_accumulate: theta {tuple(th.shape)} is not [{n_obs} * {per}, dim >= 1]")
    dim = th.shape[1]
    tt = torch.as_tensor(theta_true).to(device=dev, dtype=torch.float64)
    if tt.shape != (n_obs, dim):
        raise ValueError(f"rank_accumulate: theta_true {tuple(tt.shape)} is not [{n_obs}, {dim}]")
    if (logp is None) != (logp_true is None) or (ref is None) != (inv_scale is None):
        raise ValueError("rank_accumulate: logp / logp_true and ref / inv_scale are given in pairs")
    if counts.dtype != torch.int64 or counts.shape != (n_obs, dim + 2, 2):
        raise ValueError(f"rank_accumulate: counts must be an int64 [{n_obs}, {dim + 2}, 2] tensor")
    th = th.reshape(n_obs, per, dim)
    if take is None:
        on = torch.ones((n_obs, per), dtype=torch.bool, device=dev)
    else:
        on = torch.as_tensor(take).to(dev).reshape(-1) != 0
        if on.shape[0] != n_obs * per:
            raise ValueError(f"rank_accumulate: take has {on.shape[0]} entries, theta {n_obs * per} rows")
        on = on.reshape(n_obs, per)

    def add(col, less, equal):
        counts[:, col, 0] += (less & on).sum(1)
        counts[:, col, 1] += (equal & on).sum(1)

    for k in range(dim):
        add(k, th[:, :, k] < tt[:, None, k], th[:, :, k] == tt[:, None, k])
    if logp is not None:
        lp = torch.as_tensor(logp).to(device=dev, dtype=torch.float64).reshape(-1)
        lt = torch.as_tensor(logp_true).to(device=dev, dtype=torch.float64).reshape(-1)
        if lp.shape[0] != n_obs * per or lt.shape[0] != n_obs:
            raise ValueError(f"rank_accumulate: logp {tuple(lp.shape)} / logp_true {tuple(lt.shape)} do not match "
                             f"{n_obs} observations of {per} rows")
        lp = lp.reshape(n_obs, per)
        add(dim, lp > lt[:, None], lp == lt[:, None])
    if ref is not None:
        rf = torch.as_tensor(ref).to(device=dev, dtype=torch.float64)
        sc = torch.as_tensor(inv_scale).to(device=dev, dtype=torch.float64).reshape(-1)
        if rf.shape != (n_obs, dim) or sc.shape[0] != dim:
            raise ValueError(f"rank_accumulate: ref {tuple(rf.shape)} / inv_scale {tuple(sc.shape)} do not match "
                             f"[{n_obs}, {dim}] / [{dim}]")
        d2 = torch.zeros((n_obs, per), dtype=torch.float64, device=dev)
        d2t = torch.zeros(n_obs, dtype=torch.float64, device=dev)
        for k in range(dim):   # ascending, one rounding per operation: the kernel's own chain
            a = (th[:, :, k] - rf[:, None, k]) * sc[k]
            b = (tt[:, k] - rf[:, k]) * sc[k]
            d2 = d2 + a * a
            d2t = d2t + b * b
        add(dim + 1, d2 < d2t[:, None], d2 == d2t[:, None])


@dataclass
class CoverageRanks:
    """Rank statistics of M true parameters among ``num_samples`` posterior draws each
    (``NPE_PFN_Core.coverage_batched``).  Column k < d_theta of ``less`` / ``equal`` [M, d_theta +
    2] (int64) counts the draws whose theta_k is below / equal to the truth's, column d_theta the
    draws with a log density above / equal to the truth's, column d_theta + 1 the draws closer to
    / as close to ``references`` [M, d_theta] as the truth in the distance scaled by ``inv_scale``
    [d_theta].  ``log_prob_true`` [M] is the truths' log density; ``samples`` [M, num_samples,
    d_theta] and ``sample_log_probs`` [M, num_samples] are kept only on request."""

    less: Tensor
    equal: Tensor
    num_samples: int
    log_prob_true: Tensor
    references: Tensor
    inv_scale: Tensor
    samples: Optional[Tensor] = None
    sample_log_probs: Optional[Tensor] = None

    @property
    def dim_theta(self) -> int:
        return int(self.less.shape[1]) - 2

    @property
    def sbc_ranks(self) -> Tensor:
        """[M, d_theta]: simulation-based-calibration rank of each parameter, in 0..num_samples."""
        return self.less[:, : self.dim_theta]

    @property
    def hpd_ranks(self) -> Tensor:
        """[M]: the number of draws denser than the truth; ``hpd_ranks / num_samples`` is the
        smallest credibility whose highest-posterior-density region holds the truth."""
        return self.less[:, self.dim_theta]

    @property
    def tarp_ranks(self) -> Tensor:
        """[M]: the number of draws closer to the reference point than the truth (TARP)."""
        return self.less[:, self.dim_theta + 1]

    def midranks(self) -> Tensor:
        """[M, d_theta + 2] float64: ``less + equal / 2`` (ties split evenly)."""
        return self.less.to(torch.float64) + self.equal.to(torch.float64) / 2


def _rank_columns(ranks, num_samples: int, what: str) -> Tuple[Tensor, int]:
    r = torch.as_tensor(ranks)
    S = int(num_samples)
    if r.ndim not in (1, 2) or r.shape[0] < 1 or S < 1:
        raise ValueError(f"{what}: ranks must be [M] or [M, C] with M >= 1 and num_samples >= 1, got "
                         f"{tuple(r.shape)} and {S}")
    if r.is_floating_point() or int(r.min()) < 0 or int(r.max()) > S:
        raise ValueError(f"{what}: ranks must be integers in 0..{S}")
    return r.to(torch.int64), S


def rank_ks_statistic(ranks, num_samples: int) -> Tensor:
    """Distance of each column of integer ``ranks`` [M] or [M, C] from the discrete uniform
    distribution on {0..num_samples}: max over r = 0..S of |ECDF(r) - (r + 1) / (S + 1)|, float64
    [] or [C] (a statistic only, no p-value, as :func:`pit_ks_statistic`).  The ranks of a truth
    among S draws of a calibrated posterior are uniform on {0..S}."""
    r, S = _rank_columns(ranks, num_samples, "rank_ks_statistic")
    cols = r.reshape(r.shape[0], -1)
    hist = torch.zeros((S + 1, cols.shape[1]), dtype=torch.float64, device=cols.device)
    hist.scatter_add_(0, cols, torch.ones(cols.shape, dtype=torch.float64, device=cols.device))
    ecdf = torch.cumsum(hist, 0) / cols.shape[0]
    unif = torch.arange(1, S + 2, dtype=torch.float64, device=cols.device)[:, None] / (S + 1)
    ks = (ecdf - unif).abs().max(dim=0).values
    return ks[0] if r.ndim == 1 else ks


def expected_coverage(ranks, num_samples: int, levels=None) -> Tuple[Tensor, Tensor]:
    """``(levels [L], ecp [L] or [L, C])`` with ecp(c) = mean over m of 1{ranks_m / num_samples <
    c}, float64; ``levels`` defaults to ``linspace(0, 1, 21)``.  For ``CoverageRanks.hpd_ranks``
    ecp(c) is the share of pairs whose truth lies inside the c-credible highest-posterior-density
    region, for ``tarp_ranks`` TARP's coverage curve; calibrated means ecp(c) ~ c."""
    r, S = _rank_columns(ranks, num_samples, "expected_coverage")
    if levels is None:
        lv = torch.linspace(0, 1, 21, dtype=torch.float64)
    else:
        lv = torch.as_tensor(levels, dtype=torch.float64).reshape(-1)
    lv = lv.to(r.device)
    frac = r.to(torch.float64) / S
    ecp = (frac[None] < lv.reshape(-1, *([1] * r.ndim))).to(torch.float64).mean(1)
    return lv, ecp


# ------------------------------------------------------------------ MMD two-sample test
MMD_SCALE = float(2 ** 28)   # npfn_mmd_sums' fixed point: q = sum_b round(k_b * 2^28)
MMD_DEFAULT_BANDWIDTHS = {"rbf": (10.0, 15.0, 20.0, 50.0), "multiscale": (0.2, 0.5, 0.9, 1.3)}


def mmd_sums_host(z, labels, kernel, bandwidths) -> Tuple[Tensor, Tensor, Tensor]:
    """``(sums [n_obs, n_label, 2] int64, total [n_obs] int64, bad [n_obs] int32)`` -- the
    definition of the engine's ``npfn_mmd_sums`` (``Engine.mmd_sums``, same arguments), in torch on
    the CPU.

    ``z`` [n_obs, N, dim] is every observation's pooled sample (both sets stacked), ``labels``
    [n_label, N] marks (non-zero) the points of group X under each labelling, ``kernel`` is "rbf" /
    "multiscale" (0 / 1), ``bandwidths`` the a_b (1..8 of them).  In fp32, every operation rounded
    on its own: d2(i, j) = sum over k ascending of t * t, t = z_i[k] - z_j[k]; k_b = exp(d2 * c_b),
    c_b = -0.5 / a_b (rbf) or s_b / (s_b + d2), s_b = a_b * a_b (multiscale).  q(i, j) = sum over b
    of round(k_b * 2^28) (fp64 product, round half to even), an integer.  Over ORDERED pairs, the
    diagonal included: sums[u, p, 0] adds q over the pairs inside group X of labelling p, sums[u,
    p, 1] over the pairs inside its complement, total[u] over all N^2 pairs.  An observation with a
    non-finite coordinate gets bad[u] = 1 and zero sums (the engine leaves them unspecified).
    Multiscale equals the engine exactly; rbf to the last bit of the two exp."""
    z = torch.as_tensor(z).detach().to(device="cpu", dtype=torch.float32)
    labels = torch.as_tensor(labels).detach().cpu()
    code, bw = check_mmd_args(z.shape, labels.shape, kernel, bandwidths)
    n_obs, N, dim = z.shape
    L = (labels != 0).to(torch.int64)
    Lc = 1 - L
    a = torch.tensor(bw, dtype=torch.float32)
    c = torch.tensor(-0.5, dtype=torch.float32) / a if code == 0 else a * a
    sums = torch.zeros((n_obs, L.shape[0], 2), dtype=torch.int64)
    total = torch.zeros(n_obs, dtype=torch.int64)
    bad = torch.zeros(n_obs, dtype=torch.int32)
    for u in range(n_obs):
        zu = z[u]
        if not bool(torch.isfinite(zu).all()):
            bad[u] = 1
            continue
        d2 = torch.zeros((N, N), dtype=torch.float32)
        for k in range(dim):   # ascending, one rounding per operation: the kernel's own chain
            t = zu[:, None, k] - zu[None, :, k]
            d2 = d2 + t * t
        q = torch.zeros((N, N), dtype=torch.int64)
        for b in range(len(bw)):
            kb = torch.exp(d2 * c[b]) if code == 0 else c[b] / (c[b] + d2)
            q += torch.round(kb.to(torch.float64) * MMD_SCALE).to(torch.int64)
        sums[u, :, 0] = ((L @ q) * L).sum(1)
        sums[u, :, 1] = ((Lc @ q) * Lc).sum(1)
        total[u] = q.sum()
    return sums, total, bad


def permutation_labels(n: int, m: int, num_permutations: int, seed: int = 0) -> Tensor:
    """Group labels of a permutation test on n + m pooled points: uint8 [num_permutations + 1, n +
    m] (CPU).  Row 0 is n ones followed by m zeros (the observed split); row p >= 1 marks the
    first n entries of the p-th ``torch.randperm(n + m)`` of a CPU ``torch.Generator`` seeded with
    ``seed``, so a seed gives the same labels on every machine.  Every row has exactly n ones."""
    n, m, P = int(n), int(m), int(num_permutations)
    if n < 1 or m < 1 or P < 0:
        raise ValueError(f"permutation_labels: need n >= 1, m >= 1 and num_permutations >= 0, got {n}, {m}, {P}")
    gen = torch.Generator().manual_seed(int(seed))
    lab = torch.zeros((P + 1, n + m), dtype=torch.uint8)
    lab[0, :n] = 1
    for p in range(1, P + 1):
        lab[p, torch.randperm(n + m, generator=gen)[:n]] = 1
    return lab


@dataclass
class TwoSampleResult:
    """Maximum mean discrepancy between two sets of draws per observation (:func:`mmd_batched`),
    float64 on the device of the draws.  ``mmd2_biased`` [M] is the reference's statistic
    mean(k(x, x')) + mean(k(y, y')) - 2 mean(k(x, y)), the kernels summed over ``bandwidths`` and
    the diagonals included; ``mmd2_unbiased`` [M] drops the diagonals (NaN for n < 2 or m < 2).
    ``null`` [M, P] is the biased statistic under each of P random relabellings of the pooled
    points and ``p_value`` [M] = (1 + #{null >= observed}) / (P + 1) (None for P = 0).  An
    observation with a non-finite draw is NaN everywhere.  ``n`` / ``m`` are the sizes of the two
    sets."""

    mmd2_biased: Tensor
    mmd2_unbiased: Tensor
    null: Tensor
    p_value: Optional[Tensor]
    n: int
    m: int
    kernel: str
    bandwidths: Tuple[float, ...]


def mmd_p_value(observed: Tensor, null: Tensor) -> Tensor:
    """(1 + #{p : null[..., p] >= observed[...]}) / (P + 1): the permutation p-value, in {1 / (P +
    1), ..., 1}; NaN where ``observed`` is NaN."""
    P = null.shape[-1]
    p = (1 + (null >= observed[..., None]).sum(-1)).to(torch.float64) / (P + 1)
    return torch.where(torch.isnan(observed), torch.full_like(p, float("nan")), p)


def _standardise(z: Tensor, a: Tensor) -> Tensor:
    """``z`` [M, N, d] by the per-observation mean and unbiased std of ``a`` [M, n, d]; a zero std
    counts as 1 (the reference's C2ST z-score)."""
    mu, sd = a.mean(1, keepdim=True), a.std(1, keepdim=True)
    return (z - mu) / torch.where(sd == 0, torch.ones_like(sd), sd)


def mmd_batched(a, b, kernel: str = "rbf", bandwidths=None, num_permutations: int = 0, seed: int = 0,
                z_score: bool = False, engine=None) -> TwoSampleResult:
    """MMD two-sample test between ``a`` [M, n, d] and ``b`` [M, m, d], observation by observation
    (2-D inputs: M = 1), with a permutation null: the reference's MMD (scripts/
    evaluate_ropefm.py:283-320) for n != m too, and a p-value to read it by.

    ``kernel`` "rbf" sums exp(-0.5 d2 / a) and "multiscale" a^2 / (a^2 + d2) over ``bandwidths``
    (default: the reference's, [10, 15, 20, 50] / [0.2, 0.5, 0.9, 1.3]; at most 8).
    ``num_permutations`` P <= 4095 relabellings (:func:`permutation_labels` with ``seed``, shared by
    all observations) give ``null`` and ``p_value``.  ``z_score=True`` standardises both sets by
    ``a``'s per-observation mean and unbiased std first (a zero std counts as 1), as the
    reference's C2ST does.  n + m <= 32768, d <= 64.

    Tensors on the GPU go through ``npfn_mmd_sums`` (``engine.mmd_sums`` when an engine is given,
    otherwise the library's engine-free entry): every kernel value is computed once, quantised
    to 2^-28 and folded into all P + 1 labellings on the device; no n x n matrix is stored.  CPU
    tensors go through :func:`mmd_sums_host`, the same statement in torch.  The statistics are
    formed in fp64 from the integer sums."""
    a, b = torch.as_tensor(a).detach(), torch.as_tensor(b).detach()
    if kernel not in MMD_DEFAULT_BANDWIDTHS:
        raise ValueError(f"mmd_batched: kernel must be 'rbf' or 'multiscale', got {kernel!r}")
    if a.ndim == 2 and b.ndim == 2:
        a, b = a[None], b[None]
    if a.ndim != 3 or b.ndim != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or a.shape[1] < 1 \
            or b.shape[1] < 1:
        raise ValueError(f"mmd_batched: a {tuple(a.shape)} and b {tuple(b.shape)} are not [M, n >= 1, d] and "
                         "[M, m >= 1, d] (or [n, d] and [m, d])")
    P = int(num_permutations)
    if not 0 <= P <= MMD_MAX_LABELLINGS - 1:
        raise ValueError(f"mmd_batched: num_permutations must lie in 0..{MMD_MAX_LABELLINGS - 1}, got {P}")
    n, m = a.shape[1], b.shape[1]
    if z_score and n < 2:
        raise ValueError("mmd_batched: z_score needs n >= 2 draws in a (the unbiased std)")
    bw = MMD_DEFAULT_BANDWIDTHS[kernel] if bandwidths is None else bandwidths
    dev = a.device
    a, b = a.to(torch.float32), b.to(device=dev, dtype=torch.float32)
    z = torch.cat([a, b], 1)
    _, bw = check_mmd_args(z.shape, (P + 1, n + m), kernel, bw)
    if z_score:
        z = _standardise(z, a)
    labels = permutation_labels(n, m, P, seed)
    if dev.type == "cuda":
        from .engine import mmd_sums

        sums, total, bad = engine.mmd_sums(z, labels, kernel, bw) if engine is not None else \
            mmd_sums(z, labels, kernel, bw)
    else:
        sums, total, bad = mmd_sums_host(z, labels, kernel, bw)
    sums, total, bad = sums.to(dev), total.to(dev), bad.to(dev)

    B = len(bw)
    diag = B * 2 ** 28   # q(i, i) exactly
    f64 = lambda t: t.to(torch.float64)  # noqa: E731
    XX, YY = f64(sums[:, :, 0]) / MMD_SCALE, f64(sums[:, :, 1]) / MMD_SCALE
    XY = f64(total[:, None] - sums[:, :, 0] - sums[:, :, 1]) / (2 * MMD_SCALE)
    stat = XX / (n * n) + YY / (m * m) - 2 * XY / (n * m)
    if n >= 2 and m >= 2:
        unbiased = (f64(sums[:, 0, 0] - n * diag) / MMD_SCALE / (n * (n - 1))
                    + f64(sums[:, 0, 1] - m * diag) / MMD_SCALE / (m * (m - 1)) - 2 * XY[:, 0] / (n * m))
    else:
        unbiased = torch.full_like(stat[:, 0], float("nan"))
    nan = bad != 0
    stat = torch.where(nan[:, None], torch.full_like(stat, float("nan")), stat)
    unbiased = torch.where(nan, torch.full_like(unbiased, float("nan")), unbiased)
    biased, null = stat[:, 0].contiguous(), stat[:, 1:].contiguous()
    return TwoSampleResult(biased, unbiased, null, mmd_p_value(biased, null) if P > 0 else None, n, m, kernel,
                           tuple(bw))


# ------------------------------------------------------------------ exact 2-Wasserstein distance
W2_MAX_COST = 2 ** 41   # npfn_w2_assign's bound on an integer cost


def transport_scale(a: Tensor, b: Tensor) -> Tuple[Tensor, Tensor]:
    """``(scale [M] float64, nonfinite [M] bool)`` of ``a`` and ``b`` [M, n, d] fp32, on their
    device, without a host synchronisation.  Per observation, from its own pooled points only and
    in fp64: bound = (1 + 2^-10) * sum over k of (max_k - min_k)^2 (above every fp32 d2 of the
    observation: the chain's rounding is below d 2^-24), scale = 2^floor(log2(2^40 / bound)), an
    exact power of two, 1 for bound = 0 or a non-finite coordinate."""
    z = torch.cat([a, b], 1).to(torch.float64)
    nonfinite = ~torch.isfinite(z).all(2).all(1)
    rng = z.max(1).values - z.min(1).values
    bound = (1.0 + 2.0 ** -10) * (rng * rng).sum(1)
    ok = (bound > 0) & torch.isfinite(bound) & ~nonfinite
    _, ex = torch.frexp(2.0 ** 40 / torch.where(ok, bound, torch.ones_like(bound)))   # quotient in [2^(ex-1), 2^ex)
    e = torch.where(ok, (ex - 1).clamp(-1000, 1000), torch.zeros_like(ex))
    return torch.ldexp(torch.ones_like(bound), e), nonfinite


def transport_costs_host(a, b) -> Tuple[Tensor, Tensor, Tensor]:
    """``(cq [M, n, n] int64, scale [M] float64, bad [M] int32)`` -- the integer costs that the
    engine's ``npfn_w2_assign`` recomputes row by row, in torch on the device of ``a``.

    ``a`` and ``b`` are [M, n, d] fp32.  d2(i, j) is ``npfn_mmd_sums``' chain: in fp32, k ascending,
    t = a_i[k] - b_j[k], acc = acc + t * t, every operation rounded on its own.  ``scale`` is
    :func:`transport_scale`'s power of two, and cq(i, j) = round(d2 * scale) in fp64 (exact product,
    round half to even), so 0 <= cq <= 2^41; with n <= 2048 every potential and sum of the solver
    stays below 2^53.  An observation with a non-finite coordinate gets bad = 1, one with a cost
    above 2^41 (a d2 that overflowed fp32) bad = 2; both get zero costs."""
    a = torch.as_tensor(a).detach().to(torch.float32)
    b = torch.as_tensor(b).detach().to(device=a.device, dtype=torch.float32)
    M, n, d = check_transport_args(a.shape, b.shape)
    scale, nonfinite = transport_scale(a, b)
    d2 = torch.zeros((M, n, n), dtype=torch.float32, device=a.device)
    for k in range(d):   # ascending, one rounding per operation: the kernel's own chain
        t = a[:, :, None, k] - b[:, None, :, k]
        d2 = d2 + t * t
    p = d2.to(torch.float64) * scale[:, None, None]
    over = ~(p <= float(W2_MAX_COST)).all(2).all(1) & ~nonfinite
    drop = nonfinite | over
    cq = torch.round(torch.where(drop[:, None, None], torch.zeros_like(p), p)).to(torch.int64)
    bad = nonfinite.to(torch.int32) + 2 * over.to(torch.int32)
    return cq, scale, bad


def _assignment_solve_one(c: "np.ndarray"):
    n = c.shape[0]
    inf = np.iinfo(np.int64).max
    u, v = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    row = np.full(n, -1, dtype=np.int64)   # column -> row
    way = np.empty(n, dtype=np.int64)
    steps = 0
    for i in range(n):
        minv = np.full(n, inf, dtype=np.int64)
        used = np.zeros(n, dtype=bool)
        way[:] = -1                        # -1: the virtual column, which holds row i
        j0, i0 = -1, i
        while True:
            steps += 1
            if j0 >= 0:
                used[j0] = True
            free = ~used
            cur = c[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            masked = np.where(free, minv, inf)
            j1 = int(np.argmin(masked))    # the lowest column of the minimum
            delta = masked[j1]
            u[row[used]] += delta
            u[i] += delta
            v[used] -= delta
            minv[free] -= delta
            j0, i0 = j1, int(row[j1])
            if i0 < 0:
                break
        while j0 >= 0:
            j1 = int(way[j0])
            row[j0] = i if j1 < 0 else row[j1]
            j0 = j1
    assign = np.empty(n, dtype=np.int64)
    assign[row] = np.arange(n)
    return assign, u, v, int(c[np.arange(n), assign].sum()), steps


def assignment_solve_host(cq) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(assign [M, n] int32, duals [M, 2, n] int64, cost_sum [M] int64, steps [M] int64)`` (CPU)
    of the linear assignment problems ``cq`` [M, n, n] int64 -- the definition of the engine's
    ``npfn_w2_assign``: the shortest-augmenting-path Hungarian method from zero duals, in int64.

    Rows i = 0..n-1 are inserted in order.  For row i: minv[j] = INF, used[j] = false, and a
    virtual column holds row i.  A step marks the current column j0 used and takes its row i0; for
    every unused column j, cur = cq[i0][j] - u[i0] - v[j], and where cur < minv[j] (strictly)
    minv[j] = cur and way[j] = j0; delta is the minimum of minv over the unused columns and j1 its
    lowest column; u[row of j] += delta and v[j] -= delta over the used columns (the virtual one,
    i.e. u[i], included), minv[j] -= delta over the unused ones; j0 = j1, and the steps end when
    j0 has no row.  Then the path is flipped along way.  ``steps`` counts the steps (at most n (n +
    1) / 2), ``assign[i]`` is the column matched to row i, ``duals`` is (u, v): u_i + v_j <= cq_ij
    everywhere with equality on the assignment, so cost_sum = sum_i cq[i, assign[i]] = sum(u) +
    sum(v) certifies optimality.  Vectorised over the columns in numpy: n = 1000 takes seconds."""
    c = torch.as_tensor(cq).detach().cpu().to(torch.int64).numpy()
    if c.ndim != 3 or c.shape[1] != c.shape[2] or c.shape[1] < 1:
        raise ValueError(f"assignment_solve_host: cq {c.shape} is not [M, n >= 1, n]")
    M, n, _ = c.shape
    assign = torch.zeros((M, n), dtype=torch.int32)
    duals = torch.zeros((M, 2, n), dtype=torch.int64)
    cost_sum, steps = torch.zeros(M, dtype=torch.int64), torch.zeros(M, dtype=torch.int64)
    for m in range(M):
        asg, u, v, total, st = _assignment_solve_one(c[m])
        assign[m] = torch.from_numpy(asg).to(torch.int32)
        duals[m, 0], duals[m, 1] = torch.from_numpy(u), torch.from_numpy(v)
        cost_sum[m], steps[m] = total, st
    return assign, duals, cost_sum, steps


@dataclass
class TransportResult:
    """Exact 2-Wasserstein distance between two sets of n draws per observation
    (:func:`wasserstein_batched`), on the device of the draws.  ``wasserstein`` [M] float64 is the
    reference's number sqrt(sum_i d2(i, assignment[i]) / n) = sqrt(cost_sum / scale / n) and
    ``w2_squared`` [M] its square; ``assignment`` [M, n] int64 is the optimal matching (row i of a
    with row assignment[i] of b); ``cost_sum`` [M] int64 its total integer cost at ``scale`` [M]
    float64, a power of two; ``steps`` [M] int64 the solver's steps (-1 where another solver ran).
    An observation with a non-finite draw is NaN, its assignment -1."""

    wasserstein: Tensor
    w2_squared: Tensor
    assignment: Tensor
    cost_sum: Tensor
    scale: Tensor
    steps: Tensor
    n: int


def wasserstein_batched(a, b, z_score: bool = False, engine=None) -> TransportResult:
    """Exact 2-Wasserstein distance between ``a`` and ``b`` [M, n, d], observation by observation
    (2-D inputs: M = 1): the reference's ``sqrt(ot.emd2(uniform, uniform, ot.dist(a, b)))``
    (scripts/evaluate_ropefm.py:592-710).  Between two uniform sets of equal size optimal transport
    is a linear assignment problem; it is solved exactly on the integer costs round(d2 * scale),
    scale a power of two per observation (:func:`transport_scale`), so the only error against the
    real-valued problem is d2's fp32 rounding and 2^-41 of the largest cost.  n <= 2048, d <= 64,
    n * d <= 32768.  ``z_score=True`` standardises both sets by ``a``'s per-observation mean and
    unbiased std first (a zero std counts as 1), as in :func:`mmd_batched`.

    Tensors on the GPU go through ``npfn_w2_assign`` (``engine.w2_assign`` when an engine is given,
    otherwise the library's engine-free entry), one workgroup per observation, and equal
    :func:`assignment_solve_host` on :func:`transport_costs_host` bit for bit.  CPU tensors go
    through :func:`transport_costs_host` and ``scipy.optimize.linear_sum_assignment``: the same
    ``cost_sum``, a valid optimal assignment (not necessarily the same one), ``steps`` = -1."""
    a, b = torch.as_tensor(a).detach(), torch.as_tensor(b).detach()
    if a.ndim == 2 and b.ndim == 2:
        a, b = a[None], b[None]
    if a.ndim != 3 or b.ndim != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or a.shape[1] < 1 \
            or b.shape[1] < 1:
        raise ValueError(f"wasserstein_batched: a {tuple(a.shape)} and b {tuple(b.shape)} are not both [M, n >= 1, d] "
                         "(or [n, d])")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"wasserstein_batched: a has {a.shape[1]} points and b {b.shape[1]}: uniform transport "
                         "between sets of unequal size is not an assignment (an optimal plan splits mass), and the "
                         "reference harness always compares sets of equal size")
    M, n, _ = check_transport_args(a.shape, b.shape)
    if z_score and n < 2:
        raise ValueError("wasserstein_batched: z_score needs n >= 2 draws in a (the unbiased std)")
    dev = a.device
    a, b = a.to(torch.float32), b.to(device=dev, dtype=torch.float32)
    if z_score:
        mu, sd = a.mean(1, keepdim=True), a.std(1, keepdim=True)
        sd = torch.where(sd == 0, torch.ones_like(sd), sd)
        a, b = (a - mu) / sd, (b - mu) / sd
    if dev.type == "cuda":
        from .engine import w2_assign

        scale, _ = transport_scale(a, b)
        assign, _, cost_sum, steps, bad = engine.w2_assign(a, b, scale) if engine is not None else \
            w2_assign(a, b, scale)
        assign, cost_sum, steps, bad = assign.to(dev).to(torch.int64), cost_sum.to(dev), steps.to(dev), bad.to(dev)
        scale = scale.to(dev)
    else:
        from scipy.optimize import linear_sum_assignment

        cq, scale, bad = transport_costs_host(a, b)
        assign = torch.zeros((M, n), dtype=torch.int64)
        cost_sum = torch.zeros(M, dtype=torch.int64)
        steps = torch.full((M,), -1, dtype=torch.int64)
        for m in range(M):
            if int(bad[m]) == 0:
                c = cq[m].numpy()
                rows, cols = linear_sum_assignment(c)
                assign[m, torch.from_numpy(rows)] = torch.from_numpy(cols)
                cost_sum[m] = int(c[rows, cols].sum())
    nan = bad != 0
    w2 = cost_sum.to(torch.float64) / (scale * float(n))   # scale * n is exact: one rounding
    w2 = torch.where(nan, torch.full_like(w2, float("nan")), w2)
    assign = torch.where(nan[:, None], torch.full_like(assign, -1), assign)
    return TransportResult(torch.sqrt(w2), w2, assign, cost_sum, scale, steps, n)


# ------------------------------------------------------------------ classifier two-sample test
C2ST_MODELS = ("mlp", "mlp_small", "linear")   # the reference's _MODEL_REGISTRY


def c2st_folds(n: int, m: int, n_folds: int = 5, seed: int = 1) -> Tensor:
    """Stratified, shuffled folds of n + m pooled points: uint8 [n + m] (CPU), the fold that holds
    each point out.  With p = ``torch.randperm(n)`` and then q = ``torch.randperm(m)`` of a CPU
    ``torch.Generator`` seeded with ``seed``, point p[i] of the first set gets fold i % n_folds and
    point n + q[i] of the second fold (i + n) % n_folds, so fold sizes differ by at most one overall
    and per class, and a seed gives the same folds on every machine."""
    n, m, F = int(n), int(m), int(n_folds)
    if not 2 <= F <= C2ST_MAX_FOLDS:
        raise ValueError(f"c2st_folds: n_folds must lie in 2..{C2ST_MAX_FOLDS}, got {F}")
    if n < F or m < F:
        raise ValueError(f"c2st_folds: need at least n_folds = {F} points in each set, got {n} and {m}")
    gen = torch.Generator().manual_seed(int(seed))
    p, q = torch.randperm(n, generator=gen), torch.randperm(m, generator=gen)
    fold = torch.empty(n + m, dtype=torch.uint8)
    fold[p] = (torch.arange(n) % F).to(torch.uint8)
    fold[n + q] = ((torch.arange(m) + n) % F).to(torch.uint8)
    return fold


def c2st_order(n_pool: int, epochs: int, seed: int) -> Tensor:
    """Visiting order of the pooled points per epoch: int32 [epochs, n_pool] (CPU), row e the e-th
    ``torch.randperm(n_pool)`` of a CPU ``torch.Generator`` seeded with ``seed``.  Fold f visits
    epoch e's row in that order and skips its own held-out points; batches are consecutive runs of
    ``batch_size`` of what is left, a short last batch kept (as the reference's DataLoader does)."""
    n_pool, epochs = int(n_pool), int(epochs)
    if n_pool < 1 or epochs < 1:
        raise ValueError(f"c2st_order: need n_pool >= 1 and epochs >= 1, got {n_pool} and {epochs}")
    gen = torch.Generator().manual_seed(int(seed))
    return torch.stack([torch.randperm(n_pool, generator=gen) for _ in range(epochs)]).to(torch.int32)


def c2st_widths(model: str, d: int) -> list:
    """Layer widths of the reference's classifiers on d inputs: "mlp" [d, 4d, 8d, 8d, 4d, 2]
    (DefaultMLP), "mlp_small" [d, 4d, 4d, 2], "linear" [d, 2]."""
    d = int(d)
    if model == "mlp":
        return [d, 4 * d, 8 * d, 8 * d, 4 * d, 2]
    if model == "mlp_small":
        return [d, 4 * d, 4 * d, 2]
    if model == "linear":
        return [d, 2]
    raise ValueError(f"c2st_widths: model must be one of {C2ST_MODELS}, got {model!r}")


def c2st_init(widths, seed: int) -> Tensor:
    """Starting parameters of the MLP with these ``widths``: float32 [P] (CPU), layer by layer W
    [out, in] row-major then b [out], each uniform in +-1 / sqrt(in) (``torch.nn.Linear``'s default)
    from a CPU ``torch.Generator`` seeded with ``seed``.  The same vector starts every fold of every
    observation."""
    gen = torch.Generator().manual_seed(int(seed))
    parts = []
    for fan_in, out in zip(widths[:-1], widths[1:]):
        bound = 1.0 / math.sqrt(int(fan_in))
        for shape in ((int(out), int(fan_in)), (int(out),)):
            parts.append(((torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound).reshape(-1))
    return torch.cat(parts).to(torch.float32)


def c2st_adam_table(lr: float, n_steps: int, dtype=torch.float32) -> Tensor:
    """Adam's per-step factors, float32 [n_steps, 2] (CPU): row t (step t + 1) is (lr / (1 -
    beta1^(t+1)), 1 / sqrt(1 - beta2^(t+1))) with torch's default betas, computed in fp64 and
    rounded once.  The engine and ``c2st_fit_host`` at float32 read the same table;
    ``c2st_fit_host`` at float64 asks for it unrounded (``dtype=torch.float64``), since the
    rounding of the step size alone moves a loss by 1e-9 within a few dozen steps."""
    t = torch.arange(1, int(n_steps) + 1, dtype=torch.float64)
    b1, b2 = C2ST_BETAS
    return torch.stack([float(lr) / (1.0 - b1 ** t), 1.0 / torch.sqrt(1.0 - b2 ** t)], 1).to(dtype)


def c2st_fit_host(z, n_first, fold, order, widths, init, epochs, batch_size=128, lr=1e-3, weight_decay=0.0,
                  dtype=torch.float32) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(correct [M, F] int32, loss [M, F, E], prob [M, N], bad [M] int32)`` (CPU) -- the
    definition of the engine's ``npfn_c2st_fit`` (``engine.c2st_fit``, same arguments), in plain
    torch matmuls at ``dtype`` (float32 or float64).

    ``z`` [M, N, d] is every observation's pooled sample; points 0..n_first-1 have label 0, the
    rest label 1.  Per observation and fold f (``fold`` [N]) the MLP of ``widths`` starts at
    ``init`` and is trained for ``epochs`` passes: epoch e visits row e of ``order`` [E, N] without
    the points of fold f, in batches of ``batch_size`` (a short last batch kept).  Per batch of B
    rows: logits (l0, l1) from Linear / ReLU layers, d = l1 - l0, row loss max(s, 0) + log1p(exp(-
    |s|)) with s = d for label 0 and -d for label 1 (cross-entropy), batch loss their mean; the
    gradient is back-propagated from (sigmoid(d) - label) / B; Adam as ``torch.optim.Adam`` (betas
    0.9 / 0.999, eps 1e-8, no amsgrad, ``weight_decay`` added to the gradient), 1 - beta formed at
    ``dtype``, the step's bias corrections from :func:`c2st_adam_table` at ``dtype``.  loss[., f, e] = (sum over
    the batches of batch loss * B) / n_train, the reference's epoch_loss / len(train_ds).  After
    the last epoch every point of fold f gets prob = sigmoid(d) under this network and counts as
    correct when its prediction (1 exactly when l1 > l0; a tie is 0, as argmax) is its label.
    bad = 1 for a non-finite coordinate (zero outputs), 2 when an epoch loss is not finite."""
    z = torch.as_tensor(z).detach().to(device="cpu", dtype=dtype)
    fold = torch.as_tensor(fold).detach().cpu().to(torch.int64)
    order = torch.as_tensor(order).detach().cpu().to(torch.int64)
    init = torch.as_tensor(init).detach().to(device="cpu", dtype=dtype)
    F = int(fold.max()) + 1
    E, bs = int(epochs), int(batch_size)
    M, N, d, P = check_c2st_args(z.shape, n_first, widths, F, E, bs)
    if tuple(fold.shape) != (N,) or tuple(order.shape) != (E, N) or tuple(init.shape) != (P,):
        raise ValueError(f"c2st_fit_host: fold {tuple(fold.shape)}, order {tuple(order.shape)} and init "
                         f"{tuple(init.shape)} are not [{N}], [{E}, {N}] and [{P}]")
    widths = [int(w) for w in widths]
    L = len(widths) - 1
    label = (torch.arange(N) >= int(n_first)).to(dtype)
    finite = torch.isfinite(z).all(2).all(1)
    zz = torch.where(finite[:, None, None], z, torch.zeros_like(z))
    b1, b2 = torch.tensor(C2ST_BETAS[0], dtype=dtype), torch.tensor(C2ST_BETAS[1], dtype=dtype)
    omb1, omb2 = 1 - b1, 1 - b2
    eps, wd = torch.tensor(C2ST_EPS, dtype=dtype), torch.tensor(float(weight_decay), dtype=dtype)
    n_train = [N - int((fold == f).sum()) for f in range(F)]
    table = c2st_adam_table(lr, E * ((max(n_train) + bs - 1) // bs), dtype=dtype)

    correct = torch.zeros((M, F), dtype=torch.int32)
    loss = torch.zeros((M, F, E), dtype=dtype)
    prob = torch.zeros((M, N), dtype=dtype)

    def forward(params, x):
        hs = [x]
        for l, (W, b) in enumerate(params):
            h = hs[-1] @ W.transpose(1, 2) + b[:, None, :]
            hs.append(torch.relu(h) if l + 1 < L else h)
        return hs

    for f in range(F):
        params, off = [], 0
        for i, o in zip(widths[:-1], widths[1:]):
            W = init[off:off + o * i].view(1, o, i).repeat(M, 1, 1)
            b = init[off + o * i:off + o * i + o].view(1, o).repeat(M, 1)
            params.append([W, b])
            off += o * i + o
        state = [[torch.zeros_like(t) for t in (W, b, W, b)] for W, b in params]   # mW, mb, vW, vb
        step = 0
        for e in range(E):
            row = order[e]
            row = row[fold[row] != f]
            eloss = torch.zeros(M, dtype=dtype)
            for b0 in range(0, n_train[f], bs):
                idx = row[b0:b0 + bs]
                B = idx.numel()
                y = label[idx]
                hs = forward(params, zz[:, idx])
                dl = hs[-1][:, :, 1] - hs[-1][:, :, 0]
                s = torch.where(y > 0, -dl, dl)
                row_loss = s.clamp(min=0) + torch.log1p(torch.exp(-s.abs()))
                eloss = eloss + row_loss.sum(1) / B * B
                d1 = (torch.sigmoid(dl) - y) / B
                delta = torch.stack([-d1, d1], 2)
                lr_t, c2 = table[step, 0], table[step, 1]
                grads = []
                for l in range(L - 1, -1, -1):
                    W, b = params[l]
                    grads.append((delta.transpose(1, 2) @ hs[l], delta.sum(1)))
                    if l > 0:
                        delta = (delta @ W) * (hs[l] > 0).to(dtype)
                grads.reverse()
                for l in range(L):
                    for j in range(2):
                        w, g = params[l][j], grads[l][j] + wd * params[l][j]
                        mom = b1 * state[l][j] + omb1 * g
                        var = b2 * state[l][2 + j] + omb2 * g * g
                        state[l][j], state[l][2 + j] = mom, var
                        params[l][j] = w - lr_t * (mom / (var.sqrt() * c2 + eps))
                step += 1
            loss[:, f, e] = eloss / n_train[f]
        held = torch.nonzero(fold == f).reshape(-1)
        logits = forward(params, zz[:, held])[-1]
        dl = logits[:, :, 1] - logits[:, :, 0]
        prob[:, held] = torch.sigmoid(dl)
        correct[:, f] = ((logits[:, :, 1] > logits[:, :, 0]) == (label[held] > 0)).sum(1).to(torch.int32)
    bad = (~finite).to(torch.int32)
    bad = torch.where(finite & ~torch.isfinite(loss).all(2).all(1), torch.full_like(bad, 2), bad)
    nf = ~finite
    correct[nf], loss[nf], prob[nf] = 0, 0, 0
    return correct, loss, prob, bad


@dataclass
class ClassifierTestResult:
    """Classifier two-sample test per observation (:func:`c2st_batched`), on the device of the
    draws.  ``c2st`` [M] float64 is the reference's number: the mean over folds of each fold's
    held-out accuracy (not the pooled accuracy); 0.5 = the classifier cannot tell the sets apart.
    ``fold_accuracy`` [M, F] float64 and ``train_loss`` [M, F, E] float32 (the mean training loss of
    each epoch) are per fold; ``probs`` [M, n + m] (None unless asked for) is each point's
    probability of belonging to the second set under the classifier that held it out; ``fold`` [n +
    m] uint8 (CPU) the fold of every pooled point.  An observation with a non-finite draw, or whose
    training loss stopped being finite, is NaN throughout."""

    c2st: Tensor
    fold_accuracy: Tensor
    train_loss: Tensor
    probs: Optional[Tensor]
    fold: Tensor
    n: int
    m: int
    model: str
    seed: int


def c2st_batched(a, b, seed: int = 1, n_folds: int = 5, model: str = "mlp", z_score: bool = True, epochs: int = 100,
                 batch_size: int = 128, lr: float = 1e-3, weight_decay: float = 0.0, return_probs: bool = False,
                 engine=None) -> ClassifierTestResult:
    """Classifier two-sample test between ``a`` [M, n, d] and ``b`` [M, m, d], observation by
    observation (2-D inputs: M = 1; n != m allowed): the reference's
    ``classifier_two_samples_test_torch`` (scripts/evaluate_ropefm.py:119-280) with its defaults.

    Both sets are z-scored by ``a``'s per-observation mean and unbiased std (``z_score``; a zero
    std counts as 1), pooled with labels 0 / 1, and split into ``n_folds`` stratified shuffled folds
    (:func:`c2st_folds`, shared by all observations).  Per fold a fresh ``model`` ("mlp": d -> 4d ->
    8d -> 8d -> 4d -> 2 with ReLUs, "mlp_small": d -> 4d -> 4d -> 2, "linear": d -> 2), started from
    :func:`c2st_init`, is trained with Adam (``lr``, ``weight_decay``) for ``epochs`` passes in
    batches of ``batch_size`` (:func:`c2st_order`) on cross-entropy and scored on the held-out fold;
    ``c2st`` is the mean held-out accuracy over the folds.  ``seed`` fixes folds, order and init
    through CPU generators, so a seed gives the same inputs on every machine.

    Tensors on the GPU go through ``npfn_c2st_fit`` (``engine.c2st_fit`` when an engine is given,
    otherwise the library's engine-free entry): one workgroup per (observation, fold) trains and
    scores its classifier in a single launch.  It holds at most 16384 parameters in layers of at
    most 128 units: "mlp" reaches d = 11, "mlp_small" d = 28, "linear" d = 64 (ValueError past
    that); n + m <= 32768.  CPU tensors go through :func:`c2st_fit_host` in float32, the same
    statement in torch.  Not offered: the reference's ``noise_scale``, ``cv="KFold"``, callable
    models and scorings other than accuracy."""
    a, b = torch.as_tensor(a).detach(), torch.as_tensor(b).detach()
    if model not in C2ST_MODELS:
        raise ValueError(f"c2st_batched: model must be one of {C2ST_MODELS}, got {model!r}")
    if a.ndim == 2 and b.ndim == 2:
        a, b = a[None], b[None]
    if a.ndim != 3 or b.ndim != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise ValueError(f"c2st_batched: a {tuple(a.shape)} and b {tuple(b.shape)} are not [M, n, d] and [M, m, d] "
                         "(or [n, d] and [m, d])")
    M, n, d = a.shape
    m = b.shape[1]
    if z_score and n < 2:
        raise ValueError("c2st_batched: z_score needs n >= 2 draws in a (the unbiased std)")
    F, E = int(n_folds), int(epochs)
    fold = c2st_folds(n, m, F, seed)
    widths = c2st_widths(model, d)
    dev = a.device
    a, b = a.to(torch.float32), b.to(device=dev, dtype=torch.float32)
    z = torch.cat([a, b], 1)
    check_c2st_args(z.shape, n, widths, F, E, batch_size)
    if z_score:
        z = _standardise(z, a)
    order = c2st_order(n + m, E, seed)
    init = c2st_init(widths, seed)
    if dev.type == "cuda":
        from .engine import c2st_fit

        fit = engine.c2st_fit if engine is not None else c2st_fit
        correct, loss, prob, _, bad = fit(z, n, fold, order, widths, init, E, batch_size, lr, weight_decay,
                                          return_probs=return_probs)
    else:
        correct, loss, prob, bad = c2st_fit_host(z, n, fold, order, widths, init, E, batch_size, lr, weight_decay,
                                                 dtype=torch.float32)
        prob = prob if return_probs else None
    correct, loss, bad = correct.to(dev), loss.to(dev), bad.to(dev)
    held = torch.bincount(fold.to(torch.int64), minlength=F).to(device=dev, dtype=torch.float64)
    acc = correct.to(torch.float64) / held[None, :]
    nan = bad != 0
    acc = torch.where(nan[:, None], torch.full_like(acc, float("nan")), acc)
    loss = torch.where(nan[:, None, None], torch.full_like(loss, float("nan")), loss)
    if prob is not None:
        prob = prob.to(dev)
        prob = torch.where(nan[:, None], torch.full_like(prob, float("nan")), prob)
    return ClassifierTestResult(acc.mean(1), acc, loss, prob, fold, n, m, model, int(seed))
