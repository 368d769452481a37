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
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

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
