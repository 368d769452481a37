"""Posterior marginals averaged over the sampler's own conditionals.

Every autoregressive sampler step forms, for draw i, the full predictive distribution of theta_k
given x and the draw's own theta_<k -- the ensemble mixture over the bars -- and draws one number
from it.  The mean of those row mixtures over the draws estimates the marginal q(theta_k | x)
(the "Rao-Blackwellised" marginal): the same draws as a histogram of the samples, with the
variance inside each conditional integrated out instead of sampled.  All rows of a step share
the step's bar borders, so the mean is a plain per-bar average and the result is again a bar
distribution, summarised by the same routines as any predictive distribution
(npfn_bar_stats / npfn_bar_cdf / npfn_bar_nll on the device; their fp64 restatement below for
tensors on the CPU).

``NPE_PFN_Core.marginals`` builds a :class:`PosteriorMarginals`; with the engine-backed
regressor the average is formed on the device by npfn_ar_marginals (include/npfn.h).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from .diagnostics import HALFNORMAL_MEDIAN, bar_cdf

SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


# --------------------------------------------------------------- host summaries (fp64, torch)
def _norm64(p: Tensor) -> Tensor:
    p = p.to(torch.float64)
    return p / p.sum(-1, keepdim=True)


def host_bar_mean(p: Tensor, borders: Tensor) -> Tensor:
    """Mean per row of masses ``p`` [R, nb]: bar centres, half-normal means in the two tail bars."""
    b = borders.to(torch.float64)
    w = b[1:] - b[:-1]
    m = b[:-1] + w / 2
    m[0] = b[1] - (w[0] / HALFNORMAL_MEDIAN) * SQRT_2_OVER_PI
    m[-1] = b[-2] + (w[-1] / HALFNORMAL_MEDIAN) * SQRT_2_OVER_PI
    return _norm64(p) @ m


def host_bar_mode(p: Tensor, borders: Tensor) -> Tensor:
    """Centre of the densest bar per row (bars of width 0 are never the mode)."""
    b = borders.to(torch.float64)
    w = b[1:] - b[:-1]
    dens = torch.where(w > 0, _norm64(p) / torch.where(w > 0, w, torch.ones_like(w)),
                       torch.full_like(w, float("-inf")))
    j = dens.argmax(-1)
    return b[j] + w[j] / 2


def host_bar_quantile(p: Tensor, borders: Tensor, q: float) -> Tensor:
    """icdf(q) per row: the first bar WITH MASS whose cumulative sum reaches q (the last bar with
    mass if none does), linear inside it -- never a point inside a zero-mass bar."""
    p = _norm64(p)
    b = borders.to(torch.float64)
    cdf = torch.cumsum(p, -1)
    cdf0 = cdf - p
    mass = p > 0
    ok = mass & (cdf >= q)
    first = ok.to(torch.int8).argmax(-1)
    nb = p.shape[-1]
    last_mass = nb - 1 - mass.flip(-1).to(torch.int8).argmax(-1)
    j = torch.where(ok.any(-1), first, last_mass)
    pj = p.gather(-1, j[:, None])[:, 0]
    frac = ((q - cdf0.gather(-1, j[:, None])[:, 0]) / pj).clamp(0.0, 1.0)
    out = b[j] + (b[j + 1] - b[j]) * frac
    return torch.where(mass.any(-1), out, torch.full_like(out, float("nan")))


def host_bar_logpdf(p: Tensor, borders: Tensor, y: Tensor) -> Tensor:
    """Log density at y_i under row i: log(p_j / w_j) in an inner bar, the half-normal tails of the
    full-support bar distribution in the two end bars (the negative of ``criterion(logits, y)``)."""
    p = _norm64(p)
    b = borders.to(torch.float64)
    y = y.to(torch.float64).reshape(-1)
    nb = p.shape[-1]
    w = b[1:] - b[:-1]
    idx = torch.searchsorted(b, y.contiguous(), right=False) - 1
    idx = torch.where(y == b[0], torch.zeros_like(idx), idx)
    idx = torch.where(y == b[-1], torch.full_like(idx, nb - 1), idx)
    idx = idx.clamp(0, nb - 1)
    lp = torch.log(p.gather(-1, idx[:, None])[:, 0]) - torch.log(w[idx])

    def hn_logpdf(v, s):
        return torch.log(SQRT_2_OVER_PI / s) - v * v / (2.0 * s * s)

    s0, s1 = w[0] / HALFNORMAL_MEDIAN, w[-1] / HALFNORMAL_MEDIAN
    lp = torch.where(idx == 0, lp + hn_logpdf((b[1] - y).clamp(min=1e-8), s0) + torch.log(w[0]), lp)
    lp = torch.where(idx == nb - 1, lp + hn_logpdf((y - b[-2]).clamp(min=1e-8), s1) + torch.log(w[-1]), lp)
    return lp


class PosteriorMarginals:
    """Per-parameter posterior marginals of ``M`` observations as bar distributions.

    * ``probs`` [M, d_theta, n_bars]: ``probs[m, k]`` are the bar masses of q(theta_k | x_m), the
      mean over the draws of observation m of the conditionals they were drawn from;
    * ``borders`` [d_theta, n_bars + 1]: the bar borders of dimension k (shared by all observations);
    * ``num_draws``: draws per observation behind the average;
    * ``support_fraction`` [M] float64: the share of those draws inside the prior's support (NaN
      without a prior);
    * ``samples`` [M, num_draws, d_theta] when asked for, else None.

    These are the marginals of the estimator BEFORE truncation to the prior's support: the draws
    averaged over are the sampler's proposals, not the ones ``sample`` keeps after its rejection
    step.  ``support_fraction`` says how much of the estimator's mass that rejection would remove
    (1 - support_fraction is the leakage); no reweighting is applied.

    Every summary is one call per dimension into the bar routines on ``log(probs[:, k])`` and
    ``borders[k]``: the engine's (npfn_bar_stats / npfn_bar_cdf / npfn_bar_nll) for device tensors
    built by the engine-backed regressor, their fp64 restatement for tensors on the CPU.  A bar
    without mass is never returned as a quantile or a median.
    """

    def __init__(self, probs: Tensor, borders: Tensor, num_draws: int, support_fraction: Optional[Tensor] = None,
                 engine=None, samples: Optional[Tensor] = None):
        probs = torch.as_tensor(probs)
        borders = torch.as_tensor(borders)
        if probs.ndim != 3 or borders.shape != (probs.shape[1], probs.shape[2] + 1) or probs.shape[2] < 2:
            raise ValueError(f"PosteriorMarginals: probs {tuple(probs.shape)} must be [M, d_theta, n_bars >= 2] and "
                             f"borders {tuple(borders.shape)} [d_theta, n_bars + 1]")
        self.probs = probs
        self.borders = borders.to(probs.device)
        self.num_draws = int(num_draws)
        if support_fraction is None:
            support_fraction = torch.full((probs.shape[0],), float("nan"), dtype=torch.float64, device=probs.device)
        self.support_fraction = support_fraction
        self.samples = samples
        self._engine = engine if (engine is not None and probs.is_cuda) else None

    # ------------------------------------------------------------------ shapes
    @property
    def num_observations(self) -> int:
        return self.probs.shape[0]

    @property
    def dim_theta(self) -> int:
        return self.probs.shape[1]

    @property
    def num_bars(self) -> int:
        return self.probs.shape[2]

    def _logits(self, k: int) -> Tensor:
        return torch.log(self.probs[:, k]).contiguous()   # a bar without mass: -inf

    def _stats(self, k: int, quantiles=(), mean: bool = False, mode: bool = False) -> dict:
        """{"mean": [M], "mode": [M], "quantiles": [len(q), M]} of dimension k (keys as asked for)."""
        if self._engine is not None:
            return self._engine.bar_stats(self._logits(k), self.borders[k], quantiles, mean=mean, mode=mode)
        p, b = self.probs[:, k], self.borders[k]
        out = {}
        if mean:
            out["mean"] = host_bar_mean(p, b)
        if mode:
            out["mode"] = host_bar_mode(p, b)
        if len(quantiles):
            out["quantiles"] = torch.stack([host_bar_quantile(p, b, float(q)) for q in quantiles], 0)
        return out

    def _per_dim(self, fn) -> Tensor:
        return torch.stack([fn(k) for k in range(self.dim_theta)], -1)

    # --------------------------------------------------------------- summaries
    def mean(self) -> Tensor:
        """Posterior mean of every parameter, [M, d_theta] (half-normal tail bars)."""
        return self._per_dim(lambda k: self._stats(k, mean=True)["mean"])

    def mode(self) -> Tensor:
        """Centre of the densest bar of every marginal, [M, d_theta]."""
        return self._per_dim(lambda k: self._stats(k, mode=True)["mode"])

    def quantile(self, q) -> Tensor:
        """Marginal quantiles: [M, d_theta] for a float level, [len(q), M, d_theta] for a 1-D list of
        at most 64 levels in [0, 1] (ValueError otherwise)."""
        from .engine import check_quantiles

        lv = torch.as_tensor(q, dtype=torch.float64)
        if lv.ndim > 1:
            raise ValueError(f"quantile: q must be a float or a 1-D list, got shape {tuple(lv.shape)}")
        levels = check_quantiles(lv.reshape(-1).tolist())
        if not levels:
            raise ValueError("quantile: no level given")
        out = self._per_dim(lambda k: self._stats(k, levels)["quantiles"])   # [len(q), M, d_theta]
        return out[0] if lv.ndim == 0 else out

    def median(self) -> Tensor:
        return self.quantile(0.5)

    def interval(self, level: float = 0.9) -> Tensor:
        """Equal-tailed credible interval of every marginal: [M, d_theta, 2] = the quantiles
        (1 - level) / 2 and (1 + level) / 2."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError(f"interval: level must lie in (0, 1), got {level!r}")
        q = self.quantile([(1.0 - level) / 2, (1.0 + level) / 2])
        return torch.stack([q[0], q[1]], -1)

    def _points(self, theta) -> Tensor:
        """theta as [M, K, d_theta] (K points per observation) and the shape to give back."""
        th = torch.as_tensor(theta).to(self.probs.device)
        M, d = self.num_observations, self.dim_theta
        if th.shape[-1:] != (d,) or th.ndim not in (1, 2, 3) or (th.ndim >= 2 and th.shape[0] != M):
            raise ValueError(f"theta {tuple(th.shape)} must be [d_theta], [M, d_theta] or [M, K, d_theta] with "
                             f"M = {M}, d_theta = {d}")
        shape = th.shape
        if th.ndim == 1:
            th = th.expand(M, d)
        return th.reshape(M, -1, d), shape

    def _pointwise(self, theta, dev_fn, host_fn) -> Tensor:
        th, shape = self._points(theta)
        M, K, _ = th.shape
        cols = []
        for k in range(self.dim_theta):
            y = th[:, :, k].reshape(-1)
            if self._engine is not None:
                cols.append(dev_fn(self._logits(k).repeat_interleave(K, 0), self.borders[k], y))
            else:
                cols.append(host_fn(self.probs[:, k].repeat_interleave(K, 0), self.borders[k], y))
        out = torch.stack(cols, -1).reshape(M, K, -1)
        return out if len(shape) == 3 else out[:, 0]

    def cdf(self, theta) -> Tensor:
        """Marginal CDFs F_k(theta_k | x_m) per dimension: [M, d_theta] for ``theta`` [M, d_theta]
        or [d_theta] (the same point for every observation), [M, K, d_theta] for K points per
        observation."""
        return self._pointwise(theta, lambda lg, b, y: self._engine.bar_cdf(lg, b, y),
                               lambda p, b, y: bar_cdf(torch.log(_norm64(p)), b, y))

    def log_prob(self, theta) -> Tensor:
        """Per-dimension marginal log densities log q(theta_k | x_m), shaped like :meth:`cdf`'s
        result (NOT the joint log density: the marginals carry no dependence between parameters)."""
        return self._pointwise(theta, lambda lg, b, y: -self._engine.bar_nll(lg, b, y), host_bar_logpdf)
