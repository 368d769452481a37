"""Calibration diagnostics of the autoregressive posterior, in torch (no scipy).

``bar_cdf`` is the host restatement (fp64) of the engine's ``npfn_bar_cdf`` (include/npfn.h): the
CDF of tabpfn's full-support bar distribution, the integral of exactly the density whose negative
log ``criterion(logits, y)`` returns.  ``NPE_PFN_Core.pit_batched`` uses it with every estimator
that has no fused ``ar_score`` (e.g. the CPU oracle).  ``pit_ks_statistic`` condenses the
per-dimension probability integral transform values ``u_k = F_k(theta_k | x, theta_<k)`` -- uniform
exactly when conditional k is calibrated -- into one Kolmogorov-Smirnov distance per dimension.
"""

from __future__ import annotations

import math

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
