"""References shared by the pair-marginals tests (host and GPU).

``cell_mass_ref`` restates npfn_bar_cell_mass in fp64 torch on the same fp32 masses: cumulative
sums by ``torch.cumsum``, the NLL's bucket rule and bar_cdf's fraction rules, F always from the
left.  ``pair_index`` is the pair axis' layout.
"""
import math

import torch

HALFNORMAL_MEDIAN = 0.6744897501960817


def pair_index(j, k):
    assert j < k
    return k * (k - 1) // 2 + j


def cell_mass_ref(p, borders, edges):
    """p [R, nb] unnormalised fp32 masses, borders [nb + 1], edges [G + 1] (fp32 values) ->
    [R, G] float64 on p's device; NaN rows where the total is not positive and finite."""
    p64 = p.to(torch.float64)
    dev = p64.device
    b = borders.to(device=dev, dtype=torch.float64).contiguous()
    e = edges.to(device=dev, dtype=torch.float64).contiguous()
    nb = p64.shape[1]
    cum = torch.cumsum(p64, 1)
    tot = cum[:, -1]
    L = torch.cat([torch.zeros_like(cum[:, :1]), cum[:, :-1]], 1)
    idx = torch.searchsorted(b, e, right=False) - 1
    idx = torch.where(e == b[0], torch.zeros_like(idx), idx)
    idx = torch.where(e == b[-1], torch.full_like(idx, nb - 1), idx)
    idx = idx.clamp(0, nb - 1)
    left, right = b[idx], b[idx + 1]
    wd = right - left
    pos = wd > 0
    wd_safe = torch.where(pos, wd, torch.ones_like(wd))
    scale = wd_safe / HALFNORMAL_MEDIAN * math.sqrt(2.0)
    frac = ((e - left) / wd_safe).clamp(0.0, 1.0)
    frac_l = torch.erfc((right - e).clamp(min=0.0) / scale)
    frac_r = torch.erf((e - left).clamp(min=0.0) / scale)
    frac = torch.where(idx == 0, frac_l, torch.where(idx == nb - 1, frac_r, frac))
    frac = torch.where(pos, frac, torch.ones_like(frac))
    F = (L[:, idx] + p64[:, idx] * frac[None, :]) / tot[:, None]
    w = (F[:, 1:] - F[:, :-1]).clamp(min=0.0)
    ok = (tot > 0) & torch.isfinite(tot)
    return torch.where(ok[:, None], w, torch.full_like(w, float("nan")))
