"""2-D posterior marginals folded from the sampler's own conditionals (the corner / pair plot).

At autoregressive step k the sampler forms, for every draw i, the full predictive distribution
p_i(theta_k | x, theta_<k^i) and keeps one number from it.  ``marginals`` averages those row
mixtures into 1-D marginals; the same mixtures give the 2-D marginal of every pair (j, k), j < k,
on a coarse grid of G x G cells:

    pair[u][(j, k)][a][c] = (1 / per) * sum over the rows i of observation u of
                            1{theta_j^i in cell a of dim j} * P_i(theta_k in cell c | x_u, theta_<k^i)

-- "half Rao-Blackwellised": the earlier coordinate is a draw indicator, the later one a cell mass
of the row's conditional, integrated instead of sampled.  Its variance is below a 2-D histogram's
of the same draws and it costs no forward pass beyond the sampler's own.

``NPE_PFN_Core.pair_marginals`` builds a :class:`PosteriorPairMarginals`; with the engine-backed
regressor the tables are folded on the device by npfn_ar_pair_marginals (include/npfn.h), whose
accumulation :func:`pair_accumulate_host` restates in torch.  Every method below is plain torch on
the tensors' device.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

MIN_BINS, MAX_BINS = 2, 128   # n_cells of npfn_ar_pair_marginals
PAIR_SCALE = float(2 ** 40)   # q = round(w * 2^40)
MAX_PER = 2 ** 22             # rows per observation and call: 2^22 * 2^40 < 2^63


def grid_edges(limits, bins: int) -> Tensor:
    """Cell edges [d, bins + 1] (float32) of ``limits`` [d, 2]: ``lo + (hi - lo) * c / bins`` in
    fp64, rounded to fp32, the last edge exactly ``hi``.  ValueError for ``bins`` outside 2..128, a
    non-finite limit, ``hi <= lo``, or limits so close that the fp32 edges do not increase."""
    bins = int(bins)
    if not MIN_BINS <= bins <= MAX_BINS:
        raise ValueError(f"pair_marginals: bins must lie in {MIN_BINS}..{MAX_BINS}, got {bins}")
    lim = torch.as_tensor(limits).detach().to(torch.float64)
    if lim.ndim != 2 or lim.shape[1] != 2 or lim.shape[0] < 1:
        raise ValueError(f"pair_marginals: limits must be [d_theta, 2], got {tuple(lim.shape)}")
    if not bool(torch.isfinite(lim).all()):
        raise ValueError("pair_marginals: limits must be finite")
    lo, hi = lim[:, :1], lim[:, 1:]
    c = torch.arange(bins + 1, dtype=torch.float64, device=lim.device)[None, :]
    edges = (lo + (hi - lo) * c / bins).to(torch.float32)
    edges[:, -1] = hi[:, 0].to(torch.float32)
    if not bool((edges[:, 1:] > edges[:, :-1]).all()):
        raise ValueError("pair_marginals: degenerate limits (need low < high, far enough apart for "
                         f"{bins} float32 cells)")
    return edges


def pair_index(j: int, k: int) -> int:
    """Index of pair (j, k), j < k, along the pair axis: k (k - 1) / 2 + j."""
    return k * (k - 1) // 2 + j


def pair_accumulate_host(w, theta, edges, r0: int, per: int, pairQ: Tensor, cellQ: Tensor, bad: Tensor) -> None:
    """Adds one window of cell masses to the integer tables (in place; the caller zeroes them before
    the first window) -- the definition of the engine's ``npfn_pair_accumulate``
    (``Engine.pair_accumulate``, same arguments), in torch on the device of ``pairQ``.

    ``w`` [n, G] float64; window row r is row ``r0 + r`` of the call and belongs to observation
    ``u = (r0 + r) // per``.  ``q = round(w * 2^40)`` (``torch.round``: half to even) as int64;
    ``cellQ`` [U, G] gets ``q`` of every row; for each earlier dimension j < n_prev (``edges``
    [n_prev, G + 1], ``theta`` [n, >= n_prev]) whose draw has a cell a (``edges[j][a] <= theta_j <
    edges[j][a + 1]``; below the first edge, at or above the last, or NaN: none), ``pairQ`` [U,
    n_prev, G, G] gets ``q`` at ``[u, j, a, :]``.  A row with a NaN in ``w`` sets ``bad[u] = 1``
    (int32 [U]) and adds nothing.  ``theta`` and ``edges`` may be None (n_prev = 0).  Integer sums:
    exact, whatever the order of the windows."""
    dev = pairQ.device
    w = torch.as_tensor(w).to(device=dev, dtype=torch.float64)
    if w.ndim != 2:
        raise ValueError(f"pair_accumulate_host: w {tuple(w.shape)} is not [n, G]")
    n, G = w.shape
    r0, per = int(r0), int(per)
    if per < 1 or per > MAX_PER or r0 < 0:
        raise ValueError(f"pair_accumulate_host: need 1 <= per <= 2^22 and r0 >= 0, got {per} and {r0}")
    if (theta is None) != (edges is None):
        raise ValueError("pair_accumulate_host: theta and edges are given together")
    n_prev = 0
    if edges is not None:
        edges = torch.as_tensor(edges).to(device=dev, dtype=torch.float32)
        theta = torch.as_tensor(theta).to(device=dev, dtype=torch.float32)
        n_prev = edges.shape[0] if edges.ndim == 2 else -1
        if edges.ndim != 2 or edges.shape[1] != G + 1 or theta.ndim != 2 or theta.shape[0] != n or theta.shape[1] < n_prev:
            raise ValueError(f"pair_accumulate_host: theta {tuple(theta.shape)} / edges {tuple(edges.shape)} do not "
                             f"match {n} rows of {G} cells")
    U = cellQ.shape[0]
    if (pairQ.dtype != torch.int64 or cellQ.dtype != torch.int64 or bad.dtype != torch.int32
            or tuple(pairQ.shape) != (U, n_prev, G, G) or tuple(cellQ.shape) != (U, G) or tuple(bad.shape) != (U,)):
        raise ValueError(f"pair_accumulate_host: pairQ / cellQ / bad must be int64 [{U}, {n_prev}, {G}, {G}], int64 "
                         f"[{U}, {G}] and int32 [{U}]")
    if n == 0:
        return
    u = (r0 + torch.arange(n, device=dev)) // per
    if int(u[-1]) >= U:
        raise ValueError(f"pair_accumulate_host: rows {r0}..{r0 + n - 1} of {per} per observation exceed {U} observations")
    rowbad = torch.isnan(w).any(1)
    q = torch.round(torch.nan_to_num(w, nan=0.0) * PAIR_SCALE).to(torch.int64)
    q = torch.where(rowbad[:, None], torch.zeros_like(q), q)
    bad.index_fill_(0, u[rowbad], 1)
    cellQ.index_add_(0, u, q)
    flat = pairQ.view(-1, G)
    for j in range(n_prev):
        th = theta[:, j].contiguous()
        a = torch.searchsorted(edges[j].contiguous(), torch.nan_to_num(th, nan=0.0), right=True) - 1
        ok = (a >= 0) & (a < G) & ~torch.isnan(th) & ~rowbad
        flat.index_add_(0, ((u * n_prev + j) * G + a)[ok], q[ok])


def tables_from_sums(Q: Tensor, bad: Tensor, per: int) -> Tensor:
    """``Q / (2^40 per)`` in fp64 rounded to fp32, NaN for the observations of ``bad`` (k_pair_final)."""
    out = (Q.to(torch.float64) / (PAIR_SCALE * per)).to(torch.float32)
    out[bad.to(torch.bool)] = float("nan")
    return out


class PosteriorPairMarginals:
    """2-D posterior marginals of ``M`` observations on a grid of G cells per parameter.

    * ``probs`` [M, n_pairs, G, G]: ``probs[m, k (k - 1) / 2 + j, a, c]``, j < k, is the mass of
      (theta_j in cell a, theta_k in cell c) given x_m (:meth:`pair` picks and orients a table);
    * ``marginal_probs`` [M, d_theta, G]: the mass of theta_k in cell c (the 1-D marginals on the
      same cells);
    * ``edges`` [d_theta, G + 1]: the cell edges of every parameter; cell a is ``[edges[a],
      edges[a + 1])``;
    * ``num_draws``: draws per observation behind the tables;
    * ``samples`` [M, num_draws, d_theta] when asked for, else None.

    Mass outside the limits ``edges[:, 0]``, ``edges[:, -1]`` of either parameter is not in a
    table: :meth:`mass_inside` says how much is.  Like ``marginals``, these are the marginals of
    the estimator BEFORE truncation to the prior's support.
    """

    def __init__(self, probs: Tensor, marginal_probs: Tensor, edges: Tensor, num_draws: int,
                 samples: Optional[Tensor] = None):
        probs = torch.as_tensor(probs)
        marginal_probs = torch.as_tensor(marginal_probs)
        edges = torch.as_tensor(edges)
        if marginal_probs.ndim != 3 or marginal_probs.shape[2] < 2:
            raise ValueError(f"PosteriorPairMarginals: marginal_probs {tuple(marginal_probs.shape)} must be "
                             "[M, d_theta, G >= 2]")
        M, d, G = marginal_probs.shape
        if tuple(probs.shape) != (M, d * (d - 1) // 2, G, G) or tuple(edges.shape) != (d, G + 1):
            raise ValueError(f"PosteriorPairMarginals: probs {tuple(probs.shape)} must be [{M}, {d * (d - 1) // 2}, "
                             f"{G}, {G}] and edges {tuple(edges.shape)} [{d}, {G + 1}]")
        if not bool((edges[:, 1:] > edges[:, :-1]).all()):
            raise ValueError("PosteriorPairMarginals: every row of edges must be strictly increasing")
        self.probs = probs
        self.marginal_probs = marginal_probs.to(probs.device)
        self.edges = edges.to(probs.device)
        self.num_draws = int(num_draws)
        self.samples = samples

    # ------------------------------------------------------------------ shapes
    @property
    def num_observations(self) -> int:
        return self.marginal_probs.shape[0]

    @property
    def dim_theta(self) -> int:
        return self.marginal_probs.shape[1]

    @property
    def bins(self) -> int:
        return self.marginal_probs.shape[2]

    def centres(self) -> Tensor:
        """Cell centres [d_theta, G] (float64)."""
        e = self.edges.to(torch.float64)
        return (e[:, 1:] + e[:, :-1]) / 2

    def widths(self) -> Tensor:
        """Cell widths [d_theta, G] (float64)."""
        e = self.edges.to(torch.float64)
        return e[:, 1:] - e[:, :-1]

    def _check_pair(self, j: int, k: int):
        j, k = int(j), int(k)
        d = self.dim_theta
        if not (0 <= j < d and 0 <= k < d):
            raise ValueError(f"pair: parameters ({j}, {k}) are not in 0..{d - 1}")
        if j == k:
            raise ValueError(f"pair: the two parameters must differ (got {j} twice); the 1-D marginal is "
                             "marginal_probs[:, j]")
        return j, k

    # --------------------------------------------------------------- summaries
    def pair(self, j: int, k: int) -> Tensor:
        """[M, G, G] masses of (theta_j, theta_k): the first cell axis is parameter ``j``, the
        second ``k`` (the stored table transposed when j > k).  ValueError for j == k."""
        j, k = self._check_pair(j, k)
        if j < k:
            return self.probs[:, pair_index(j, k)]
        return self.probs[:, pair_index(k, j)].transpose(-1, -2)

    def density(self, j: int, k: int) -> Tensor:
        """[M, G, G] (float64): mass divided by cell area."""
        j, k = self._check_pair(j, k)
        w = self.widths()
        return self.pair(j, k).to(torch.float64) / (w[j][:, None] * w[k][None, :])

    def mass_inside(self, j: int, k: int) -> Tensor:
        """[M] (float64): the mass of (theta_j, theta_k) inside the limits of both parameters."""
        return self.pair(j, k).to(torch.float64).sum((-1, -2))

    def credible_region(self, j: int, k: int, level: float = 0.9) -> Tensor:
        """Boolean [M, G, G]: the densest cells that hold ``level`` of the mass inside the limits --
        cells are taken in order of decreasing density until their mass reaches ``level *
        mass_inside(j, k)``; what a contour is drawn from.  ValueError for a level outside (0, 1]."""
        level = float(level)
        if not 0.0 < level <= 1.0:
            raise ValueError(f"credible_region: level must lie in (0, 1], got {level!r}")
        mass = self.pair(j, k).to(torch.float64)
        M, G = mass.shape[0], mass.shape[-1]
        dens = self.density(j, k).reshape(M, -1)
        mass = mass.reshape(M, -1)
        order = torch.argsort(dens, dim=1, descending=True, stable=True)
        m_sorted = mass.gather(1, order)
        before = torch.cumsum(m_sorted, 1) - m_sorted
        take = (before < level * mass.sum(1, keepdim=True)) & (m_sorted > 0)
        return torch.zeros_like(take).scatter_(1, order, take).reshape(M, G, G)

    def correlation(self) -> Tensor:
        """[M, d_theta, d_theta] (float64): Pearson correlation of every pair from the cell centres,
        each table normalised by its mass inside the limits (its own two margins give the means
        and variances); 1 on the diagonal.  NaN where a margin has no spread."""
        M, d = self.num_observations, self.dim_theta
        ctr = self.centres()
        out = torch.ones((M, d, d), dtype=torch.float64, device=self.probs.device)
        for k in range(d):
            for j in range(k):
                p = self.pair(j, k).to(torch.float64)
                p = p / p.sum((-1, -2), keepdim=True)
                pj, pk = p.sum(-1), p.sum(-2)
                mj, mk = pj @ ctr[j], pk @ ctr[k]
                vj = pj @ (ctr[j] ** 2) - mj ** 2
                vk = pk @ (ctr[k] ** 2) - mk ** 2
                cov = torch.einsum("mac,a,c->m", p, ctr[j], ctr[k]) - mj * mk
                out[:, j, k] = out[:, k, j] = cov / torch.sqrt(vj * vk)
        return out
