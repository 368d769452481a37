"""Seeded k-means for the unconditional estimator (K13, include/npfn.h ``npfn_kmeans_fit``).

The reference clusters the thetas with ``sklearn.cluster.KMeans`` on the host (npe_pfn.py:793-794)
and calls ``KMeans.predict`` inside every ``log_prob`` (:855).  Here the clustering is one fixed
algorithm -- k-means++ seeding with one Philox candidate per centre, Lloyd iterations, every
distance and sum in fp64 on the fp32 points -- with two implementations that give the same
clusters:

* the engine's HIP kernels (``Engine.kmeans_fit`` / ``Engine.kmeans_assign``) when an engine is
  given: thetas, labels and centres stay on the device;
* a numpy restatement otherwise (the generic estimator path, e.g. the CPU oracle in
  tests/test_uncond_orchestration.py).

:class:`KMeansState` holds the result as plain tensors, so it pickles with the estimator.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

_ROWS_PER_BLOCK = 1 << 16


def _philox_uniforms(seed: int, counter: int, n: int) -> np.ndarray:
    """u(seed, counter, row), row < n: Philox4x32-10 (Salmon et al., SC'11) on the counter block
    (row_lo, row_hi, counter_lo, counter_hi) keyed by (seed_lo, seed_hi); the first output word's
    top 24 bits -- the engine's ``philox_uniform`` (csrc/npfn_common.h)."""
    mask = np.uint64(0xFFFFFFFF)
    seed &= 0xFFFFFFFFFFFFFFFF
    counter &= 0xFFFFFFFFFFFFFFFF
    row = np.arange(n, dtype=np.uint64)
    ctr = [row & mask, row >> np.uint64(32), np.full(n, counter & 0xFFFFFFFF, np.uint64),
           np.full(n, counter >> 32, np.uint64)]
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for _ in range(10):
        a = np.uint64(0xD2511F53) * ctr[0]
        b = np.uint64(0xCD9E8D57) * ctr[2]
        ctr = [(b >> np.uint64(32)) ^ ctr[1] ^ np.uint64(key[0]), b & mask,
               (a >> np.uint64(32)) ^ ctr[3] ^ np.uint64(key[1]), a & mask]
        key = [(key[0] + 0x9E3779B9) & 0xFFFFFFFF, (key[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return (ctr[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def _nearest(p: np.ndarray, cen: np.ndarray):
    """(label, squared distance) of the nearest row of cen per row of p, ties to the lower index."""
    best = np.full(p.shape[0], np.inf)
    lab = np.zeros(p.shape[0], dtype=np.int64)
    for c in range(cen.shape[0]):
        diff = p - cen[c]
        dist = (diff * diff).sum(axis=1)
        closer = dist < best
        best[closer] = dist[closer]
        lab[closer] = c
    return lab, best


def host_assign(pts: np.ndarray, centers: np.ndarray) -> np.ndarray:
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    cen = np.asarray(centers, dtype=np.float32).astype(np.float64)
    out = np.empty(pts.shape[0], dtype=np.int64)
    for i in range(0, pts.shape[0], _ROWS_PER_BLOCK):
        out[i: i + _ROWS_PER_BLOCK] = _nearest(pts[i: i + _ROWS_PER_BLOCK].astype(np.float64), cen)[0]
    return out


def host_fit(pts: np.ndarray, k: int, seed: int, max_iter: int = 300, tol: float = 1e-4):
    """The algorithm of ``npfn_kmeans_fit`` in numpy fp64 -> (centers float32 [k, dim], labels, counts, n_iter)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n, dim = pts.shape
    if k < 1 or k > n:
        raise ValueError(f"kmeans: need 1 <= k <= n_rows, got k = {k} and n_rows = {n}")
    p = pts.astype(np.float64)
    tol_abs = float(np.float32(tol)) * float(np.mean(np.var(p, axis=0)))
    u = _philox_uniforms(seed, 0, k)
    # k-means++, one candidate per centre
    cen = np.empty((k, dim))
    cen[0] = p[min(int(u[0] * n), n - 1)]
    d2 = None
    for c in range(1, k):
        diff = p - cen[c - 1]
        dist = (diff * diff).sum(axis=1)
        d2 = dist if d2 is None else np.minimum(d2, dist)
        prefix = np.cumsum(d2)
        total = prefix[-1]
        if total == 0.0:
            row = min(int(u[c] * n), n - 1)
        else:
            row = int(np.searchsorted(prefix, u[c] * total, side="right"))  # first prefix > target
            if row >= n:
                row = int(np.flatnonzero(d2 > 0.0)[-1])
        cen[c] = p[row]
    # Lloyd
    n_iter = 0
    for _ in range(max_iter):
        lab, _ = _nearest(p, cen)
        cnt = np.bincount(lab, minlength=k)
        sums = np.zeros((k, dim))
        for j in range(dim):
            sums[:, j] = np.bincount(lab, weights=p[:, j], minlength=k)
        moved = np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], cen)
        shift = float(((moved - cen) ** 2).sum())
        cen = moved
        n_iter += 1
        if shift <= tol_abs:
            break
    centers = cen.astype(np.float32)
    labels = host_assign(pts, centers)
    return centers, labels, np.bincount(labels, minlength=k).astype(np.int64), n_iter


class KMeansState:
    """Fitted clustering: ``centers`` [k, dim] float32 and ``labels_`` [n] int64 on the thetas'
    device, ``counts`` [k] int64 on the host, ``n_iter``."""

    def __init__(self, num_clusters: int, seed: int = 0, max_iter: int = 300, tol: float = 1e-4):
        self.num_clusters = int(num_clusters)
        self.seed = int(seed)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.centers: Optional[Tensor] = None
        self.labels_: Optional[Tensor] = None
        self.counts: Optional[Tensor] = None
        self.n_iter = 0

    def fit(self, theta: Tensor, engine=None) -> "KMeansState":
        """Cluster theta [n, dim]; on the device through ``engine`` when one is given."""
        if engine is not None:
            centers, labels, counts, n_iter = engine.kmeans_fit(theta, self.num_clusters, self.seed, self.max_iter,
                                                                self.tol)
            self.centers, self.labels_ = centers.to(theta.device), labels.to(theta.device)
            self.counts, self.n_iter = counts.cpu(), int(n_iter.item())
            return self
        centers, labels, counts, n_iter = host_fit(theta.detach().cpu().numpy(), self.num_clusters, self.seed,
                                                   self.max_iter, self.tol)
        self.centers = torch.from_numpy(centers).to(theta.device)
        self.labels_ = torch.from_numpy(labels).to(theta.device)
        self.counts, self.n_iter = torch.from_numpy(counts), n_iter
        return self

    def predict(self, theta: Tensor, engine=None) -> Tensor:
        """Index of the nearest centre per row of theta (on theta's device)."""
        if self.centers is None:
            raise RuntimeError("KMeansState.predict before fit")
        if engine is not None:
            return engine.kmeans_assign(theta, self.centers).to(theta.device)
        lab = host_assign(theta.detach().cpu().numpy(), self.centers.cpu().numpy())
        return torch.from_numpy(lab).to(theta.device)
