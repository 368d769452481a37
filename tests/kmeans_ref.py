"""numpy restatement of K13 (include/npfn.h ``npfn_kmeans_fit`` / ``npfn_kmeans_assign``).

Test infrastructure only: written from the algorithm's statement, not from the product's host
path (npe_pfn/kmeans.py), so that the two can be held against each other.  All distances and
sums are fp64 on the fp32 points.
"""
from __future__ import annotations

import numpy as np

from oracle.philox import uniforms


def _sqdist(p64: np.ndarray, centre: np.ndarray) -> np.ndarray:
    d = p64 - centre[None, :]
    return np.einsum("ij,ij->i", d, d)


def assign(pts: np.ndarray, centers: np.ndarray) -> np.ndarray:
    """labels[i] = argmin_c |pts[i] - centers[c]|^2, ties to the lower c."""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    c = np.asarray(centers).astype(np.float64)
    dist = np.stack([_sqdist(p, c[j]) for j in range(c.shape[0])], axis=1)
    return np.argmin(dist, axis=1).astype(np.int64)  # argmin returns the first minimum


def seed_rows(p: np.ndarray, k: int, seed: int) -> list:
    """k-means++ with one candidate per centre: the rows chosen as initial centres."""
    n = p.shape[0]
    u = uniforms(seed, 0, k).astype(np.float64)
    rows = [min(int(np.floor(u[0] * n)), n - 1)]
    d2 = _sqdist(p, p[rows[0]])
    for c in range(1, k):
        cum = np.cumsum(d2)
        tot = cum[-1]
        if tot == 0.0:
            r = min(int(np.floor(u[c] * n)), n - 1)
        else:
            hit = np.nonzero(cum > u[c] * tot)[0]
            r = int(hit[0]) if hit.size else int(np.nonzero(d2 > 0)[0][-1])
        rows.append(r)
        d2 = np.minimum(d2, _sqdist(p, p[r]))
    return rows


def fit(pts: np.ndarray, k: int, seed: int, max_iter: int = 300, tol: float = 1e-4):
    """-> centers [k, dim] float32, labels [n] int64, counts [k] int64, n_iter."""
    pts = np.asarray(pts, dtype=np.float32)
    p = pts.astype(np.float64)
    n, dim = p.shape
    if not (1 <= k <= n):
        raise ValueError("need 1 <= k <= n")
    tol_abs = float(np.float32(tol)) * p.var(axis=0).mean()
    cen = p[seed_rows(p, k, seed)].copy()
    n_iter = 0
    while n_iter < max_iter:
        lab = assign(pts, cen)
        new = cen.copy()
        for c in range(k):
            m = lab == c
            if m.any():
                new[c] = p[m].sum(axis=0) / m.sum()
        shift = ((new - cen) ** 2).sum()
        cen = new
        n_iter += 1
        if shift <= tol_abs:
            break
    centers = cen.astype(np.float32)
    labels = assign(pts, centers)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    return centers, labels, counts, n_iter


# Degenerate inputs shared by tests/test_support_ref_host.py (which pins what `fit` gives on
# them) and tests/test_gpu_kmeans.py (which holds the device to it).  Every coordinate is a small
# integer, so every member sum is exact in any order and the centres must agree bit for bit.
FIVE_ROWS = np.array([[0, 0, 0], [4, 1, 0], [1, 5, 2], [7, 7, 7], [2, 8, 3]], dtype=np.float32)
LATTICE_SHAPES = [(129, 4), (64, 2), (1000, 7)]


def few_distinct_points() -> np.ndarray:
    """5 distinct rows tiled 40x: fewer distinct points than the k = 8 asked for."""
    return np.tile(FIVE_ROWS, (40, 1))


def identical_points() -> np.ndarray:
    return np.full((100, 3), 2.0, dtype=np.float32)


def lattice_points(n: int) -> np.ndarray:
    return (np.arange(n) % 17).astype(np.float32)[:, None]


def symmetric_points() -> np.ndarray:
    """{-1, 0, 1} x 50 in one dimension: 0 is exactly midway between centres at -1 and 1."""
    return np.tile(np.array([-1.0, 0.0, 1.0], dtype=np.float32), 50)[:, None]


class KMeansShim:
    """The part of sklearn.cluster.KMeans the reference's unconditional estimator uses
    (``fit``, ``labels_``, ``predict``), over this module (tests/golden/make_golden_uncond.py)."""

    seed = 0

    def __init__(self, n_clusters: int = 1, **_ignored):
        self.n_clusters = n_clusters

    def fit(self, X):
        self.cluster_centers_, self.labels_, self.counts_, self.n_iter_ = fit(X, self.n_clusters, self.seed)
        return self

    def predict(self, X):
        return assign(X, self.cluster_centers_)
