"""K13 on the host: the product's numpy k-means (npe_pfn/kmeans.py) against the independent
restatement tests/kmeans_ref.py, against the true partition of separated blobs, and against
sklearn's KMeans on those blobs (CPU, no GPU needed).
"""
import numpy as np
import pytest
import torch

import kmeans_ref

CASES = [(64, 1, 2), (257, 33, 4), (1000, 4, 5), (4099, 7, 8), (20000, 3, 16), (300001, 2, 3),
         (10, 3, 1), (5, 2, 5), (64, 64, 64)]
BLOBS = [(300, 2, 3), (1000, 4, 5), (257, 33, 4)]


def _points(n, d, seed):
    return np.random.default_rng(100 + seed).standard_normal((n, d)).astype(np.float32)


def _blobs(n, d, k):
    """Unit-normal blobs around k centres at least 8 apart (centre c sits at 8 c on every axis:
    neighbours are 8 sqrt(d) >= 8 apart); every blob gets members."""
    rng = np.random.default_rng(n + d + k)
    truth = np.arange(n) % k
    rng.shuffle(truth)
    pts = rng.standard_normal((n, d)) + 8.0 * truth[:, None]
    return pts.astype(np.float32), truth


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_philox_of_the_host_path_is_the_oracles():
    from npe_pfn.kmeans import _philox_uniforms
    from oracle.philox import uniforms

    for seed, counter in ((0, 0), (7, 3), (2 ** 40 + 5, 2 ** 33 + 1)):
        np.testing.assert_array_equal(_philox_uniforms(seed, counter, 70).astype(np.float32),
                                      uniforms(seed, counter, 70))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,d,k", CASES)
def test_host_path_equals_restatement(n, d, k, seed):
    from npe_pfn.kmeans import host_fit

    pts = _points(n, d, seed)
    cen, lab, cnt, it = host_fit(pts, k, seed)
    rcen, rlab, rcnt, rit = kmeans_ref.fit(pts, k, seed)
    assert it == rit
    np.testing.assert_array_equal(lab, rlab)
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_allclose(cen, rcen, rtol=1e-6)
    assert cen.dtype == np.float32 and lab.dtype == np.int64 and cnt.sum() == n


@pytest.mark.parametrize("n,d,k", BLOBS)
def test_separated_blobs_are_recovered(n, d, k):
    from sklearn.cluster import KMeans

    from npe_pfn.kmeans import KMeansState

    pts, truth = _blobs(n, d, k)
    km = KMeansState(k, seed=0).fit(torch.from_numpy(pts))
    lab = km.labels_.numpy()
    assert _same_partition(lab, truth)
    sk = KMeans(n_clusters=k, n_init=10, random_state=0).fit(pts.astype(np.float64))
    assert _same_partition(lab, sk.labels_)
    np.testing.assert_array_equal(km.counts.numpy(), np.bincount(lab, minlength=k))


@pytest.mark.parametrize("n,d,k", [(257, 33, 4), (1000, 4, 5), (64, 64, 64)])
def test_predict_of_the_training_rows_is_labels(n, d, k):
    from npe_pfn.kmeans import KMeansState

    pts = torch.from_numpy(_points(n, d, 1))
    km = KMeansState(k, seed=1).fit(pts)
    assert torch.equal(km.predict(pts), km.labels_)
    assert km.centers.shape == (k, d) and km.centers.dtype == torch.float32


def test_host_path_rejects_more_clusters_than_rows():
    from npe_pfn.kmeans import host_fit

    with pytest.raises(ValueError, match="k"):
        host_fit(_points(5, 2, 0), 6, 0)


def test_package_does_not_import_sklearn():
    import os
    import re

    from conftest import ROOT

    pkg = os.path.join(ROOT, "npe-pfn_amd", "npe_pfn")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            src = open(os.path.join(pkg, name)).read()
            assert not re.search(r"^\s*(from|import)\s+sklearn", src, flags=re.M), name
