"""K13 on the GPU: npfn_kmeans_fit / npfn_kmeans_assign through the C-ABI against the numpy
restatement tests/kmeans_ref.py.

Labels, counts and the iteration count must be equal exactly, the centres within one fp32
rounding (rtol 1e-6; an ulp is 1.2e-7): both sides compute every distance and sum in fp64, and
on these inputs the closest call is far from fp64 summation-order noise (~1e-13 relative) --
the smallest relative gap between a point's two nearest centres over all Lloyd iterations is
1.7e-9, the smallest relative distance of a seeding target from a prefix-sum step 6.5e-8.
"""
import numpy as np
import pytest
import torch

import kmeans_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

SHAPES = [(64, 1, 2), (257, 33, 4), (1000, 4, 5), (4099, 7, 8), (20000, 3, 16), (300001, 2, 3),
          (10, 3, 1), (5, 2, 5), (64, 64, 64)]  # the last three: k = 1, k = n, k * dim at the LDS cap


@pytest.fixture(scope="module")
def engine():
    from npe_pfn.engine import Engine

    return Engine(device=DEV)


def _points(n, d, seed):
    return np.random.default_rng(100 + seed).standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_fit_matches_restatement(engine, n, d, k, seed):
    pts = _points(n, d, seed)
    rcen, rlab, rcnt, rit = kmeans_ref.fit(pts, k, seed)
    dev = torch.from_numpy(pts).to(DEV)
    cen, lab, cnt, it = engine.kmeans_fit(dev, k, seed)
    assert cen.dtype == torch.float32 and lab.dtype == torch.int64 and cnt.dtype == torch.int64
    print(f"n={n} d={d} k={k} seed={seed}: n_iter gpu {int(it)} ref {rit}, label mismatches "
          f"{int((lab.cpu().numpy() != rlab).sum())}")
    assert int(it) == rit
    np.testing.assert_array_equal(lab.cpu().numpy(), rlab)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_allclose(cen.cpu().numpy(), rcen, rtol=1e-6)
    # predict on the training rows returns the fit's labels bit for bit
    assert torch.equal(engine.kmeans_assign(dev, cen), lab)
    # the same inputs and seed give the same bits
    cen2, lab2, cnt2, it2 = engine.kmeans_fit(dev, k, seed)
    assert torch.equal(cen2, cen) and torch.equal(lab2, lab) and torch.equal(cnt2, cnt) and torch.equal(it2, it)


def test_assign_on_new_points_matches_restatement(engine):
    pts, query = _points(1000, 4, 0), _points(777, 4, 9)
    cen, _, _, _ = engine.kmeans_fit(torch.from_numpy(pts).to(DEV), 5, 0)
    lab = engine.kmeans_assign(torch.from_numpy(query).to(DEV), cen)
    np.testing.assert_array_equal(lab.cpu().numpy(), kmeans_ref.assign(query, cen.cpu().numpy()))


def test_max_iter_stops_the_iteration(engine):
    pts = _points(4099, 7, 0)
    for max_iter in (1, 3, 9):  # below, and one past, the host's look at the convergence flag
        rcen, rlab, _, rit = kmeans_ref.fit(pts, 8, 0, max_iter=max_iter)
        cen, lab, _, it = engine.kmeans_fit(torch.from_numpy(pts).to(DEV), 8, 0, max_iter=max_iter)
        assert int(it) == rit <= max_iter
        np.testing.assert_array_equal(lab.cpu().numpy(), rlab)
        np.testing.assert_allclose(cen.cpu().numpy(), rcen, rtol=1e-6)


def test_caps_are_refused(engine):
    from npe_pfn.engine import EngineError

    with pytest.raises(EngineError, match="exceeds n_rows"):
        engine.kmeans_fit(torch.zeros(5, 2, device=DEV), 6, 0)
    with pytest.raises(EngineError, match="4096"):
        engine.kmeans_fit(torch.zeros(100, 64, device=DEV), 65, 0)
    with pytest.raises(EngineError, match="4096"):
        engine.kmeans_assign(torch.zeros(10, 64, device=DEV), torch.zeros(65, 64, device=DEV))
    with pytest.raises(EngineError, match="k >= 1"):
        engine.kmeans_fit(torch.zeros(5, 2, device=DEV), 0, 0)
