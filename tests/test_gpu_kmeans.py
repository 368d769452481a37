"""K13 on the GPU: npfn_kmeans_fit / npfn_kmeans_assign through the C-ABI against the numpy
restatement tests/kmeans_ref.py.

Labels, counts and the iteration count must be equal exactly, the centres within one fp32
rounding (rtol 1e-6; an ulp is 1.2e-7): both sides compute every distance and sum in fp64, and
on these inputs the closest call is far from fp64 summation-order noise (~1e-13 relative) --
the smallest relative gap between a point's two nearest centres over all Lloyd iterations is
1.7e-9, the smallest relative distance of a seeding target from a prefix-sum step 6.5e-8.
The same two figures, measured on the CPU with the restatement, for the shapes added since
(relative gap of the squared distances, seeds 0-2):
  (1000, d, 6), d in 5, 6, 8, 9 (the last register-resident templates and the first generic
      one)                                            6.0e-6 and 2.8e-6
  n in 63..257 with d = 2, k = 3                      1.5e-5 and 1.4e-5
      ((1, 1, 1) has one centre and nothing to compare)
  (2000, 9, 6), seed 0 (51 iterations to converge)    1.1e-5 and 6.4e-5
  (33000, 64, 64), seed 0, 3 iterations               5.3e-7 and 1.8e-7

The degenerate inputs (kmeans_ref.few_distinct_points and the others there) have small integer
coordinates: every member sum is exact in any order, so there the centres must be equal bit for
bit, and exact distance ties must fall as the restatement's argmin does, to the lower index.
tests/test_support_ref_host.py pins what the restatement gives on them.
"""
import numpy as np
import pytest
import torch

import kmeans_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

SHAPES = [(64, 1, 2), (257, 33, 4), (1000, 4, 5), (4099, 7, 8), (20000, 3, 16), (300001, 2, 3),
          (10, 3, 1), (5, 2, 5), (64, 64, 64)]  # the last three: k = 1, k = n, k * dim at the LDS cap
SHAPES += [(1000, d, 6) for d in (5, 6, 8, 9)]  # templates 5, 6, 8 (the last in registers) and the generic one
SHAPES += [(1, 1, 1)] + [(n, 2, 3) for n in (63, 64, 65, 255, 256, 257)]  # around one wave and one block of rows


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


# --------------------------------------------------------------------------- degenerate data
def _fit_equals_restatement(engine, pts, k, seed, **kw):
    """Labels, counts, n_iter and (bit for bit) centres of the device against the restatement."""
    rcen, rlab, rcnt, rit = kmeans_ref.fit(pts, k, seed, **kw)
    cen, lab, cnt, it = engine.kmeans_fit(torch.from_numpy(pts).to(DEV), k, seed, **kw)
    assert int(it) == rit
    np.testing.assert_array_equal(lab.cpu().numpy(), rlab)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_array_equal(cen.cpu().numpy(), rcen)
    return rcen, rcnt, rit


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fewer_distinct_points_than_clusters(engine, seed):
    # the seeding runs out of distinct rows (sum(d2) == 0); the spare clusters stay empty
    _, cnt, it = _fit_equals_restatement(engine, kmeans_ref.few_distinct_points(), 8, seed)
    assert cnt.tolist() == [40, 40, 40, 40, 40, 0, 0, 0] and it == 1


def test_identical_points(engine):
    cen, cnt, it = _fit_equals_restatement(engine, kmeans_ref.identical_points(), 4, 0)
    assert cnt.tolist() == [100, 0, 0, 0] and it == 1
    assert np.array_equal(cen, np.full((4, 3), 2.0, np.float32))


@pytest.mark.parametrize("tol", [1e-4, 0.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,k", kmeans_ref.LATTICE_SHAPES)
def test_lattice_with_exact_ties(engine, n, k, seed, tol):
    _, _, it = _fit_equals_restatement(engine, kmeans_ref.lattice_points(n), k, seed, tol=tol)
    assert it < 300  # at tol = 0 only a shift of exactly 0 stops the iteration


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_symmetric_ties_go_to_the_lower_centre(engine, seed):
    _, cnt, _ = _fit_equals_restatement(engine, kmeans_ref.symmetric_points(), 2, seed)
    assert cnt.tolist() == [100, 50]


# --------------------------------------------------------------------------- iteration control
@pytest.mark.parametrize("max_iter", [0, 8, 16, 17])  # none; at, and one past, the host's flag reads
def test_max_iter_at_the_flag_reads(engine, max_iter):
    pts = _points(2000, 9, 0)  # 51 iterations when left to converge
    rcen, rlab, rcnt, rit = kmeans_ref.fit(pts, 6, 0, max_iter=max_iter)
    cen, lab, cnt, it = engine.kmeans_fit(torch.from_numpy(pts).to(DEV), 6, 0, max_iter=max_iter)
    assert int(it) == rit == max_iter
    np.testing.assert_array_equal(lab.cpu().numpy(), rlab)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_allclose(cen.cpu().numpy(), rcen, rtol=1e-6)
    if max_iter == 0:  # the seeding alone: the chosen rows bit for bit
        rows = kmeans_ref.seed_rows(pts.astype(np.float64), 6, 0)
        np.testing.assert_array_equal(cen.cpu().numpy(), pts[rows])


def test_converged_fit_ignores_a_larger_max_iter(engine):
    pts = torch.from_numpy(_points(2000, 9, 0)).to(DEV)
    a = engine.kmeans_fit(pts, 6, 0, max_iter=300)
    b = engine.kmeans_fit(pts, 6, 0, max_iter=56)  # converged at 51, before the flag read at 56
    assert int(a[3]) == int(b[3]) == 51
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_partial_sum_cap_sets_the_grid(engine):
    # (k dim + k) doubles per wave: the 16 MB cap allows 126 blocks where 33000 rows ask for 129
    pts = _points(33000, 64, 0)
    rcen, rlab, rcnt, rit = kmeans_ref.fit(pts, 64, 0, max_iter=3)
    cen, lab, cnt, it = engine.kmeans_fit(torch.from_numpy(pts).to(DEV), 64, 0, max_iter=3)
    assert int(it) == rit == 3
    np.testing.assert_array_equal(lab.cpu().numpy(), rlab)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_allclose(cen.cpu().numpy(), rcen, rtol=1e-6)


# --------------------------------------------------------------------------- kmeans_assign
def test_assign_midway_queries_take_the_lower_index(engine):
    cen = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]], np.float32)
    q = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 2.0]], np.float32)  # 0|1, 0|2, all three, 1|2
    lab = engine.kmeans_assign(torch.from_numpy(q), torch.from_numpy(cen)).cpu().numpy()
    assert lab.tolist() == [0, 0, 0, 1]
    np.testing.assert_array_equal(lab, kmeans_ref.assign(q, cen))
    # every template: a query at the origin between centres at +-e_0, in either order
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 33):
        c = np.zeros((3, d), np.float32)
        c[0, 0], c[1, 0], c[2, 0] = 5.0, -1.0, 1.0
        lab = engine.kmeans_assign(torch.zeros(130, d), torch.from_numpy(c))
        assert lab.cpu().tolist() == [1] * 130, d


def test_assign_one_row_and_no_rows(engine):
    cen = torch.from_numpy(_points(5, 4, 3)).to(DEV)
    q = _points(1, 4, 4)
    lab = engine.kmeans_assign(torch.from_numpy(q).to(DEV), cen)
    np.testing.assert_array_equal(lab.cpu().numpy(), kmeans_ref.assign(q, cen.cpu().numpy()))
    none = engine.kmeans_assign(torch.empty(0, 4, device=DEV), cen)
    assert none.shape == (0,) and none.dtype == torch.int64
