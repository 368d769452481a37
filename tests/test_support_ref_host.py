"""The references and bounds of tests/support_ref.py and the k-means pins, without a GPU.

The GPU tests (tests/test_gpu_support.py, tests/test_gpu_kmeans.py) accept a device answer that
differs from the fp64 order only inside a derived rounding bound.  That is a check only while
few rows or groups sit inside the bound, so the conditions are asserted here for every GPU case:

* K12: the rows within their bound of the k-th distance number at most ``filter_band_cap(k)``;
  no column mean or std lies within 1e-9 relative of an fp32 rounding midpoint (the device adds
  in another order); a float32 emulation of the kernel without FMA stays inside the bound (it
  uses at most 0.11 of it); the torch formula of ``standardized_euclidean_filtering`` (the CPU
  fallback) passes ``check_filter`` on the same cases, which pins the reference itself.
* K11: the groups whose target lies within 2^-20 s of a CDF step number at most
  ``max(1, G // 500)`` (1 group at (1000, 100), 0 elsewhere).
* K13: ``kmeans_ref.fit`` on the degenerate inputs gives the counts and iteration counts written
  out below, so an edit of the reference cannot move them silently.

Each test prints its figures (``pytest -s``).
"""
import numpy as np
import pytest
import torch

import kmeans_ref
import support_ref as sr
from oracle.support_oracle import sir_select as oracle_sir

FILTER_IDS = [f"{n}x{d}-k{k}" + ("-shift" if s else "") for n, d, k, s in sr.FILTER_SHAPES]


@pytest.mark.parametrize("n,dim,k,shift", sr.FILTER_SHAPES, ids=FILTER_IDS)
def test_filter_case_conditions(n, dim, k, shift):
    x, obs = sr.filter_case(n, dim, k, shift)
    d, bound = sr.filter_rank(x, obs)
    in_band = sr.filter_in_band(x, obs, k)
    mean, std = sr.column_stats64(x)
    margin = min(sr.midpoint_margin(mean), sr.midpoint_margin(std))
    share = float(np.max(np.abs(sr.filter_emulate_fp32(x, obs).astype(np.float64) - d) / bound))
    print(f"K12 n={n} dim={dim} k={k} shift={shift}: in-band rows {in_band} (cap {sr.filter_band_cap(k)}), "
          f"midpoint margin {margin:.2e}, fp32 emulation uses {share:.3f} of the bound")
    assert 1 <= in_band <= sr.filter_band_cap(k)
    assert margin > 1e-9
    assert share <= 1.0


@pytest.mark.parametrize("n,dim,k,shift", sr.FILTER_SHAPES, ids=FILTER_IDS)
def test_cpu_fallback_passes_check_filter(n, dim, k, shift):
    from npe_pfn.support_posterior import standardized_euclidean_filtering

    x, obs = sr.filter_case(n, dim, k, shift)
    rows = torch.arange(n, dtype=torch.float32)[:, None]  # exact: n < 2^24
    th, xs = standardized_euclidean_filtering(torch.from_numpy(obs), rows, torch.from_numpy(x), k)
    idx = th[:, 0].long().numpy()
    assert torch.equal(xs, torch.from_numpy(x)[idx])
    use = sr.check_filter(idx, x, obs, k)
    print(f"K12 fallback n={n} dim={dim} k={k} shift={shift}: order violations use {use:.3f} of the bound")


def test_check_filter_refuses_wrong_answers():
    x, obs = sr.filter_case(1000, 4, 100)
    d, _ = sr.filter_rank(x, obs)
    order = np.argsort(d, kind="stable")
    good = order[:100]
    assert sr.check_filter(good, x, obs, 100) == 0.0
    with pytest.raises(AssertionError, match="unselected|selected"):
        sr.check_filter(np.concatenate([good[:-1], order[100:101]]), x, obs, 100)  # the 101st for the 100th
    with pytest.raises(AssertionError, match="out of order"):
        sr.check_filter(np.concatenate([good[1:2], good[0:1], good[2:]]), x, obs, 100)
    with pytest.raises(AssertionError, match="repeated"):
        sr.check_filter(np.concatenate([good[:-1], good[:1]]), x, obs, 100)
    with pytest.raises(AssertionError, match="range"):
        sr.check_filter(np.concatenate([good[:-1], [1000]]), x, obs, 100)
    with pytest.raises(AssertionError):
        sr.check_filter(good[:99], x, obs, 100)


def test_midpoint_margin():
    one = np.float64(np.float32(1.0))
    ulp = np.float64(np.nextafter(np.float32(1.0), np.float32(2.0))) - one
    assert sr.midpoint_margin(np.array([one + 0.5 * ulp])) == 0.0
    assert sr.midpoint_margin(np.array([one + 0.25 * ulp])) == pytest.approx(0.25 * ulp, rel=1e-6)
    assert sr.midpoint_margin(np.array([one])) == pytest.approx(0.5 * ulp, rel=1e-6)


@pytest.mark.parametrize("G,k", sr.SIR_SHAPES)
def test_sir_case_conditions(G, k):
    _, lpr, lq, thr = sr.sir_shape_case(G, k)
    c, s, u = sr.sir_steps(lpr.numpy(), lq.numpy(), float(thr), k, sr.SIR_SEED, sr.SIR_COUNTER)
    in_band = sr.sir_in_band(c, s, u)
    print(f"K11 G={G} k={k}: groups with the target within 2^-20 s of a step: {in_band} "
          f"(cap {max(1, G // 500)})")
    assert in_band <= max(1, G // 500)
    # the steps restate the oracle: its pick is the first step past the target
    ref_pick, _ = oracle_sir(lpr.numpy(), lq.numpy(), float(thr), k, sr.SIR_SEED, sr.SIR_COUNTER)
    live = s > 0
    first = np.argmax(c > (u * s)[:, None], axis=1)
    past = ~(c > (u * s)[:, None]).any(axis=1)
    np.testing.assert_array_equal(first[live & ~past], ref_pick[live & ~past])


def test_sir_mismatch_is_rounding_rule():
    c = np.array([1.0, 2.0, 2.0, 4.0])
    s = 4.0
    eps = 0.5 * sr.SIR_BAND * s
    assert sr.sir_mismatch_is_rounding(c, s, (2.0 + eps) / s, 1, 3)       # steps 1, 2 both in the band
    assert sr.sir_mismatch_is_rounding(c, s, (2.0 - eps) / s, 3, 1)
    assert not sr.sir_mismatch_is_rounding(c, s, (2.0 + eps) / s, 0, 3)   # step 0 is far from the target
    assert not sr.sir_mismatch_is_rounding(c, s, (2.0 + 4 * eps) / s, 1, 2)
    assert not sr.sir_mismatch_is_rounding(c, s, 0.5, 1, 4)               # a pick out of range
    assert sr.sir_mismatch_is_rounding(c, s, 0.1, 2, 2)


# --------------------------------------------------------------------------- K13 pins
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_kmeans_ref_fewer_distinct_points_than_k(seed):
    pts = kmeans_ref.few_distinct_points()
    cen, lab, cnt, it = kmeans_ref.fit(pts, 8, seed)
    assert cnt.tolist() == [40, 40, 40, 40, 40, 0, 0, 0] and it == 1
    # the first five centres are the five distinct rows; the rest repeat one (all-duplicates seeding)
    assert sorted(map(tuple, cen[:5])) == sorted(map(tuple, kmeans_ref.FIVE_ROWS))
    assert all(tuple(c) in set(map(tuple, kmeans_ref.FIVE_ROWS)) for c in cen[5:])


def test_kmeans_ref_identical_points():
    cen, lab, cnt, it = kmeans_ref.fit(kmeans_ref.identical_points(), 4, 0)
    assert cnt.tolist() == [100, 0, 0, 0] and it == 1
    assert np.array_equal(cen, np.full((4, 3), 2.0, np.float32)) and not lab.any()


LATTICE_PINS = {  # (n, k, seed) -> (counts, n_iter), the same at tol 1e-4 and at tol 0
    (129, 4, 0): ([32, 28, 40, 29], 3), (129, 4, 1): ([40, 40, 21, 28], 7), (129, 4, 2): ([40, 35, 24, 30], 2),
    (64, 2, 0): ([32, 32], 3), (64, 2, 1): ([36, 28], 2), (64, 2, 2): ([32, 32], 4),
    (1000, 7, 0): ([236, 118, 177, 116, 118, 177, 58], 2), (1000, 7, 1): ([118, 236, 177, 118, 174, 118, 59], 2),
    (1000, 7, 2): ([118, 177, 236, 116, 118, 117, 118], 2),
}


@pytest.mark.parametrize("tol", [1e-4, 0.0])
@pytest.mark.parametrize("n,k,seed", sorted(LATTICE_PINS))
def test_kmeans_ref_lattice(n, k, seed, tol):
    cen, lab, cnt, it = kmeans_ref.fit(kmeans_ref.lattice_points(n), k, seed, tol=tol)
    assert (cnt.tolist(), it) == LATTICE_PINS[n, k, seed]
    assert it < 300  # at tol 0 the shift reached 0 exactly


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_kmeans_ref_symmetric_ties(seed):
    cen, lab, cnt, it = kmeans_ref.fit(kmeans_ref.symmetric_points(), 2, seed)
    assert cnt.tolist() == [100, 50]
    assert sorted(np.abs(cen[:, 0]).tolist()) == [0.5, 1.0]


def test_kmeans_ref_midway_queries_take_the_lower_index():
    cen = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]], np.float32)
    q = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 2.0]], np.float32)  # 0|1, 0|2, all three, 1|2
    assert kmeans_ref.assign(q, cen).tolist() == [0, 0, 0, 1]
