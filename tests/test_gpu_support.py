"""GPU parity of the support kernels (K9-K12) through the C-ABI.

* K11 ``npfn_sir_select`` vs oracle/support_oracle.sir_select on the same
  inputs and Philox stream: ESS within rtol 1e-5 (fp32 exp / fp64 sums on both
  sides), picks identical except where u * sum lands within rounding of a CDF
  step (allowed: <= 0.2 % of groups, and each such group must pass
  support_ref.sir_mismatch_is_rounding), gathered rows bit-exact for the pick;
* K9 mask + K10 ordered compaction vs torch boolean indexing: bit-exact;
* K12 standardized-Euclidean filter vs the reference-generated golden
  (tests/golden/filters.npz): bit-exact selection;
* PosteriorSupport (rejection and SIR) end to end on the engine, shaped like
  the reference's tests/test_support_posterior.py (sizes reduced).

Below the "edges" line, every chunk, wave and tie edge of the four kernels:

* K12 against the fp64 rank of tests/support_ref.py at sizes around one block of sort keys, far
  from a power of two, at k = 1, n - 1, n, with a shifted table; exact ties, all-NaN distances,
  k = 0 and the refused calls.  The conditions that make the acceptance strict (few rows within
  the bound of the k-th distance) are asserted in tests/test_support_ref_host.py.
  Measured on an MI355X, largest rank displacement / bound per case: 0.024 at 65537 x 4,
  k = 5000 (the CPU fallback's fp32 order shows the same 0.024 there) and 0.000 (the fp64 order
  itself) in the 15 other cases.
* K10 through the C-ABI into a sentinel-filled ``dst``: n on the 64- and 1024-row boundaries,
  empty to full masks, set bytes other than 1; rows from ``count`` on stay untouched.
* K9 at the closed bounds and one float outside them, NaN cells, signed zeros, infinite and
  inverted bounds, scalar bounds.
* K11 groups whose answer is exact (no mismatch allowed, ESS equal), the strict threshold, theta
  wider than a wave, ``group_offset`` splitting and the empty call.
  Measured on an MI355X: 0 mismatching groups in each of the 12 (G, k) cases, so no mismatch
  had to be justified (the host test finds 1 group in the band at (1000, 100), 0 elsewhere).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import support_ref as sr
from oracle.philox import uniforms
from oracle.support_oracle import box_mask, sir_select as oracle_sir

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("G,k", sr.SIR_SHAPES)
def test_sir_select_matches_oracle(G, k):
    from npe_pfn.support_posterior import sir_select

    th, lpr, lq, thr = sr.sir_shape_case(G, k)
    sel, pick, ess = sir_select(th.to(DEV), lpr.to(DEV), lq.to(DEV), thr.to(DEV), k, seed=sr.SIR_SEED,
                                counter=sr.SIR_COUNTER)
    ref_pick, ref_ess = oracle_sir(lpr.numpy(), lq.numpy(), float(thr), k, seed=sr.SIR_SEED, counter=sr.SIR_COUNTER)
    pick, ess, sel = pick.cpu().numpy(), ess.cpu().numpy(), sel.cpu().numpy()
    np.testing.assert_allclose(ess, ref_ess, rtol=1e-5)
    mism = np.flatnonzero(pick != ref_pick)
    print(f"K11 G={G} k={k}: {mism.size} mismatching groups (all must be rounding at a CDF step)")
    assert mism.size <= max(1, G // 500), (mism.size, G)
    c, s, u = sr.sir_steps(lpr.numpy(), lq.numpy(), float(thr), k, sr.SIR_SEED, sr.SIR_COUNTER)
    for g in mism:
        assert sr.sir_mismatch_is_rounding(c[g], s[g], u[g], pick[g], ref_pick[g]), \
            (int(g), int(pick[g]), int(ref_pick[g]), float(u[g]))
    np.testing.assert_array_equal(sel, th.numpy().reshape(G, k, 3)[np.arange(G), pick])


def test_sir_select_degenerate_groups():
    from npe_pfn.support_posterior import sir_select

    k = 10
    lq = torch.linspace(-5, 5, 3 * k)
    lpr = torch.zeros(3 * k)
    lpr[2 * k:] = float("nan")  # group 2: every ratio NaN -> -inf -> NaN probabilities in torch
    thr = torch.tensor(-4.0)  # group 0 partly, group 1 not truncated
    thr_all = torch.tensor(0.5)  # group 0 fully truncated: uniform like the reference
    th = torch.arange(3 * k * 2, dtype=torch.float32).reshape(3 * k, 2)
    for t in (thr, thr_all):
        _, pick, ess = sir_select(th.to(DEV), lpr.to(DEV), lq.to(DEV), t.to(DEV), k, seed=1)
        rp, re = oracle_sir(lpr.numpy(), lq.numpy(), float(t), k, seed=1, counter=0)
        np.testing.assert_allclose(ess.cpu().numpy()[:2], re[:2], rtol=1e-5)
        assert np.isnan(ess.cpu().numpy()[2]) and np.isnan(re[2])
        np.testing.assert_array_equal(pick.cpu().numpy(), rp)


def test_box_compact_bit_exact():
    from npe_pfn.support_posterior import box_compact

    g = torch.Generator().manual_seed(4)
    for n, D in [(100_000, 3), (1_000, 1), (0, 2), (5_000, 10)]:
        s = torch.randn(n, D, generator=g)
        lo, hi = -torch.rand(D, generator=g), torch.rand(D, generator=g)
        got = box_compact(s.to(DEV), lo.to(DEV), hi.to(DEV)).cpu()
        ref = s[torch.from_numpy(box_mask(s.numpy(), lo.numpy(), hi.numpy()))]
        assert torch.equal(got, ref)


def test_prereject_with_bounds_on_device():
    from npe_pfn.support_posterior import prereject_with_bounds

    prior = torch.distributions.Independent(
        torch.distributions.Normal(torch.zeros(2, device=DEV), torch.ones(2, device=DEV)), 1)
    lo, hi = torch.tensor([-0.5, -1.0], device=DEV), torch.tensor([1.0, 0.2], device=DEV)
    torch.manual_seed(0)
    s, rate = prereject_with_bounds(prior, lo, hi, sampling_batch_size=5000, pre_sampling_batch_size=20_000)
    assert s.shape == (5000, 2) and s.is_cuda
    assert bool(((s >= lo) & (s <= hi)).all())
    assert 0.1 < rate < 0.3  # P(box) = 0.2902 * 0.4207 = 0.122 for N(0, 1)


def test_stdeuclid_filter_matches_golden():
    from npe_pfn.support_posterior import standardized_euclidean_filtering

    g = np.load(os.path.join(GOLDEN, "filters.npz"))
    t, x = standardized_euclidean_filtering(torch.from_numpy(g["obs"]).to(DEV), torch.from_numpy(g["theta"]).to(DEV),
                                            torch.from_numpy(g["x"]).to(DEV), 100)
    np.testing.assert_array_equal(t.cpu().numpy(), g["standardized_euclidean_filtering_theta"])
    np.testing.assert_array_equal(x.cpu().numpy(), g["standardized_euclidean_filtering_x"])


@pytest.mark.parametrize("method,n", [("rejection", 300), ("sir", 40)])
def test_posterior_support_on_engine(method, n):
    """Reference tests/test_support_posterior.py:14-70 at reduced sizes, on the GPU engine."""
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN
    from npe_pfn.support_posterior import PosteriorSupport

    torch.manual_seed(0)
    prior = torch.distributions.MultivariateNormal(torch.zeros(2, device=DEV), torch.eye(2, device=DEV))
    theta = prior.sample((1000,))
    x = theta + torch.randn_like(theta)
    post = TabPFN_Based_NPE_PFN(prior=prior, filter_type="standardized_euclidean_filtering",
                                regressor_init_kwargs={"random_state": 0, "device": DEV})
    post.append_simulations(theta, x)
    sup = PosteriorSupport(prior, post, torch.zeros(2, device=DEV), num_samples_to_estimate_support=2000,
                           batch_size_for_estimate_support=2000, allowed_false_negatives=0.001,
                           sampling_method=method, oversample_sir=10)
    out = sup.sample((n,), show_progress_bars=False, sampling_batch_size=1000,
                     **({"return_ess": True} if method == "sir" else {}))
    s = out[0] if method == "sir" else out
    assert s.shape == (n, 2)
    assert torch.isfinite(s).all()
    if method == "sir":
        ess = out[1]
        assert ess.shape == (((n + 99) // 100) * 100,)
        assert bool(((ess >= 1.0 - 1e-4) & (ess <= 10.0 + 1e-3)).all())


# =========================================================================== edges
@pytest.fixture(scope="module")
def engine():
    from npe_pfn.engine import Engine

    return Engine(device=DEV)


def _abi():
    import ctypes

    from npe_pfn.engine import _check, _ptr, load_library

    return load_library(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream), _check, _ptr


# --------------------------------------------------------------------------- K12
@pytest.mark.parametrize("n,dim,k,shift", sr.FILTER_SHAPES,
                         ids=[f"{n}x{d}-k{k}" + ("-shift" if s else "") for n, d, k, s in sr.FILTER_SHAPES])
def test_filter_is_the_fp64_rank_within_the_fp32_bound(engine, n, dim, k, shift):
    x, obs = sr.filter_case(n, dim, k, shift)
    idx = engine.filter_stdeuclid(torch.from_numpy(x).to(DEV), torch.from_numpy(obs).to(DEV), k)
    assert idx.dtype == torch.int64 and idx.shape == (k,)
    use = sr.check_filter(idx.cpu().numpy(), x, obs, k)
    print(f"K12 n={n} dim={dim} k={k} shift={shift}: largest rank displacement / bound = {use:.3f}")


@pytest.mark.parametrize("k", [200, 201])
def test_filter_exact_ties_go_to_the_lower_row(engine, k):
    n, dim = 600, 3
    rng = np.random.default_rng(12)
    base = rng.standard_normal((n // 2, dim)).astype(np.float32)
    x = np.concatenate([base, base])
    obs = (0.5 * rng.standard_normal(dim)).astype(np.float32)
    idx = engine.filter_stdeuclid(torch.from_numpy(x).to(DEV), torch.from_numpy(obs).to(DEV), k).cpu().numpy()
    pairs = idx[:200].reshape(100, 2)
    assert np.all(pairs[:, 0] < n // 2), pairs[pairs[:, 0] >= n // 2]
    np.testing.assert_array_equal(pairs[:, 1], pairs[:, 0] + n // 2)  # twin rows adjacent, lower row first
    sr.check_filter(idx, x, obs, k)
    if k == 201:  # the split pair gives its lower row
        assert idx[200] < n // 2 and idx[200] not in set(pairs[:, 0].tolist())


@pytest.mark.parametrize("why", ["constant column", "one NaN cell"])
def test_filter_all_nan_distances_keep_row_order(engine, why):
    n, dim, k = 1000, 3, 300  # 1024 keys: four blocks of the sort
    x = np.random.default_rng(13).standard_normal((n, dim)).astype(np.float32)
    if why == "constant column":
        x[:, 1] = 3.0  # std 0: 0 / 0
    else:
        x[517, 2] = np.nan  # the column's mean is NaN
    obs = np.zeros(dim, np.float32)
    idx = engine.filter_stdeuclid(torch.from_numpy(x).to(DEV), torch.from_numpy(obs).to(DEV), k)
    np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(k))


def test_filter_empty_and_refused_calls(engine):
    from npe_pfn.engine import EngineError

    x = torch.randn(10, 2, device=DEV)
    obs = torch.zeros(2, device=DEV)
    idx = engine.filter_stdeuclid(x, obs, 0)
    assert idx.shape == (0,) and idx.dtype == torch.int64
    with pytest.raises(EngineError, match="k <= n_rows"):
        engine.filter_stdeuclid(x, obs, 11)
    with pytest.raises(EngineError, match="n_rows >= 1"):
        engine.filter_stdeuclid(x[:0], obs, 0)
    with pytest.raises(EngineError, match="dim >= 1"):
        engine.filter_stdeuclid(x[:, :0], obs[:0], 1)


# --------------------------------------------------------------------------- K10
def _masks(n, rng):
    i = np.arange(n)
    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": i == 0, "last": i == n - 1,
           "alternating": i % 2 == 1, "0 mod 64": i % 64 == 0, "63 mod 64": i % 64 == 63}
    for p in (0.01, 0.5, 0.99):
        out[f"random {p}"] = rng.random(n) < p
    return out


SENTINEL = -12345.0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000])
def test_compact_rows_counts_orders_and_leaves_the_rest(n):
    lib, stream, _check, _ptr = _abi()
    rng = np.random.default_rng(n)
    for dim in (1, 3, 10):
        src = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32))
        src_d = src.to(DEV)
        for name, m in _masks(n, rng).items():
            for drawn in (False, True):  # set bytes 1, or any of 1, 2, 128, 255
                byte = rng.choice(np.array([1, 2, 128, 255], np.uint8), n) if drawn else np.ones(n, np.uint8)
                mask = torch.from_numpy(np.where(m, byte, 0).astype(np.uint8)).to(DEV)
                dst = torch.full((n, dim), SENTINEL, device=DEV)
                cnt = torch.full((1,), -1, dtype=torch.int64, device=DEV)
                _check(lib, lib.npfn_compact_rows(_ptr(src_d), _ptr(mask), n, dim, _ptr(dst), _ptr(cnt), stream),
                       "npfn_compact_rows")
                ref = src[torch.from_numpy(m)]
                what = (n, dim, name, drawn)
                assert int(cnt.item()) == ref.shape[0], what
                got = dst.cpu()
                assert torch.equal(got[: ref.shape[0]].view(torch.int32), ref.view(torch.int32)), what
                assert bool((got[ref.shape[0]:] == SENTINEL).all()), what


@pytest.mark.parametrize("dim", [1, 3])
def test_compaction_of_no_rows_is_empty(engine, dim):
    from npe_pfn.support_posterior import box_compact

    empty = torch.empty(0, dim, device=DEV)
    out = engine.compact_rows(empty, torch.empty(0, dtype=torch.bool, device=DEV))
    assert out.shape == (0, dim) and out.dtype == torch.float32
    out = box_compact(empty, -torch.ones(dim, device=DEV), torch.ones(dim, device=DEV))
    assert out.shape == (0, dim) and out.dtype == torch.float32


# --------------------------------------------------------------------------- K9
def _f32(v):
    return np.float32(v)


def test_box_support_closed_bounds_nan_and_zero_signs(engine):
    low = np.array([-1.0, 0.0, 2.0], np.float32)
    high = np.array([1.0, 0.5, 2.0], np.float32)  # column 2: low == high
    inside = np.array([0.25, 0.25, 2.0], np.float32)
    up, down = _f32(np.inf), _f32(-np.inf)
    cells = [(0, low[0], True), (0, high[0], True), (1, low[1], True), (1, high[1], True),
             (0, np.nextafter(low[0], down), False), (0, np.nextafter(high[0], up), False),
             (1, np.nextafter(low[1], down), False), (1, np.nextafter(high[1], up), False),
             (2, np.nextafter(low[2], down), False), (2, np.nextafter(high[2], up), False),
             (1, _f32(-0.0), True),  # -0.0 against the +0.0 bound
             (0, _f32(np.nan), False), (1, _f32(np.nan), False), (2, _f32(np.nan), False),
             (0, up, False), (0, down, False)]
    rows, want = [inside.copy()], [True]
    for j, v, ok in cells:
        r = inside.copy()
        r[j] = v
        rows.append(r)
        want.append(ok)
    theta = np.stack(rows)
    got = engine.box_support(torch.from_numpy(theta), torch.from_numpy(low), torch.from_numpy(high))
    assert got.dtype == torch.bool
    np.testing.assert_array_equal(got.cpu().numpy(), np.array(want))
    np.testing.assert_array_equal(np.array(want), box_mask(theta, low, high))
    # +0.0 against a -0.0 bound
    z = engine.box_support(torch.tensor([[0.0], [-0.0]]), torch.tensor([-0.0]), torch.tensor([-0.0]))
    assert z.cpu().tolist() == [True, True]


def test_box_support_infinite_and_inverted_bounds(engine):
    theta = torch.tensor([[0.0, 1e38], [float("inf"), 0.0], [0.0, -float("inf")], [float("nan"), 0.0],
                          [-3.0e38, 3.0e38]])
    inf = float("inf")
    got = engine.box_support(theta, torch.tensor([-inf, -inf]), torch.tensor([inf, inf]))
    assert got.cpu().tolist() == [True, True, True, False, True]  # only the NaN row is outside
    got = engine.box_support(theta, torch.tensor([-inf, 0.0]), torch.tensor([0.0, inf]))
    assert got.cpu().tolist() == [True, False, False, False, True]
    got = engine.box_support(theta, torch.tensor([1.0, -inf]), torch.tensor([-1.0, inf]))  # low > high
    assert not got.any()
    got = engine.box_support(theta, torch.tensor(1.0), torch.tensor(-1.0))
    assert not got.any()


@pytest.mark.parametrize("dim", [1, 3, 10])
def test_box_support_scalar_bounds_broadcast(engine, dim):
    rng = np.random.default_rng(dim)
    for n in (255, 256, 257, 0):
        theta = rng.standard_normal((n, dim)).astype(np.float32)
        got = engine.box_support(torch.from_numpy(theta), torch.tensor(-1.5), torch.tensor(2.0))
        assert got.shape == (n,) and got.dtype == torch.bool
        ref = box_mask(theta, np.float32(-1.5), np.float32(2.0))  # 0.91 per cell: 0.39 of the rows at dim 10
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
        assert n == 0 or 0 < ref.sum() < n


# --------------------------------------------------------------------------- K11
NEVER = torch.tensor(-3.0e38)  # a threshold that truncates nothing


def _exact_groups():
    """Groups of k = 130 whose pick and ESS involve no rounding -> (lpr, lq, [(indices with
    mass, ess)], k).  Every ratio that is not named is -FLT_MAX after the clip (lpr = -inf with
    finite lq), so its exp against any finite maximum is exactly 0."""
    k = 130
    lpr_rows, lq_rows, want = [], [], []

    def group(masses):
        lpr = torch.full((k,), -float("inf"))
        lq = torch.zeros(k)
        for i, (a, b) in masses.items():
            lpr[i], lq[i] = a, b
        lpr_rows.append(lpr)
        lq_rows.append(lq)

    for p in (0, 63, 64, k - 1):  # one proposal carries all the mass: the pick for every u
        for _ in range(6):
            group({p: (0.5, -1.0)})
            want.append(((p,), 1.0))
    for i, j in ((0, k - 1), (63, 64), (64, 65), (5, 70), (0, 1), (127, 128)):  # two equal masses
        for _ in range(6):
            group({i: (1.0, 1.0), j: (1.0, 1.0)})
            want.append(((i, j), 2.0))
    for p in (0, 64, k - 1):  # lpr = +inf with finite lq wins outright against finite ratios
        lpr = torch.linspace(-1, 1, k)
        lpr[p] = float("inf")
        lpr_rows.append(lpr)
        lq_rows.append(torch.zeros(k))
        want.append(((p,), 1.0))
    return torch.cat(lpr_rows), torch.cat(lq_rows), want, k


def test_sir_select_exact_groups():
    from npe_pfn.support_posterior import sir_select

    lpr, lq, want, k = _exact_groups()
    G = len(want)
    th = torch.arange(G * k, dtype=torch.float32)[:, None]
    _, pick, ess = sir_select(th.to(DEV), lpr.to(DEV), lq.to(DEV), NEVER.to(DEV), k, seed=7, counter=3)
    pick, ess = pick.cpu().numpy(), ess.cpu().numpy()
    u = uniforms(7, 3, G)
    lower = 0
    for g, (where, e) in enumerate(want):
        expect = where[0] if len(where) == 1 or u[g] < 0.5 else where[1]
        lower += len(where) == 2 and u[g] < 0.5
        assert pick[g] == expect, (g, where, float(u[g]), int(pick[g]))
        assert ess[g] == e, (g, where, float(ess[g]))
    assert 0 < lower < 36  # both halves of the two-mass groups were drawn
    ref_pick, ref_ess = oracle_sir(lpr.numpy(), lq.numpy(), float(NEVER), k, seed=7, counter=3)
    np.testing.assert_array_equal(pick, ref_pick)
    np.testing.assert_array_equal(ess, ref_ess)


def test_sir_select_threshold_is_strict():
    from npe_pfn.support_posterior import sir_select

    k, G = 130, 8
    thr = torch.tensor(0.7)
    below = torch.nextafter(thr, torch.tensor(-1.0))
    lq = below.repeat(G * k)
    keep = torch.arange(G) * k + torch.tensor([0, 1, 63, 64, 65, 100, 128, 129])
    lq[keep] = thr  # lq == thr is kept, the float below it is truncated
    lpr = torch.zeros(G * k)
    th = torch.arange(G * k, dtype=torch.float32)[:, None]
    sel, pick, ess = sir_select(th.to(DEV), lpr.to(DEV), lq.to(DEV), thr.to(DEV), k, seed=2)
    np.testing.assert_array_equal(pick.cpu().numpy() + np.arange(G) * k, keep.numpy())
    assert ess.cpu().tolist() == [1.0] * G
    np.testing.assert_array_equal(sel.cpu().numpy()[:, 0], keep.numpy().astype(np.float32))


@pytest.mark.parametrize("width", [1, 64, 65, 130])
def test_sir_select_gathers_every_column(width):
    from npe_pfn.support_posterior import sir_select

    G, k = 9, 65
    th, lpr, lq, thr = sr.sir_case(G, k, seed=width, width=width)
    sel, pick, _ = sir_select(th.to(DEV), lpr.to(DEV), lq.to(DEV), thr.to(DEV), k, seed=4, counter=1)
    assert sel.shape == (G, width)
    ref = th.reshape(G, k, width)[torch.arange(G), pick.cpu()]
    assert torch.equal(sel.cpu().view(torch.int32), ref.view(torch.int32))
    ref_pick, _ = oracle_sir(lpr.numpy(), lq.numpy(), float(thr), k, seed=4, counter=1)
    np.testing.assert_array_equal(pick.cpu().numpy(), ref_pick)


def _sir_abi(th, lpr, lq, thr, G, k, offset, seed=31, counter=2):
    lib, stream, _check, _ptr = _abi()
    D = th.shape[1]
    pick = torch.full((G,), -1, dtype=torch.int64, device=DEV)
    ess = torch.full((G,), -1.0, device=DEV)
    out = torch.full((G, D), SENTINEL, device=DEV)
    _check(lib, lib.npfn_sir_select(_ptr(lpr), _ptr(lq), _ptr(thr), G, k, seed, counter, offset, _ptr(th), D,
                                    _ptr(pick), _ptr(ess), _ptr(out), stream), "npfn_sir_select")
    return pick, ess, out


def test_sir_select_group_offset_splits_a_call():
    G, k = 10, 65
    th, lpr, lq, thr = (t.to(DEV).contiguous() for t in sr.sir_case(G, k, seed=5))
    thr = thr.reshape(1)
    whole = _sir_abi(th, lpr, lq, thr, G, k, 0)
    h = G // 2
    first = _sir_abi(th[: h * k], lpr[: h * k], lq[: h * k], thr, h, k, 0)
    second = _sir_abi(th[h * k:], lpr[h * k:], lq[h * k:], thr, G - h, k, h)
    for w, a, b in zip(whole, first, second):
        assert torch.equal(w, torch.cat([a, b]))
    assert bool(torch.isfinite(whole[1]).all())
    ref_pick, _ = oracle_sir(lpr.cpu().numpy(), lq.cpu().numpy(), float(thr), k, seed=31, counter=2)
    np.testing.assert_array_equal(whole[0].cpu().numpy(), ref_pick)
    # the offset matters: the second half at offset 0 draws the first half's uniforms
    u = uniforms(31, 2, G)
    assert not np.array_equal(u[:h], u[h:])


def test_sir_select_no_groups_is_a_no_op():
    from npe_pfn.support_posterior import sir_select

    e = torch.empty(0, device=DEV)
    sel, pick, ess = sir_select(torch.empty(0, 3, device=DEV), e, e, torch.tensor(0.0, device=DEV), 5, seed=1)
    assert sel.shape == (0, 3) and pick.shape == (0,) and ess.shape == (0,)
    assert pick.dtype == torch.int64
