"""Pair marginals on the CPU: PosteriorPairMarginals' arithmetic on hand-made 2 x 2 and 3 x 3 tables,
pair_accumulate_host on hand-made rows, NPE_PFN_Core.pair_marginals through the generic dimension
loop with a stub regressor whose step-1 predictive depends on the step-0 draw in a known way, the
unconditional estimator's mix, and the C ABI of the three new entry points.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from test_abi import declared_functions, declared_prototypes

Q40 = 2 ** 40


def _ppm(table, edges, cell=None):
    """One observation, two parameters: ``table`` [G, G] is pair (0, 1)."""
    from npe_pfn.pair_marginals import PosteriorPairMarginals

    t = torch.tensor(table, dtype=torch.float32)
    cell = torch.stack([t.sum(1), t.sum(0)]) if cell is None else torch.tensor(cell, dtype=torch.float32)
    return PosteriorPairMarginals(t[None, None], cell[None], torch.tensor(edges, dtype=torch.float32), num_draws=1)


# ------------------------------------------------------------- hand-made tables
def test_orientation_and_density_2x2():
    """Cells of dim 0: [0, 1), [1, 3); of dim 1: [0, 2), [2, 3)."""
    pm = _ppm([[0.1, 0.2], [0.3, 0.4]], [[0.0, 1.0, 3.0], [0.0, 2.0, 3.0]])
    assert pm.num_observations == 1 and pm.dim_theta == 2 and pm.bins == 2
    p01, p10 = pm.pair(0, 1), pm.pair(1, 0)
    assert p01.shape == (1, 2, 2)
    assert p01[0, 1, 0].item() == pytest.approx(0.3) and p10[0, 0, 1].item() == pytest.approx(0.3)
    assert torch.equal(p10, p01.transpose(-1, -2))
    # density = mass / area: areas [[1*2, 1*1], [2*2, 2*1]]
    np.testing.assert_allclose(pm.density(0, 1)[0].numpy(), [[0.05, 0.2], [0.075, 0.2]], atol=1e-8)
    np.testing.assert_allclose(pm.density(1, 0)[0].numpy(), [[0.05, 0.075], [0.2, 0.2]], atol=1e-8)
    assert pm.mass_inside(0, 1).item() == pytest.approx(1.0, abs=1e-7)
    with pytest.raises(ValueError):
        pm.pair(0, 0)
    with pytest.raises(ValueError):
        pm.pair(0, 2)


def test_credible_region_splits_two_cells():
    """Unit cells, masses .5 / .3 / .15 / .05: the densest cell alone holds 50 %, so a level just
    below 0.5 is that cell and one just above needs the second (the masses are fp32 values: a level
    of exactly 0.5 would test their rounding); mass outside the limits does not count."""
    pm = _ppm([[0.5, 0.05], [0.15, 0.3]], [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]])
    assert pm.credible_region(0, 1, 0.49)[0].tolist() == [[True, False], [False, False]]
    assert pm.credible_region(0, 1, 0.51)[0].tolist() == [[True, False], [False, True]]
    assert pm.credible_region(0, 1, 0.79)[0].tolist() == [[True, False], [False, True]]
    assert pm.credible_region(0, 1, 0.81)[0].tolist() == [[True, False], [True, True]]
    assert pm.credible_region(0, 1, 1.0)[0].all()
    assert pm.credible_region(1, 0, 0.81)[0].tolist() == [[True, True], [False, True]]
    # half of the mass outside the limits: the levels are shares of what is inside
    half = _ppm([[0.25, 0.025], [0.075, 0.15]], [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]])
    assert half.mass_inside(0, 1).item() == pytest.approx(0.5, abs=1e-7)
    assert half.credible_region(0, 1, 0.51)[0].tolist() == [[True, False], [False, True]]
    # density, not mass, orders the cells: a wide cell with more mass but less density comes later
    wide = _ppm([[0.4, 0.0], [0.6, 0.0]], [[0.0, 1.0, 11.0], [0.0, 1.0, 2.0]])
    assert wide.credible_region(0, 1, 0.3)[0].tolist() == [[True, False], [False, False]]
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            pm.credible_region(0, 1, bad)


def test_correlation_3x3():
    edges = [[0.0, 1.0, 2.0, 3.0], [10.0, 12.0, 14.0, 16.0]]
    diag = _ppm([[0.2, 0, 0], [0, 0.5, 0], [0, 0, 0.3]], edges)
    c = diag.correlation()
    assert c.shape == (1, 2, 2) and c.dtype == torch.float64
    np.testing.assert_allclose(c[0].numpy(), [[1.0, 1.0], [1.0, 1.0]], atol=1e-12)
    anti = _ppm([[0, 0, 0.2], [0, 0.5, 0], [0.3, 0, 0]], edges)
    assert anti.correlation()[0, 0, 1].item() == pytest.approx(-1.0, abs=1e-12)
    indep = _ppm(np.outer([0.2, 0.5, 0.3], [0.1, 0.6, 0.3]).tolist(), edges)
    assert abs(indep.correlation()[0, 0, 1].item()) <= 1e-7


def test_constructor_refuses_bad_shapes():
    from npe_pfn.pair_marginals import PosteriorPairMarginals, grid_edges

    e = grid_edges(torch.tensor([[0.0, 1.0]] * 3), 4)
    assert e.shape == (3, 5) and e.dtype == torch.float32
    PosteriorPairMarginals(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4), e, 1)
    with pytest.raises(ValueError):
        PosteriorPairMarginals(torch.zeros(2, 2, 4, 4), torch.zeros(2, 3, 4), e, 1)       # 3 pairs for d = 3
    with pytest.raises(ValueError):
        PosteriorPairMarginals(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4), e[:, :4], 1)
    with pytest.raises(ValueError):
        PosteriorPairMarginals(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4), e.flip(1), 1)   # decreasing edges


def test_grid_edges():
    from npe_pfn.pair_marginals import grid_edges

    e = grid_edges([[-1.0, 2.0], [0.1, 0.7]], 3)
    assert e[0].tolist() == [-1.0, 0.0, 1.0, 2.0]
    assert e[1, -1].item() == np.float32(0.7) and e[1, 0].item() == np.float32(0.1)   # the last edge is hi itself
    want = (np.float64(0.1) + (np.float64(0.7) - np.float64(0.1)) * np.arange(4) / 3).astype(np.float32)
    assert e[1, :3].tolist() == want[:3].tolist()
    for bad_bins in (1, 129, 0):
        with pytest.raises(ValueError):
            grid_edges([[0.0, 1.0]], bad_bins)
    for lim in ([[0.0, 0.0]], [[1.0, 0.0]], [[0.0, float("inf")]], [[float("nan"), 1.0]], [[1.0, 1.0 + 1e-7]],
                [0.0, 1.0]):
        with pytest.raises(ValueError):
            grid_edges(lim, 8)


# ------------------------------------------------------------- pair_accumulate_host
def _tables(U, n_prev, G):
    return (torch.zeros((U, n_prev, G, G), dtype=torch.int64), torch.zeros((U, G), dtype=torch.int64),
            torch.zeros(U, dtype=torch.int32))


def test_accumulate_cells_of_the_draws():
    """G = 2, edges [0, 1, 2]: a draw on an edge goes to the upper cell; at edges[G], below
    edges[0] or NaN it has no cell; the masses still reach cellQ."""
    from npe_pfn.pair_marginals import pair_accumulate_host

    edges = torch.tensor([[0.0, 1.0, 2.0]])
    theta = torch.tensor([[0.0], [0.5], [1.0], [1.999], [2.0], [-1e-6], [float("nan")], [float("inf")]])
    w = torch.tensor([[0.25, 0.75]] * 8, dtype=torch.float64)
    pairQ, cellQ, bad = _tables(1, 1, 2)
    pair_accumulate_host(w, theta, edges, 0, 8, pairQ, cellQ, bad)
    q = torch.tensor([Q40 // 4, 3 * Q40 // 4])
    assert torch.equal(pairQ[0, 0, 0], 2 * q)       # rows 0, 1: cell 0
    assert torch.equal(pairQ[0, 0, 1], 2 * q)       # rows 2 (on the edge 1.0: the upper cell), 3
    assert torch.equal(cellQ[0], 8 * q) and bad.tolist() == [0]
    # the identity: sum_a pairQ + (q of the rows without a cell) == cellQ, exactly
    assert torch.equal(pairQ[0, 0].sum(0) + 4 * q, cellQ[0])


def test_accumulate_identity_rounding_nan_rows_and_windows():
    from npe_pfn.pair_marginals import pair_accumulate_host

    g = torch.Generator().manual_seed(3)
    U, per, n_prev, G = 3, 7, 2, 5
    n = U * per
    w = torch.rand((n, G), generator=g, dtype=torch.float64)
    w = w / w.sum(1, keepdim=True)
    w[0, 0] = 0.5 / Q40            # a tie: half to even -> 0
    w[0, 1] = 1.5 / Q40            # -> 2
    w[9, 3] = float("nan")         # row 9 (observation 1): bad, adds nothing
    theta = torch.rand((n, 3), generator=g) * 1.4 - 0.2          # some draws outside [0, 1)
    edges = torch.linspace(0, 1, G + 1)[None].repeat(n_prev, 1).contiguous()
    pairQ, cellQ, bad = _tables(U, n_prev, G)
    pair_accumulate_host(w, theta, edges, 0, per, pairQ, cellQ, bad)
    assert bad.tolist() == [0, 1, 0]
    q = torch.round(torch.nan_to_num(w) * Q40).to(torch.int64)
    q[9] = 0
    assert q[0, 0].item() == 0 and q[0, 1].item() == 2
    outside = (theta[:, :n_prev] < 0) | (theta[:, :n_prev] >= 1)
    assert 0 < int(outside.sum()) < outside.numel()               # some draws have no cell, not all
    for u in range(U):
        rows = slice(u * per, (u + 1) * per)
        assert torch.equal(cellQ[u], q[rows].sum(0))
        for j in range(n_prev):
            th = theta[rows, j]
            inside = (th >= 0) & (th < 1)
            assert torch.equal(pairQ[u, j].sum(0) + q[rows][~inside].sum(0), cellQ[u]), (u, j)
            a = (th[inside][:, None] >= edges[j][None, :]).sum(1) - 1       # the edges at or below the draw
            want = torch.zeros((G, G), dtype=torch.int64).index_add_(0, a, q[rows][inside])
            assert torch.equal(pairQ[u, j], want)
    # the same rows in three windows that ignore the observations' boundaries, out of order
    p2, c2, b2 = _tables(U, n_prev, G)
    for lo, hi in ((10, 21), (0, 4), (4, 10)):
        pair_accumulate_host(w[lo:hi], theta[lo:hi], edges, lo, per, p2, c2, b2)
    assert torch.equal(p2, pairQ) and torch.equal(c2, cellQ) and torch.equal(b2, bad)
    # n_prev = 0: only the cell sums
    p0, c0, b0 = _tables(U, 0, G)
    pair_accumulate_host(w, None, None, 0, per, p0, c0, b0)
    assert torch.equal(c0, cellQ) and torch.equal(b0, bad)


def test_accumulate_refuses_bad_arguments():
    from npe_pfn.pair_marginals import pair_accumulate_host

    w = torch.zeros((4, 2), dtype=torch.float64)
    th, ed = torch.zeros((4, 1)), torch.tensor([[0.0, 1.0, 2.0]])
    pairQ, cellQ, bad = _tables(2, 1, 2)
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th, None, 0, 2, pairQ, cellQ, bad)
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th, ed, 0, 0, pairQ, cellQ, bad)
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th, ed, 0, 2 ** 22 + 1, pairQ, cellQ, bad)
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th, ed, 2, 2, pairQ, cellQ, bad)              # rows 2..5: observation 2 of 2
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th, ed, 0, 2, pairQ.to(torch.int32), cellQ, bad)
    with pytest.raises(ValueError):
        pair_accumulate_host(w, th[:3], ed, 0, 2, pairQ, cellQ, bad)


# ------------------------------------------------------------- pair_marginals() with a stub regressor
NB = 8                     # borders -4 .. 4: bars 1..6 are the unit cells of the grid [-3, 3] x 6
LIMITS = [[-3.0, 3.0], [-3.0, 3.0]]
STEP1_SAME, STEP1_NEXT = 0.75, 0.25


class StubCriterion:
    def __init__(self, borders, draws):
        self.borders = borders
        self._draws = draws

    def sample(self, logits):
        return self._draws


class StubRegressor:
    """tabpfn's fit / predict surface with known predictive distributions on the bars [-4, 4] x 8
    (no mass in the two tail bars).  Step 0: masses .25 / .5 / .25 on three neighbouring bars
    around one chosen by the context's mean target; row i 'draws' the centre of bar lo + i % 3.
    Step 1: row i puts 0.75 on the bar of its own step-0 draw and 0.25 on the next one (cyclic
    in the bars 1..6), and draws the centre of its step-0 bar."""

    def __init__(self, **kwargs):
        self.F = None
        self.centre = None

    def fit(self, X, y):
        self.F = X.shape[1]
        self.centre = int(torch.clamp(torch.round(y.double().mean()), -2, 1).item()) + 4   # a bar in 2..5
        return self

    def predict(self, X, output_type="full", quantiles=None):
        assert output_type == "full" and X.shape[1] == self.F
        n = X.shape[0]
        borders = torch.linspace(-4.0, 4.0, NB + 1)
        p = torch.zeros((n, NB), dtype=torch.float64)
        i = torch.arange(n)
        if self.F == 1:                    # step 0 (dx = 1)
            p[:, self.centre - 1], p[:, self.centre], p[:, self.centre + 1] = 0.25, 0.5, 0.25
            bar = self.centre - 1 + i % 3
        else:
            bar = torch.floor(X[:, 1]).long() + 4          # the bar of the step-0 draw
            p[i, bar] = STEP1_SAME
            p[i, (bar - 1 + 1) % 6 + 1] = STEP1_NEXT
        draws = (borders[bar] + borders[bar + 1]) / 2
        return {"logits": torch.log(p).to(torch.float32), "criterion": StubCriterion(borders, draws)}


@pytest.fixture()
def stub_core(monkeypatch):
    import npe_pfn.npe_pfn as mod

    monkeypatch.setattr(mod, "TabPFNRegressor", StubRegressor)
    rng = np.random.default_rng(5)
    theta = torch.from_numpy(rng.normal(size=(20, 2)).astype(np.float32))
    x = torch.from_numpy(rng.normal(size=(20, 1)).astype(np.float32))
    core = mod.NPE_PFN_Core(prior=None)
    core.append_simulations(theta, x)
    return core, theta, x


def _analytic(samples):
    """The tables the stub implies, from the draws alone: ([M, G, G] pair (0, 1), [M, G] cells of
    dim 1), G = 6, cell = bar - 1."""
    M, n, _ = samples.shape
    a = torch.floor(samples[:, :, 0]).long() + 3
    pair = torch.zeros((M, 6, 6), dtype=torch.float64)
    for m in range(M):
        for ai in a[m].tolist():
            pair[m, ai, ai] += STEP1_SAME / n
            pair[m, ai, (ai + 1) % 6] += STEP1_NEXT / n
    return pair, pair.sum(1)


@pytest.mark.parametrize("n_obs,num_draws,cap,n_calls", [
    (1, 7, 3, 3),            # one observation, an unequal last call: 3 + 3 + 1
    (1, 5, 10_000, 1),       # one call
    (2, 5, 4, 3),            # two observations: 4 // 2 = 2 draws each per call, 2 + 2 + 1
])
def test_pair_marginals_through_the_generic_loop(stub_core, n_obs, num_draws, cap, n_calls):
    core, theta, x = stub_core
    pm = core.pair_marginals(x[:n_obs], num_draws=num_draws, bins=6, limits=LIMITS, max_sampling_batch_size=cap,
                             return_samples=True)
    assert pm.probs.shape == (n_obs, 1, 6, 6) and pm.probs.dtype == torch.float32
    assert pm.marginal_probs.shape == (n_obs, 2, 6) and pm.edges.shape == (2, 7) and pm.num_draws == num_draws
    assert pm.edges[0].tolist() == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    assert pm.samples.shape == (n_obs, num_draws, 2)
    want_pair, want_cell1 = _analytic(pm.samples)
    # fp64 sums of 2^-40-quantised masses, rounded to fp32 per call and combined: far below 1e-7
    np.testing.assert_allclose(pm.pair(0, 1).double().numpy(), want_pair.numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(pm.marginal_probs[:, 1].double().numpy(), want_cell1.numpy(), rtol=0, atol=1e-7)
    c = int(torch.clamp(torch.round(theta[:, 0].double().mean()), -2, 1).item()) + 4   # the stub's step-0 bar
    cell0 = torch.zeros(6, dtype=torch.float64)
    cell0[c - 2], cell0[c - 1], cell0[c] = 0.25, 0.5, 0.25
    np.testing.assert_allclose(pm.marginal_probs[:, 0].double().numpy(), cell0[None].repeat(n_obs, 1).numpy(), atol=1e-7)
    # the draws cover more than one cell, so the table is not a single spike
    assert int((pm.pair(0, 1)[0] > 0).sum()) >= 4 or num_draws < 3
    assert pm.mass_inside(0, 1).numpy() == pytest.approx(1.0, abs=1e-6)
    assert torch.equal(pm.pair(1, 0), pm.pair(0, 1).transpose(-1, -2))


def test_default_limits_and_bad_arguments(stub_core):
    core, theta, x = stub_core
    pm = core.pair_marginals(x[0], num_draws=3, bins=4)                     # no prior: the context's min / max
    assert pm.edges[:, 0].tolist() == theta.min(0).values.tolist()
    assert pm.edges[:, -1].tolist() == theta.max(0).values.tolist()
    assert pm.samples is None and pm.probs.shape == (1, 1, 4, 4)
    low, high = torch.tensor([-3.0, -2.0]), torch.tensor([3.0, 2.5])
    core.prior = torch.distributions.Independent(torch.distributions.Uniform(low, high), 1)
    pm = core.pair_marginals(x[0], num_draws=3, bins=4)                     # a box prior: its bounds
    assert pm.edges[:, 0].tolist() == low.tolist() and pm.edges[:, -1].tolist() == high.tolist()
    for kw in ({"num_draws": 0}, {"max_sampling_batch_size": 0}, {"bins": 1}, {"bins": 129},
               {"limits": [[0.0, 1.0]]}, {"limits": [[0.0, 1.0], [2.0, 2.0]]},
               {"limits": [[0.0, 1.0], [0.0, float("inf")]]}):
        with pytest.raises(ValueError):
            core.pair_marginals(x[0], **{"num_draws": 3, **kw})


def test_unconditional_estimator_mixes_its_clusters(monkeypatch):
    import npe_pfn.npe_pfn as mod

    monkeypatch.setattr(mod, "TabPFNRegressor", StubRegressor)
    rng = np.random.default_rng(11)
    theta = np.concatenate([rng.normal(-2.0, 0.1, size=(8, 2)), rng.normal(1.0, 0.1, size=(12, 2))]).astype(np.float32)
    torch.manual_seed(0)
    est = mod.TabPFN_Based_Uncond_Estimator(num_clusters=2)
    est.append_simulations(torch.from_numpy(theta))
    assert sorted(est.counts.tolist()) == [8, 12]
    pm = est.pair_marginals(num_draws=6, bins=6, limits=LIMITS, return_samples=True)
    assert pm.probs.shape == (1, 1, 6, 6) and pm.marginal_probs.shape == (1, 2, 6) and pm.num_draws == 6
    assert pm.samples.shape == (1, 12, 2) and est.cluster_state == 0
    per_cluster = []
    for c in range(2):
        est.set_cluster_state(c)
        per_cluster.append(mod.NPE_PFN_Core.pair_marginals(est, torch.zeros(1, 1), num_draws=6, bins=6, limits=LIMITS))
    est.set_cluster_state()
    assert (per_cluster[0].marginal_probs - per_cluster[1].marginal_probs).abs().max() > 0.2   # the clusters differ
    wts = est.counts / est.counts.sum()
    for name in ("probs", "marginal_probs"):
        want = sum(float(wts[c]) * getattr(per_cluster[c], name).double() for c in range(2))
        np.testing.assert_allclose(getattr(pm, name).double().numpy(), want.numpy(), rtol=0, atol=1e-7)
    # default limits: the min / max of ALL thetas, not of one cluster
    e = est.pair_marginals(num_draws=2, bins=4).edges
    assert e[:, 0].tolist() == theta.min(0).tolist() and e[:, -1].tolist() == theta.max(0).tolist()


def test_process_groups_of_more_than_one_rank_are_refused(stub_core, monkeypatch):
    import npe_pfn.distributed as nd

    core, _, x = stub_core
    pm = nd.pair_marginals_single_rank(core, x[:1], num_draws=2, bins=6, limits=LIMITS)    # no group: one rank
    assert pm.probs.shape == (1, 1, 6, 6)
    monkeypatch.setattr(nd, "_rank_world", lambda group=None: (0, 2))
    with pytest.raises(NotImplementedError, match="2 ranks"):
        nd.pair_marginals_single_rank(core, x[:1], num_draws=2)


def test_package_exports():
    import npe_pfn

    assert "PosteriorPairMarginals" in npe_pfn.__all__
    assert npe_pfn.PosteriorPairMarginals is npe_pfn.pair_marginals.PosteriorPairMarginals


# ------------------------------------------------------------- the C ABI
def test_library_exports_and_signatures():
    from npe_pfn.engine import SIGNATURES, load_library

    lib = load_library()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    want = {
        "npfn_bar_cell_mass": [vp, vp, i64, i32, vp, i32, vp, vp],
        "npfn_pair_accumulate": [vp, vp, i64, i32, vp, i32, i64, i64, i64, vp, vp, ctypes.POINTER(i32), vp],
    }
    rep = SIGNATURES["npfn_ar_sample_repeated"][1]
    # npfn_ar_marginals' arguments up to eps, then edges, n_cells, pair_out, cell_out and the stream
    want["npfn_ar_pair_marginals"] = rep[:-1] + [vp, i32, vp, vp] + rep[-1:]
    protos = declared_prototypes()
    for name, args in want.items():
        assert name in declared_functions()
        assert hasattr(lib, name), f"{name} is not exported by libnpfn.so"
        assert SIGNATURES[name][1] == args, name
        assert len(protos[name]) == len(args)
        assert "double" not in protos[name], f"{name} takes a double by value"


def test_bad_arguments_are_refused_before_any_launch():
    """Every check below is made on the host before a launch or the engine is looked at: no device
    is touched (the pointers are host buffers, the engine handle is NULL)."""
    from npe_pfn.engine import load_library

    lib = load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int32))

    def mass(n_bars=8, n_cells=4, probs=p, n_rows=1):
        return lib.npfn_bar_cell_mass(probs, p, n_rows, n_bars, p, n_cells, p, None)

    assert mass(n_cells=1) == -1 and b"bar_cell_mass" in lib.npfn_last_error()
    assert mass(n_cells=129) == -1
    assert mass(n_bars=1) == -1
    assert mass(n_bars=1 << 20) == -1                    # more bars than a workgroup's LDS holds
    assert mass(n_rows=-1) == -1
    assert mass(probs=None) == -1
    assert mass(n_rows=0) == 0                           # nothing to do, nothing launched

    def acc(w=p, n_prev=1, n_cells=4, r0=0, n_rows=1, per=1, pairQ=p, ldt=1):
        return lib.npfn_pair_accumulate(w, p, ldt, n_prev, p, n_cells, r0, n_rows, per, pairQ, p, bad, None)

    assert acc(n_cells=1) == -1 and b"pair_accumulate" in lib.npfn_last_error()
    assert acc(n_cells=129) == -1
    assert acc(per=(1 << 22) + 1) == -1 and b"2^22" in lib.npfn_last_error()
    assert acc(per=0) == -1
    assert acc(r0=-1) == -1
    assert acc(n_prev=2, ldt=1) == -1                    # fewer columns than earlier dimensions
    assert acc(w=None) == -1
    assert acc(pairQ=None) == -1
    assert acc(n_rows=0) == 0

    def fused(n_unique=2, n_rows=4, n_cells=4, edges=p, pair=p, cell=p, dim_theta=2):
        return lib.npfn_ar_pair_marginals(None, None, None, 4, 1, dim_theta, None, n_unique, n_rows, 0, 0, None, None,
                                          1e-15, edges, n_cells, pair, cell, None)

    assert fused(n_unique=0) == -1 and b"ar_pair_marginals" in lib.npfn_last_error()
    assert fused(n_unique=3) == -1                       # 3 does not divide 4
    assert fused(n_rows=0) == -1
    assert fused(n_cells=1) == -1
    assert fused(n_cells=129) == -1
    assert fused(n_unique=1, n_rows=(1 << 22) + 1) == -1 and b"2^22" in lib.npfn_last_error()
    assert fused(edges=None) == -1
    assert fused(cell=None) == -1
    assert fused(pair=None) == -1
    assert fused(pair=None, dim_theta=1) == -1           # one parameter has no pairs: this reaches the engine check
    assert b"null engine" in lib.npfn_last_error()
    assert fused() == -1 and b"null engine" in lib.npfn_last_error()
