"""GPU: pair marginals -- npfn_bar_cell_mass, npfn_pair_accumulate and the fused
npfn_ar_pair_marginals, up to NPE_PFN_Core.pair_marginals.

The fused tests use the shapes of tests/test_gpu_marginals.py: 150 context rows, dim_x = 3,
dim_theta = 3, preprocessing "none" and "ensemble", synthetic weights (seed 0); 3 observations x 50
draws = 150 rows.  Everything they read is computed once per mode (fixture ``runs``), the unfused
reference included.
"""
import json
import os

import numpy as np
import pytest
import torch

from pair_marginals_ref import cell_mass_ref, pair_index
from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
N_CTX, DX, DTH = 150, 3, 3
M_OBS, PER = 3, 50
N = M_OBS * PER
SEED = 2
COUNTER = 5
BINS = 16
DEV = torch.device("cuda", 0)
# Both sides of the npfn_bar_cell_mass comparison are fp64 and differ in summation order only:
# 5000 adds x 1.1e-16 on values <= 1 is about 6e-13, in two prefixes and a division; about 10x margin
W_BOUND = 1e-11
# A cell mass is the difference of two cumulative sums, each within CUM_BOUND = 2e-5 of the unfused
# route (tests/test_gpu_marginals.py); a mean over rows keeps the bound
CELL_BOUND = 4e-5
# NPFN_PAIR_MARGINALS_PARITY_OUT=<file>: test_fused_matches_the_unfused_route also records its maxima
# there (profiles/pair_marginals/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_PAIR_MARGINALS_PARITY_OUT")
_parity = {}


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(CFG, seed=0)


@pytest.fixture(scope="module")
def eng(weights):
    from npe_pfn.engine import Engine

    return Engine(CFG, weights, device=DEV, random_state=SEED, preprocessing="none")


# ------------------------------------------------------------------ npfn_bar_cell_mass
def _mass_case(nb, G, beyond):
    """Borders with a zero-width bar, rows of random masses plus a one-hot row, a zero-mass row and
    a row with an infinite total; edges whose second one IS a bar border (and, from G = 5 on, the
    border of the zero-width bar too), the outermost ones inside the half-normal end bars
    (``beyond`` False) or beyond every border (True)."""
    g = torch.Generator().manual_seed(nb * 131 + G)
    b = torch.cumsum(torch.rand(nb + 1, generator=g) + 0.01, 0) - 0.3 * nb
    z = nb // 2
    b[z + 1] = b[z]                                      # bar z has width 0
    b = b.to(torch.float32)
    p = torch.rand((6, nb), generator=g)
    p[1] = 0.0
    p[1, nb // 3] = 2.5                                  # one-hot
    p[2] = 0.0                                           # no mass: a NaN row
    p[3, 7] = float("inf")                               # an infinite total: a NaN row
    p[4, :z] = 0.0                                       # all mass right of the zero-width bar
    p[5] *= 1e-3                                         # unnormalised, far from 1
    if beyond:
        lo, hi = b[0] - 3.0, b[-1] + 5.0
    else:
        lo, hi = (b[0] + b[1]) / 2, (b[-2] + b[-1]) / 2
    inner = torch.sort(torch.rand(G - 1, generator=g) * (b[-2] - b[1]) + b[1]).values
    inner[0] = b[nb // 4]                                # an edge equal to a bar border
    if G >= 5:
        inner[G // 2] = b[z]                             # ... and equal to the doubled border
    e = torch.cat([lo[None], torch.sort(inner).values, hi[None]]).to(torch.float32)
    assert bool((e[1:] > e[:-1]).all())
    return p, b, e


@pytest.mark.parametrize("beyond", [False, True])
@pytest.mark.parametrize("nb,G", [(5000, 2), (5000, 5), (5000, 64), (5000, 128), (300, 5), (100, 64)])
def test_bar_cell_mass_against_the_fp64_restatement(eng, nb, G, beyond):
    p, b, e = (t.to(DEV) for t in _mass_case(nb, G, beyond))
    w = eng.bar_cell_mass(p, b, e)
    ref = cell_mass_ref(p, b, e)
    assert w.shape == (6, G) and w.dtype == torch.float64 and w.is_cuda
    assert torch.isnan(w[2]).all() and torch.isnan(w[3]).all() and torch.isnan(ref[2]).all()
    ok = [0, 1, 4, 5]
    gap = (w[ok] - ref[ok]).abs().max().item()
    print(f"nb {nb} G {G} beyond {beyond}: max |w - w_ref| = {gap:.3e}; row sums {w[ok].sum(1).tolist()}")
    assert gap <= W_BOUND, gap
    assert bool((w[ok] >= 0).all())
    # the one-hot row: its bar lies inside the grid, so all of its mass is in the cells
    assert w[1].sum().item() == pytest.approx(1.0, abs=1e-12)
    if beyond:   # the grid holds (almost) everything: the half-normal tails beyond +-3 / 5 widths aside
        assert (w[ok].sum(1) - 1).abs().max().item() <= 1e-3


# ------------------------------------------------------------------ npfn_pair_accumulate
def _acc_inputs(eng, n, n_prev, G, seed, nan_rows=()):
    """The device's own w (npfn_bar_cell_mass of random 64-bar rows) and draws that cover every
    kind of position: inside, on an edge, at the last edge, below the first, NaN."""
    g = torch.Generator().manual_seed(seed)
    nb = 64
    p = torch.rand((n, nb), generator=g)
    for r in nan_rows:
        p[r] = 0.0
    b = torch.linspace(-4.0, 4.0, nb + 1)
    edges = torch.stack([torch.linspace(-3.0 - 0.1 * j, 3.0 + 0.2 * j, G + 1) for j in range(n_prev)])
    w = eng.bar_cell_mass(p.to(DEV), b.to(DEV), torch.linspace(-3.5, 3.5, G + 1).to(DEV))
    theta = torch.rand((n, n_prev + 1), generator=g) * 8.0 - 4.0
    for j in range(n_prev):
        k = torch.randint(0, n, (max(n // 8, 1),), generator=g)
        theta[k, j] = edges[j][torch.randint(0, G + 1, (k.numel(),), generator=g)]     # exactly on an edge
    theta[torch.randint(0, n, (max(n // 50, 1),), generator=g), 0] = float("nan")
    return w, theta.to(DEV), edges.to(DEV)


def _tables(U, n_prev, G):
    return (torch.zeros((U, n_prev, G, G), dtype=torch.int64, device=DEV),
            torch.zeros((U, G), dtype=torch.int64, device=DEV), torch.zeros(U, dtype=torch.int32, device=DEV))


def _both(eng, w, theta, edges, windows, per, U):
    """(device tables, host tables) after the same windows [(lo, hi), ...] of the call's rows."""
    from npe_pfn.pair_marginals import pair_accumulate_host

    n_prev, G = edges.shape[0], w.shape[1]
    dev, host = _tables(U, n_prev, G), _tables(U, n_prev, G)
    for lo, hi in windows:
        eng.pair_accumulate(w[lo:hi], theta[lo:hi], edges, lo, per, *dev)
        pair_accumulate_host(w[lo:hi], theta[lo:hi], edges, lo, per, *host)
    return dev, host


def _same(dev, host):
    return all(torch.equal(d, h) for d, h in zip(dev, host))


@pytest.mark.parametrize("G", [2, 5, 64, 128])
@pytest.mark.parametrize("per", [1, 255, 256, 257, 600])
def test_pair_accumulate_is_the_host_definition(eng, per, G):
    U = 3
    for n_prev in (1, 3, 9):
        w, theta, edges = _acc_inputs(eng, U * per, n_prev, G, seed=per * 1000 + G * 10 + n_prev)
        dev, host = _both(eng, w, theta, edges, [(0, U * per)], per, U)
        assert _same(dev, host), (per, n_prev, G)
        assert dev[2].tolist() == [0, 0, 0] and (per == 1 or int(dev[0].sum()) > 0)
        # in int64: the cells of dim j hold the rows that have one, never more than all the rows
        assert bool((dev[0].sum(2) <= dev[1][:, None, :]).all())


def test_pair_accumulate_windows_offsets_and_nan_rows(eng):
    """Two accumulating calls with r0 > 0, a window that straddles two observations, NaN rows."""
    per, U, n_prev, G = 300, 3, 2, 64
    n = U * per
    w, theta, edges = _acc_inputs(eng, n, n_prev, G, seed=77, nan_rows=(310, 311, 899))
    assert torch.isnan(w[310]).all()
    whole_dev, whole_host = _both(eng, w, theta, edges, [(0, n)], per, U)
    assert _same(whole_dev, whole_host) and whole_dev[2].tolist() == [0, 1, 1]
    # the windows 250..650 and 650..900 straddle observations 0 | 1 and 2; given out of order
    cut_dev, cut_host = _both(eng, w, theta, edges, [(650, 900), (0, 250), (250, 650)], per, U)
    assert _same(cut_dev, cut_host) and _same(cut_dev, whole_dev)
    # n_prev = 0: the cell sums alone
    d0, h0 = _tables(U, 0, G), _tables(U, 0, G)
    from npe_pfn.pair_marginals import pair_accumulate_host

    eng.pair_accumulate(w, None, None, 0, per, *d0)
    pair_accumulate_host(w, None, None, 0, per, *h0)
    assert _same(d0, h0) and torch.equal(d0[1], whole_dev[1])


def test_pair_accumulate_many_workgroups_into_the_same_cells(eng):
    """One observation of 70 000 rows: 274 strips add into the same 64 x 64 cells, and all arrive."""
    n, G = 70_000, 64
    w, theta, edges = _acc_inputs(eng, n, 1, G, seed=5)
    dev, host = _both(eng, w, theta, edges, [(0, n)], n, 1)
    assert _same(dev, host)
    q = torch.round(w * 2.0 ** 40).to(torch.int64)
    assert torch.equal(dev[1][0], q.sum(0))


def test_pair_accumulate_errors(eng):
    w = torch.zeros((4, 4), dtype=torch.float64, device=DEV)
    th = torch.zeros((4, 1), device=DEV)
    ed = torch.linspace(0, 1, 5, device=DEV)[None]
    pairQ, cellQ, bad = _tables(2, 1, 4)
    with pytest.raises(ValueError):
        eng.pair_accumulate(w, th, ed.flip(1), 0, 2, pairQ, cellQ, bad)          # decreasing edges
    with pytest.raises(ValueError):
        eng.pair_accumulate(w, th, ed, 2, 2, pairQ, cellQ, bad)                  # rows of observation 2 of 2
    with pytest.raises(ValueError):
        eng.pair_accumulate(w, th, ed, 0, 2, pairQ.cpu(), cellQ, bad)
    with pytest.raises(ValueError):
        eng.bar_cell_mass(torch.ones((2, 8), device=DEV), torch.arange(9.0, device=DEV), torch.tensor([1.0, 1.0]))
    eng.pair_accumulate(w, th, ed, 0, 2, pairQ, cellQ, bad)
    assert int(cellQ.sum()) == 0


# ------------------------------------------------------------------ the fused call
def _data():
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX + M_OBS, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX + M_OBS, DX))).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x[:N_CTX], th[:N_CTX], x[N_CTX:]))


def _context_edges(th):
    from npe_pfn.pair_marginals import grid_edges

    return grid_edges(torch.stack([th.min(0).values, th.max(0).values], 1), BINS)


def _unfused(eng, x, th, x_rep, draws, per, edges):
    """fit -> predict_logits on the engine's own draws -> fp64 softmax -> cell_mass_ref ->
    pair_accumulate_host -> Q / (2^40 per): ([U, n_pairs, G, G], [U, DTH, G]) fp32."""
    from npe_pfn.pair_marginals import pair_accumulate_host, tables_from_sums

    joint = torch.cat([x, th], 1).cuda()
    feats = torch.cat([x_rep.cuda(), draws], 1)
    U, G = x_rep.shape[0] // per, edges.shape[1] - 1
    pairs, cells = [], []
    for k in range(DTH):
        eng.fit(joint[:, : DX + k], joint[:, DX + k])
        p = torch.softmax(eng.predict_logits(feats[:, : DX + k].contiguous()).double(), -1)
        w = cell_mass_ref(p, eng.borders(), edges[k])
        pairQ, cellQ, bad = _tables(U, k, G)
        pair_accumulate_host(w, draws if k else None, edges[:k] if k else None, 0, per, pairQ, cellQ, bad)
        if k:
            pairs.append(tables_from_sums(pairQ, bad, per))
        cells.append(tables_from_sums(cellQ, bad, per))
    return torch.cat(pairs, 1), torch.stack(cells, 1)


@pytest.fixture(scope="module", params=["none", "ensemble"])
def runs(request, weights):
    from npe_pfn.engine import Engine

    mode = request.param
    x, th, xu = _data()
    e = Engine(CFG, weights, device=DEV, random_state=SEED, preprocessing=mode)
    edges = _context_edges(th).to(DEV)
    r = {"mode": mode, "eng": e, "data": (x, th, xu), "edges": edges}
    r["theta"], r["lp"], r["pair"], r["cell"] = e.ar_pair_marginals(x, th, xu, N, COUNTER, edges, with_log_prob=True)
    r["ref_pair"], r["ref_cell"] = _unfused(e, x, th, xu.repeat_interleave(PER, 0), r["theta"], PER, edges)
    return r


def test_draws_are_those_of_ar_sample(runs):
    e = runs["eng"]
    x, th, xu = runs["data"]
    assert runs["pair"].shape == (M_OBS, 3, BINS, BINS) and runs["cell"].shape == (M_OBS, DTH, BINS)
    assert runs["pair"].is_cuda and runs["pair"].dtype == torch.float32 and runs["cell"].dtype == torch.float32
    draws, lp = e.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER, with_log_prob=True, x_unique=xu)
    assert torch.equal(runs["theta"], draws) and torch.equal(runs["lp"], lp)
    draws2, lp2 = e.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER, with_log_prob=True)
    assert torch.equal(runs["theta"], draws2) and torch.equal(runs["lp"], lp2)
    t3, none, _, _ = e.ar_pair_marginals(x, th, xu, N, COUNTER + 7, runs["edges"], row_base=1000)
    d3, _ = e.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER + 7, row_base=1000, x_unique=xu)
    assert none is None and torch.equal(t3, d3)


def test_fused_matches_the_unfused_route(runs):
    assert bool(torch.isfinite(runs["pair"]).all()) and bool(torch.isfinite(runs["cell"]).all())
    d_pair = (runs["pair"].double() - runs["ref_pair"].double()).abs().max().item()
    d_cell = (runs["cell"].double() - runs["ref_cell"].double()).abs().max().item()
    print(f"{runs['mode']}: max |pair fused - unfused| = {d_pair:.3e}, max |cell fused - unfused| = {d_cell:.3e}; "
          f"mass inside per pair {runs['pair'].sum((-1, -2))[0].tolist()}")
    _parity[runs["mode"]] = {"pair_out": d_pair, "cell_out": d_cell}
    if PARITY_OUT:
        json.dump({"bound": CELL_BOUND, "max_abs_gap": _parity}, open(PARITY_OUT, "w"), indent=1)
    assert float(runs["pair"].sum()) > 0.5 * 3 * M_OBS          # most of the mass is inside the context's range
    assert d_pair <= CELL_BOUND and d_cell <= CELL_BOUND, (d_pair, d_cell)


def test_cells_are_cdf_differences_of_the_averaged_marginals(runs):
    """cell_out against PosteriorMarginals.cdf (npfn_ar_marginals, the same counter) at the edges."""
    from npe_pfn.marginals import PosteriorMarginals

    e = runs["eng"]
    x, th, xu = runs["data"]
    _, _, probs, borders = e.ar_marginals(x, th, xu, N, COUNTER)
    pm = PosteriorMarginals(probs, borders, PER, engine=e)
    pts = runs["edges"].t()[None].expand(M_OBS, BINS + 1, DTH).contiguous()        # [M, G + 1, d]
    F = pm.cdf(pts).double()
    want = (F[:, 1:] - F[:, :-1]).transpose(1, 2)                                   # [M, d, G]
    gap = (runs["cell"].double() - want).abs().max().item()
    print(f"{runs['mode']}: max |cell_out - cdf differences| = {gap:.3e}")
    assert gap <= CELL_BOUND, gap


def test_pair_rows_sum_to_the_cells_when_the_limits_hold_every_draw(runs):
    """Limits from the draws of a first call with the same counter: every row has a cell in every
    earlier dimension, so sum_a pair == cell exactly in the integer sums; in the fp32 outputs each
    of the G + 1 numbers is rounded once: |sum_a pair - cell| <= 2^-24 (sum_a pair + cell)."""
    from npe_pfn.pair_marginals import grid_edges

    e = runs["eng"]
    x, th, xu = runs["data"]
    d = runs["theta"]
    lim = torch.stack([d.min(0).values - 0.25, d.max(0).values + 0.25], 1)
    edges = grid_edges(lim.cpu(), BINS).to(DEV)
    t, _, pair, cell = e.ar_pair_marginals(x, th, xu, N, COUNTER, edges)
    assert torch.equal(t, d)
    for k in range(1, DTH):
        for j in range(k):
            s = pair[:, pair_index(j, k)].double().sum(1)
            c = cell[:, k].double()
            bound = 2.0 ** -24 * (s + c) * (1 + 1e-6) + 1e-30
            assert bool(((s - c).abs() <= bound).all()), (j, k, (s - c).abs().max().item())
    # the first axis is the earlier parameter: its own margin is the histogram of the draws' cells
    a0 = torch.searchsorted(edges[0].contiguous(), d[:, 0].contiguous(), right=True) - 1
    hist = torch.stack([torch.bincount(a0[u * PER: (u + 1) * PER], minlength=BINS) for u in range(M_OBS)]).double() / PER
    got = pair[:, pair_index(0, 1)].double().sum(2)
    mass1 = cell[:, 1].double().sum(1, keepdim=True)                 # the share of theta_1 inside its limits
    assert (got - hist).abs().max().item() <= 1.0 - float(mass1.min()) + 1e-6


def test_reproducible_chunked_and_alone(runs):
    """The same call twice, in chunks of 32 rows (chunks 2 and 4 span two observations), and
    observation 1 alone at the Philox rows it has among the others: integer sums, so torch.equal."""
    e = runs["eng"]
    x, th, xu = runs["data"]
    want = (runs["theta"], runs["lp"], runs["pair"], runs["cell"])

    def same(got):
        return all(torch.equal(g, w) for g, w in zip(got, want))

    assert same(e.ar_pair_marginals(x, th, xu, N, COUNTER, runs["edges"], with_log_prob=True))
    e.set_chunk_rows(32)
    try:
        assert same(e.ar_pair_marginals(x, th, xu, N, COUNTER, runs["edges"], with_log_prob=True))
    finally:
        e.set_chunk_rows(16384)
    t1, lp1, p1, c1 = e.ar_pair_marginals(x, th, xu[1:2], PER, COUNTER, runs["edges"], with_log_prob=True, row_base=PER)
    assert torch.equal(t1, runs["theta"][PER: 2 * PER]) and torch.equal(lp1, runs["lp"][PER: 2 * PER])
    assert torch.equal(p1[0], runs["pair"][1]) and torch.equal(c1[0], runs["cell"][1])


def test_fused_errors(runs):
    e = runs["eng"]
    x, th, xu = runs["data"]
    with pytest.raises(ValueError):
        e.ar_pair_marginals(x, th, xu, N + 1, COUNTER, runs["edges"])             # 3 does not divide 151
    with pytest.raises(ValueError):
        e.ar_pair_marginals(x, th, xu, N, COUNTER, runs["edges"][:2])             # edges of 2 parameters
    with pytest.raises(ValueError):
        e.ar_pair_marginals(x, th, xu, N, COUNTER, runs["edges"].flip(1))
    t, _, p, c = e.ar_pair_marginals(x, th, xu, N, COUNTER, runs["edges"])        # still usable, the same bits
    assert torch.equal(t, runs["theta"]) and torch.equal(p, runs["pair"]) and torch.equal(c, runs["cell"])


# ------------------------------------------------------------------ the public API
class _GenericOnly:
    """A regressor that shows fit / predict only: NPE_PFN_Core then takes its generic loops."""

    def __init__(self, reg):
        self._reg = reg

    def fit(self, X, y):
        return self._reg.fit(X, y)

    def predict(self, X, **kw):
        return self._reg.predict(X, **kw)


def _post(x, th):
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    post = TabPFN_Based_NPE_PFN(regressor_init_kwargs={"random_state": SEED, "device": "cuda:0"})
    post.append_simulations(th, x)
    return post


def test_public_api_engine_against_the_generic_loop():
    """The engine route and a twin estimator forced through _pair_marginals_generic (the same
    counters, hence the same draws): 3 observations x 50 draws in one call, then one observation
    with 120 draws in engine calls of at most 50 (50 + 50 + 20).  The generic loop draws from the
    fp32 logits, so its draws are not the fused ones bit for bit; measured on the MI355X: draws up
    to 2.8e-3 / 2.2e-3 apart, tables 2.8e-5 / 9.3e-6 apart (bound 4e-5)."""
    x, th, xu = (a.cuda() for a in _data())
    post, twin = _post(x, th), _post(x, th)
    twin._model = _GenericOnly(twin._model)
    lim = torch.stack([th.min(0).values, th.max(0).values], 1)
    for obs, kw in ((xu, {"num_draws": PER}), (xu[:1], {"num_draws": 120, "max_sampling_batch_size": 50})):
        c0 = post._model.sample_counter
        pm = post.pair_marginals(obs, bins=BINS, return_samples=True, **kw)
        calls = -(-kw["num_draws"] // (kw.get("max_sampling_batch_size", 10_000) // obs.shape[0]))
        assert post._model.sample_counter - c0 == calls * DTH
        ref = twin.pair_marginals(obs, bins=BINS, limits=lim, return_samples=True, **kw)
        M = obs.shape[0]
        assert pm.probs.shape == (M, 3, BINS, BINS) and pm.marginal_probs.shape == (M, DTH, BINS)
        assert pm.probs.is_cuda and pm.edges.is_cuda and pm.num_draws == kw["num_draws"]
        assert pm.samples.shape == (M, kw["num_draws"], DTH)
        assert torch.equal(pm.edges, ref.edges)                  # the default limits: the context's min / max
        moved = (pm.samples - ref.samples.to(pm.samples.device)).abs().max().item()
        d_pair = (pm.probs.double() - ref.probs.double().to(DEV)).abs().max().item()
        d_cell = (pm.marginal_probs.double() - ref.marginal_probs.double().to(DEV)).abs().max().item()
        print(f"{M} obs x {kw['num_draws']}: max |draw fused - generic| = {moved:.3e}, "
              f"max |pair| gap = {d_pair:.3e}, max |cell| gap = {d_cell:.3e}")
        assert d_pair <= CELL_BOUND and d_cell <= CELL_BOUND, (d_pair, d_cell)
        # summaries run on the device
        assert pm.credible_region(0, 2, 0.9).shape == (M, BINS, BINS) and pm.correlation().shape == (M, DTH, DTH)
        inside = pm.mass_inside(0, 1)
        assert bool((inside > 0.5).all()) and bool((inside <= 1 + 1e-6).all())


def test_unconditional_estimator_mixes_its_clusters():
    from npe_pfn import TabPFN_Based_Uncond_Estimator
    from npe_pfn.npe_pfn import NPE_PFN_Core

    rng = np.random.default_rng(3)
    theta = np.concatenate([rng.normal(-2.0, 0.3, size=(40, 2)), rng.normal(1.5, 0.3, size=(60, 2))]).astype(np.float32)
    torch.manual_seed(0)
    est = TabPFN_Based_Uncond_Estimator(num_clusters=2, regressor_init_kwargs={"random_state": 0, "device": DEV})
    est.append_simulations(torch.from_numpy(theta).to(DEV))
    assert sorted(est.counts.tolist()) == [40, 60]
    c0 = est._model.sample_counter
    torch.manual_seed(7)
    pm = est.pair_marginals(num_draws=40, bins=8)
    assert pm.probs.shape == (1, 1, 8, 8) and pm.probs.is_cuda
    assert pm.edges[:, 0].tolist() == theta.min(0).tolist() and pm.edges[:, -1].tolist() == theta.max(0).tolist()
    # the clusters one by one, with the counters and the dummy x the call used
    est._model.sample_counter = c0
    torch.manual_seed(7)
    lim = torch.stack([pm.edges[:, 0], pm.edges[:, -1]], 1)
    parts = []
    for c in range(2):
        est.set_cluster_state(c)
        parts.append(NPE_PFN_Core.pair_marginals(est, torch.randn(1, 1).to(DEV), num_draws=40, bins=8, limits=lim))
    est.set_cluster_state()
    wts = est.counts / est.counts.sum()
    assert (parts[0].marginal_probs - parts[1].marginal_probs).abs().max().item() > 0.1     # the clusters differ
    for name in ("marginal_probs", "probs"):
        want = sum(float(wts[c]) * getattr(parts[c], name).double() for c in range(2))
        gap = (getattr(pm, name).double() - want).abs().max().item()
        assert gap <= 1e-7, (name, gap)                      # one fp32 rounding of the fp64 mix
    assert pm.mass_inside(0, 1).item() > 0.8
