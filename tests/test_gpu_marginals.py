"""GPU: npfn_ar_marginals -- the posterior marginals averaged over the sampler's own conditionals.

The shapes of tests/test_gpu_ar_score.py: 150 context rows, dim_x = 3, dim_theta = 3, preprocessing
"none" and "ensemble", synthetic weights (seed 0); 3 observations x 50 draws = 150 rows.  Everything
the tests read is computed once per mode (fixture ``runs``), the unfused reference included.
"""
import json
import os

import numpy as np
import pytest
import torch

from bar_stats_ref import bar_means, ulp32
from npe_pfn.diagnostics import pit_ks_statistic
from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
N_CTX, DX, DTH = 150, 3, 3
M_OBS, PER = 3, 50
N = M_OBS * PER
SEED = 2
COUNTER = 5
N_KS = 512
CUM_BOUND = 2e-5   # on cumulative sums; the bound and the reasoning of test_cdf_steps_match_the_unfused_route
# NPFN_MARGINALS_PARITY_OUT=<file>: test_steps_match_the_unfused_route also records its maxima there
# (profiles/marginals/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_MARGINALS_PARITY_OUT")
_parity = {}


def _data():
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX + M_OBS, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX + M_OBS, DX))).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x[:N_CTX], th[:N_CTX], x[N_CTX:]))


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(CFG, seed=0)


def _unfused(eng, x, th, x_rep, draws, per):
    """fit -> predict_logits per step on the draws' own features; each row normalised in fp64, the
    mean over each observation's rows in fp64: ([U, DTH, nb] fp64, [DTH, nb + 1] borders)."""
    joint = torch.cat([x, th], 1).cuda()
    feats = torch.cat([x_rep.cuda(), draws], 1)
    probs, borders = [], []
    for k in range(DTH):
        eng.fit(joint[:, : DX + k], joint[:, DX + k])
        p = torch.softmax(eng.predict_logits(feats[:, : DX + k].contiguous()).double(), -1)
        probs.append(p.reshape(-1, per, p.shape[-1]).mean(1))
        borders.append(eng.borders())
    return torch.stack(probs, 1), torch.stack(borders, 0)


@pytest.fixture(scope="module", params=["none", "ensemble"])
def runs(request, weights):
    from npe_pfn.engine import Engine

    mode = request.param
    x, th, xu = _data()
    eng = Engine(CFG, weights, device=torch.device("cuda", 0), random_state=SEED, preprocessing=mode)
    r = {"mode": mode, "eng": eng, "data": (x, th, xu)}
    r["theta"], r["lp"], r["probs"], r["borders"] = eng.ar_marginals(x, th, xu, N, COUNTER, with_log_prob=True)
    r["ref_probs"], r["ref_borders"] = _unfused(eng, x, th, xu.repeat_interleave(PER, 0), r["theta"], PER)
    return r


def _cum_gap(probs, ref):
    return (torch.cumsum(probs.double(), -1) - torch.cumsum(ref, -1)).abs().max().item()


def test_draws_are_those_of_ar_sample(runs):
    eng = runs["eng"]
    x, th, xu = runs["data"]
    assert runs["probs"].shape == (M_OBS, DTH, CFG.n_bars) and runs["borders"].shape == (DTH, CFG.n_bars + 1)
    assert runs["probs"].is_cuda and runs["probs"].dtype == torch.float32
    draws, lp = eng.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER, with_log_prob=True, x_unique=xu)
    assert torch.equal(runs["theta"], draws) and torch.equal(runs["lp"], lp)
    # the steps >= 1 went through k_mix_prob + k_group_sample(per = 1): also equal to the plain
    # sampler's fused k_mix_sample over every row
    draws2, lp2 = eng.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER, with_log_prob=True)
    assert torch.equal(runs["theta"], draws2) and torch.equal(runs["lp"], lp2)
    # and with an offset into the Philox rows, without the log density
    t3, none, _, _ = eng.ar_marginals(x, th, xu, N, COUNTER + 7, row_base=1000)
    d3, _ = eng.ar_sample(x, th, xu.repeat_interleave(PER, 0), COUNTER + 7, row_base=1000, x_unique=xu)
    assert none is None and torch.equal(t3, d3)


def test_step_0_is_the_distinct_rows_mixture(runs):
    """probs[u, 0] is the k_mix_prob row of observation u, normalised: fit on the step-0 table,
    predict_logits(x_u), exponentiated and normalised in fp64.  |d| <= 2e-5 on the cumulative sums
    (the unfused route rounds log p to fp32 and exponentiates again); borders bit for bit."""
    eng = runs["eng"]
    x, th, xu = runs["data"]
    eng.fit(x, th[:, 0])
    ref = torch.softmax(eng.predict_logits(xu).double(), -1)
    assert torch.equal(runs["borders"][0], eng.borders())
    d = _cum_gap(runs["probs"][:, 0], ref)
    print(f"{runs['mode']} step 0: max |cum fused - cum unfused| = {d:.3e}")
    _parity.setdefault(runs["mode"], {})["step0"] = d
    assert d <= CUM_BOUND, d


def test_steps_match_the_unfused_route(runs):
    for k in range(DTH):
        d = _cum_gap(runs["probs"][:, k], runs["ref_probs"][:, k])
        print(f"{runs['mode']} step {k}: max |cum fused - cum unfused| = {d:.3e}")
        _parity.setdefault(runs["mode"], {})[f"step{k}_mean_over_{PER}"] = d
        assert torch.equal(runs["borders"][k], runs["ref_borders"][k]), k
        assert d <= CUM_BOUND, (k, d)
    sums = runs["probs"].double().sum(-1)
    print(f"{runs['mode']}: max |sum_b probs - 1| = {(sums - 1).abs().max().item():.3e}")
    assert (sums - 1).abs().max().item() <= 1e-6
    assert bool((runs["probs"] >= 0).all())
    if PARITY_OUT:
        json.dump({"bound": CUM_BOUND, "max_abs_cumulative_gap": _parity}, open(PARITY_OUT, "w"), indent=1)


def test_reproducible_chunked_and_fit_reuse(runs):
    """The same call twice; in chunks of 32 rows (150 rows: 32 / 32 / 32 / 32 / 22 -- no cut on an
    observation boundary, chunks 2 and 4 span two observations); with a fit token, first and
    reused.  The reduction adds an observation's rows in row order whatever the chunking (a strip
    cut by a chunk continues from its stored fp64 partial), so the marginals are compared with
    torch.equal, not to an ulp."""
    eng = runs["eng"]
    x, th, xu = runs["data"]
    want = (runs["theta"], runs["lp"], runs["probs"], runs["borders"])

    def same(got):
        return all(torch.equal(g, w) for g, w in zip(got, want))

    assert same(eng.ar_marginals(x, th, xu, N, COUNTER, with_log_prob=True))
    eng.set_chunk_rows(32)
    try:
        assert same(eng.ar_marginals(x, th, xu, N, COUNTER, with_log_prob=True))
    finally:
        eng.set_chunk_rows(16384)
    eng.set_fit_token(4321)
    try:
        first = eng.ar_marginals(x, th, xu, N, COUNTER, with_log_prob=True)
        again = eng.ar_marginals(x, th, xu, N, COUNTER, with_log_prob=True)   # reuses every step's fit
    finally:
        eng.set_fit_token(0)
    assert same(first) and same(again)


def test_segments_do_not_leak(runs):
    """Observation 1 alone, at the Philox rows it has in the 3-observation call: its draws and its
    marginals (bit for bit: the same rows in the same order)."""
    eng = runs["eng"]
    x, th, xu = runs["data"]
    t1, lp1, p1, b1 = eng.ar_marginals(x, th, xu[1:2], PER, COUNTER, with_log_prob=True, row_base=PER)
    assert torch.equal(t1, runs["theta"][PER: 2 * PER]) and torch.equal(lp1, runs["lp"][PER: 2 * PER])
    assert torch.equal(p1[0], runs["probs"][1]) and torch.equal(b1, runs["borders"])


def test_consistent_with_the_draws(runs):
    """512 draws of one observation against the marginal CDFs: KS distance per dimension <=
    1.95 / sqrt(512) (alpha = 0.001; the draws' empirical CDF has the averaged conditionals as its
    expectation).  512 rows are 8 strips of 64; in chunks of 100 rows every cut falls inside a
    strip, and the bits stay."""
    from npe_pfn.marginals import PosteriorMarginals

    eng = runs["eng"]
    x, th, xu = runs["data"]
    draws, _, probs, borders = eng.ar_marginals(x, th, xu[:1], N_KS, 0)
    pm = PosteriorMarginals(probs, borders, N_KS, engine=eng)
    u = pm.cdf(draws[None])
    assert u.shape == (1, N_KS, DTH) and u.is_cuda
    ks = pit_ks_statistic(u[0].cpu())
    print(f"{runs['mode']}: KS per dimension = {ks.tolist()} (critical {1.95 / np.sqrt(N_KS):.4f})")
    assert float(ks.max()) <= 1.95 / np.sqrt(N_KS), ks
    eng.set_chunk_rows(100)
    try:
        d2, _, p2, _ = eng.ar_marginals(x, th, xu[:1], N_KS, 0)
    finally:
        eng.set_chunk_rows(16384)
    assert torch.equal(d2, draws) and torch.equal(p2, probs)


def test_errors(runs):
    from npe_pfn.engine import _ptr

    eng = runs["eng"]
    x, th, xu = runs["data"]
    with pytest.raises(ValueError):
        eng.ar_marginals(x, th, xu, N + 1, COUNTER)              # 3 does not divide 151
    with pytest.raises(ValueError):
        eng.ar_marginals(x, th, xu[:, :2], N, COUNTER)
    dev = [a.cuda().contiguous() for a in (x, th, xu)]
    out = torch.empty((N, DTH), device="cuda")
    marg = torch.empty((M_OBS, DTH, CFG.n_bars), device="cuda")
    bd = torch.empty((DTH, CFG.n_bars + 1), device="cuda")
    lib, h, s = eng.lib, eng.h, eng.stream
    args = (h, _ptr(dev[0]), _ptr(dev[1]), N_CTX, DX, DTH, _ptr(dev[2]))
    tail = (COUNTER, 0, _ptr(out), None, 1e-15)
    assert lib.npfn_ar_marginals(*args, M_OBS, N, *tail, None, _ptr(bd), s) == -1        # marg_out NULL
    assert b"ar_marginals" in lib.npfn_last_error()
    assert lib.npfn_ar_marginals(*args, M_OBS, N, *tail, _ptr(marg), None, s) == -1      # borders_out NULL
    assert lib.npfn_ar_marginals(*args, 0, N, *tail, _ptr(marg), _ptr(bd), s) == -1      # n_unique < 1
    assert lib.npfn_ar_marginals(*args, 4, N, *tail, _ptr(marg), _ptr(bd), s) == -1      # 4 does not divide 150
    assert lib.npfn_ar_marginals(*args, M_OBS, N, COUNTER, -1, _ptr(out), None, 1e-15, _ptr(marg), _ptr(bd),
                                 s) == -1                                                  # negative row_base
    # the engine is still usable, and gives the same bits
    t, _, p, _ = eng.ar_marginals(x, th, xu, N, COUNTER)
    assert torch.equal(t, runs["theta"]) and torch.equal(p, runs["probs"])


# ------------------------------------------------------------------ the public API
@pytest.fixture(scope="module")
def api():
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    x, th, xu = (a.cuda() for a in _data())
    post = TabPFN_Based_NPE_PFN(regressor_init_kwargs={"random_state": SEED, "device": "cuda:0"})
    post.append_simulations(th, x)
    return post, x, th, xu, post.marginals(xu, num_draws=PER)


def test_public_api_shapes_and_summaries(api):
    post, x, th, xu, pm = api
    nb = CFG.n_bars
    assert pm.probs.shape == (M_OBS, DTH, nb) and pm.borders.shape == (DTH, nb + 1) and pm.num_draws == PER
    assert pm.probs.is_cuda and pm.borders.is_cuda and pm.support_fraction.shape == (M_OBS,)
    assert torch.isnan(pm.support_fraction).all() and pm.samples is None       # no prior
    med, mean, mode, iv = pm.median(), pm.mean(), pm.mode(), pm.interval(0.9)
    assert med.shape == mean.shape == mode.shape == (M_OBS, DTH) and iv.shape == (M_OBS, DTH, 2) and med.is_cuda
    assert torch.equal(pm.quantile(0.5), med)
    assert bool((iv[..., 0] <= med).all()) and bool((med <= iv[..., 1]).all())
    qs = [0.1, 0.5, 0.9]
    quant = pm.quantile(qs)
    assert quant.shape == (3, M_OBS, DTH)
    lp = pm.log_prob(med)
    assert lp.shape == (M_OBS, DTH) and bool(torch.isfinite(lp).all())
    for k in range(DTH):
        b = pm.borders[k]
        for i, q in enumerate(qs):
            pt = quant[i, :, k]
            assert bool(((pt > b[1]) & (pt < b[-2])).all()), "a quantile of the test data fell into a tail bar"
            back = pm.cdf(quant[i])[:, k]
            gap = (back - q).abs().max().item()
            print(f"dim {k} q={q}: max |cdf(quantile(q)) - q| = {gap:.3e}")
            assert gap <= 1e-5, (k, q, gap)
        # the mean: fp64 sum of masses x bar means (half-normal tail means), bar_stats_ref's
        # statement, with test_gpu_bar_stats.py's bound 2e-5 span + 4 ulp32(|ref|)
        p64 = pm.probs[:, k].double().cpu().numpy()
        bk = b.cpu().numpy()
        ref = (p64 / p64.sum(1, keepdims=True)) @ bar_means(bk)
        err = np.abs(mean[:, k].double().cpu().numpy() - ref)
        bound = 2e-5 * (float(bk[-1]) - float(bk[0])) + 4 * ulp32(ref)
        print(f"dim {k} mean: max |mean - ref| = {err.max():.3e} (bound {bound.min():.3e})")
        assert (err <= bound).all(), (k, err.max())


def test_public_api_support_fraction_with_a_box_prior(api):
    post, x, th, xu, _ = api
    med = th.median(0).values
    low = torch.where(torch.arange(DTH, device="cuda") == 0, med, torch.full_like(med, -1e3))
    prior = torch.distributions.Independent(torch.distributions.Uniform(low, torch.full_like(med, 1e3)), 1)
    post.prior = prior
    try:
        pm = post.marginals(xu, num_draws=PER, return_samples=True)
    finally:
        post.prior = None
    assert pm.samples.shape == (M_OBS, PER, DTH)
    s = pm.samples.cpu()
    inside = ((s >= low.cpu()) & (s <= 1e3)).all(-1).sum(1).double() / PER
    print(f"support_fraction = {pm.support_fraction.tolist()}")
    assert torch.equal(pm.support_fraction.cpu(), inside)
    assert 0.0 < float(inside.sum()) < M_OBS            # the box cuts some of the draws, not all


def test_public_api_three_engine_calls(api):
    """One observation, 120 draws in calls of at most 50 rows: 50 + 50 + 20, combined with their
    row counts as weights, against the unfused route on the returned draws."""
    post, x, th, xu, _ = api
    eng = post._model.engine
    c0 = post._model.sample_counter
    pm = post.marginals(xu[:1], num_draws=120, max_sampling_batch_size=50, return_samples=True)
    assert post._model.sample_counter - c0 == 3 * DTH
    assert pm.samples.shape == (1, 120, DTH) and pm.num_draws == 120
    th_c, x_c = post.get_context(xu[:1])
    ref, ref_b = _unfused(eng, x_c.cpu(), th_c.cpu(), xu[:1].repeat_interleave(120, 0), pm.samples[0], 120)
    assert torch.equal(pm.borders, ref_b)
    for k in range(DTH):
        d = _cum_gap(pm.probs[:, k], ref[:, k])
        print(f"step {k}: max |cum fused - cum unfused| = {d:.3e}")
        assert d <= CUM_BOUND, (k, d)
    assert (pm.probs.double().sum(-1) - 1).abs().max().item() <= 1e-6


def test_unconditional_estimator_has_no_marginals():
    from npe_pfn.npe_pfn import TabPFN_Based_Uncond_Estimator

    est = TabPFN_Based_Uncond_Estimator(regressor_init_kwargs={"device": "cuda:0"})
    with pytest.raises(NotImplementedError):
        est.marginals(torch.zeros(1, 1))
