"""GPU: npfn_rank_accumulate against its torch definition (exact equality), coverage_batched and the
leakage correction on the engine, and the self-consistency of the ranks.

The estimator tests use the shapes of tests/test_gpu_marginals.py: 150 context rows, dim_x =
dim_theta = 3, synthetic weights, preprocessing "none" and "ensemble".
"""
import json
import os

import numpy as np
import pytest
import torch

from npe_pfn.diagnostics import rank_accumulate_host, rank_ks_statistic
from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
STRIP = 256                      # rows of one observation per workgroup (npfn_ranks.hip kStrip)
PERS = (1, 63, 64, 65, 130, 2 * STRIP + 1)   # the last: three workgroups per observation, one row in the third
N_CTX, DX, DTH = 150, 3, 3
M_OBS, S = 4, 64
SEED = 2
M_SELF, S_SELF = 256, 63
KS_BOUND = 1.95 / np.sqrt(M_SELF)   # alpha = 0.001, as tests/test_gpu_marginals.py at n = 512
# NPFN_COVERAGE_PARITY_OUT=<file>: test_self_consistency also records its statistics there
# (profiles/coverage/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_COVERAGE_PARITY_OUT")


@pytest.fixture(scope="module")
def eng():
    from npe_pfn.engine import Engine

    return Engine(CFG, synthetic_weights(CFG, seed=0), device=torch.device("cuda", 0), random_state=SEED)


# ------------------------------------------------------------------ the kernel
def case(n_obs, per, dim, kind, seed=0):
    """CPU tensors of one call.  "grid": multiples of 1/8 and power-of-two scales, the first draw of
    every observation equal to its truth, so every column has ties; "normal": random normals."""
    rng = np.random.default_rng(1000 * seed + 10 * per + dim)
    if kind == "grid":
        g = lambda *shape: (rng.integers(-4, 5, size=shape) / 8.0).astype(np.float32)  # noqa: E731
        inv = (2.0 ** rng.integers(-2, 3, size=dim)).astype(np.float32)
    else:
        g = lambda *shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
        inv = rng.uniform(0.1, 3.0, size=dim).astype(np.float32)
    c = dict(theta=g(n_obs * per, dim), logp=g(n_obs * per), take=None, n_obs=n_obs, per=per,
             theta_true=g(n_obs, dim), logp_true=g(n_obs), ref=g(n_obs, dim), inv_scale=inv)
    if kind == "grid":
        c["theta"][::per] = c["theta_true"]
        c["logp"][::per] = c["logp_true"]
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


ORDER = ("theta", "logp", "take", "n_obs", "per", "theta_true", "logp_true", "ref", "inv_scale")


def host(c, init=None):
    dim = c["theta"].shape[1]
    counts = torch.zeros((c["n_obs"], dim + 2, 2), dtype=torch.int64) if init is None else init.clone()
    rank_accumulate_host(*(c[k] for k in ORDER), counts)
    return counts


def device(eng, c, init=None):
    dim = c["theta"].shape[1]
    counts = torch.zeros((c["n_obs"], dim + 2, 2), dtype=torch.int64) if init is None else init.clone()
    counts = counts.cuda()
    eng.rank_accumulate(*(c[k].cuda() if isinstance(c[k], torch.Tensor) else c[k] for k in ORDER), counts)
    return counts.cpu()


@pytest.mark.parametrize("dim", [1, 3, 5, 8])
def test_kernel_equals_the_definition(eng, dim):
    for per in PERS:
        for kind in ("grid", "normal"):
            c = case(3, per, dim, kind)
            want = host(c)
            if kind == "grid":
                assert int(want[:, :, 1].min()) >= 1, "the grid case has a column without a tie"
            got = device(eng, c)
            assert torch.equal(got, want), (per, kind)
            assert torch.equal(device(eng, c), got), (per, kind)          # the same call twice


@pytest.mark.parametrize("dim", [33, 70])
def test_kernel_wide_tables_take_several_column_passes(eng, dim):
    """More than 32 columns: the strip is staged in passes of 32 columns (70 = 32 + 32 + 6)."""
    for per in (65, 2 * STRIP + 1):
        for kind in ("grid", "normal"):
            c = case(3, per, dim, kind)
            assert torch.equal(device(eng, c), host(c)), (per, kind)


@pytest.mark.parametrize("dim", [1, 3, 5, 8])
def test_kernel_masks_pairs_nan_and_accumulation(eng, dim):
    per = 2 * STRIP + 1
    rng = np.random.default_rng(77 + dim)
    for kind in ("grid", "normal"):
        c = case(3, per, dim, kind, seed=1)
        take = torch.from_numpy(rng.random((3, per)) < 0.6)
        take[0, 64:128] = False            # a wave of the first workgroup without a row
        take[0, STRIP: 2 * STRIP] = False  # a whole workgroup without a row
        take[1] = False                    # an observation without a row
        take[2, 0] = True
        c["take"] = take.reshape(-1)
        want = host(c)
        assert torch.equal(device(eng, c), want), kind
        assert int(want[1].abs().sum()) == 0 and int(want[0].sum()) > 0
        # uint8 mask, as the C entry point reads it
        assert torch.equal(device(eng, dict(c, take=c["take"].to(torch.uint8))), want)
        # a nullable pair absent: its column keeps the caller's (non-zero) values
        init = torch.arange(3 * (dim + 2) * 2, dtype=torch.int64).reshape(3, dim + 2, 2) + 7
        no_lp = device(eng, dict(c, logp=None, logp_true=None), init)
        assert torch.equal(no_lp, host(dict(c, logp=None, logp_true=None), init))
        assert torch.equal(no_lp[:, dim], init[:, dim])
        no_ref = device(eng, dict(c, ref=None, inv_scale=None), init)
        assert torch.equal(no_ref, host(dict(c, ref=None, inv_scale=None), init))
        assert torch.equal(no_ref[:, dim + 1], init[:, dim + 1])
        # a NaN row counts nowhere
        bad = dict(c, theta=c["theta"].clone(), logp=c["logp"].clone())
        bad["theta"][2 * per, 0] = float("nan")
        bad["logp"][2 * per] = float("nan")
        got = device(eng, bad)
        assert torch.equal(got, host(bad))
        gone = dict(c, take=c["take"].clone())
        gone["take"][2 * per] = False
        without = host(gone)
        for col in (0, dim, dim + 1):    # the row drops out of these; its distance is NaN too
            assert torch.equal(got[:, col], without[:, col]), col
        # two accumulating calls (rounds of 130 and 65 rows) against one call of 195 rows
        a, b = case(3, 130, dim, kind, seed=2), case(3, 65, dim, kind, seed=3)
        both = dict(a, per=195)
        for key in ("theta_true", "logp_true", "ref", "inv_scale"):
            b[key] = a[key]
        both["theta"] = torch.cat([a["theta"].reshape(3, 130, dim), b["theta"].reshape(3, 65, dim)], 1).reshape(-1, dim)
        both["logp"] = torch.cat([a["logp"].reshape(3, 130), b["logp"].reshape(3, 65)], 1).reshape(-1)
        two = device(eng, b, device(eng, a))
        assert torch.equal(two, device(eng, both)) and torch.equal(two, host(both))


def test_kernel_every_taken_row_arrives(eng):
    """One observation of 70 000 rows (274 workgroups adding into the same counters), the truth
    above every draw in dimension 0."""
    per = 70_000
    c = case(1, per, 2, "normal", seed=4)
    c["theta_true"][0, 0] = float(c["theta"][:, 0].max()) + 1.0
    got = device(eng, c)
    assert int(got[0, 0, 0]) == per and int(got[0, 0, 1]) == 0
    assert torch.equal(got, host(c))


def test_engine_method_refuses_bad_shapes(eng):
    c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in case(3, 65, 3, "grid").items()}
    counts = torch.zeros((3, 5, 2), dtype=torch.int64, device="cuda")
    args = [c[k] for k in ORDER]

    def call(**kw):
        a = dict(zip(ORDER, args), **kw)
        eng.rank_accumulate(*(a[k] for k in ORDER), a.get("counts", counts))

    for kw in (dict(theta=c["theta"][:-1]), dict(per=64), dict(theta_true=c["theta_true"][:, :2]),
               dict(logp=None), dict(inv_scale=None), dict(ref=c["ref"][:2]), dict(take=torch.ones(7).cuda()),
               dict(counts=counts.cpu()), dict(counts=counts.to(torch.int32)), dict(counts=counts[:, :4])):
        with pytest.raises(ValueError):
            call(**kw)
    assert int(counts.abs().sum()) == 0


# ------------------------------------------------------------------ coverage_batched on the engine
def _data(m):
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX + m, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX + m, DX))).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (x[:N_CTX], th[:N_CTX], x[N_CTX:], th[N_CTX:]))


def _box(th_ctx, q):
    """Cuts dimension 0 at the context's q-quantile; the other dimensions are unbounded in effect."""
    low = torch.full((DTH,), -1e3, device="cuda")
    low[0] = torch.quantile(th_ctx[:, 0], q)
    return torch.distributions.Independent(torch.distributions.Uniform(low, torch.full((DTH,), 1e3, device="cuda")), 1)


def _post(mode, prior, x, th):
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    post = TabPFN_Based_NPE_PFN(prior=prior, regressor_init_kwargs={"random_state": SEED, "device": "cuda:0",
                                                                    "preprocessing": mode})
    return post.append_simulations(th, x)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("mode", ["none", "ensemble"])
def test_coverage_batched_on_the_engine(mode, with_prior):
    x, th, x_o, th_o = _data(M_OBS)
    prior = _box(th, 0.3) if with_prior else None
    post, twin = _post(mode, prior, x, th), _post(mode, prior, x, th)
    torch.manual_seed(3)
    cov = post.coverage_batched(th_o, x_o, num_posterior_samples=S, return_samples=True)
    assert cov.less.shape == (M_OBS, DTH + 2) and cov.less.is_cuda and cov.less.dtype == torch.int64
    lp_true = twin.log_prob_batched(th_o, x_o)
    samples, sample_lp = twin.sample_batched(x_o, (S,), with_log_prob=True)
    assert torch.equal(cov.log_prob_true, lp_true)
    assert torch.equal(cov.samples, samples) and torch.equal(cov.sample_log_probs, sample_lp)
    assert post._model.sample_counter == twin._model.sample_counter
    want = torch.zeros((M_OBS, DTH + 2, 2), dtype=torch.int64)
    rank_accumulate_host(samples.reshape(M_OBS * S, DTH).cpu(), sample_lp.reshape(-1).cpu(), None, M_OBS, S,
                         th_o.cpu(), lp_true.cpu(), cov.references.cpu(), cov.inv_scale.cpu(), want)
    assert torch.equal(cov.less.cpu(), want[:, :, 0]) and torch.equal(cov.equal.cpu(), want[:, :, 1])
    # without return_samples: the same ranks from a fresh estimator, nothing kept
    lean = _post(mode, prior, x, th).coverage_batched(th_o, x_o, num_posterior_samples=S, references=cov.references)
    assert lean.samples is None and torch.equal(lean.less, cov.less) and torch.equal(lean.equal, cov.equal)
    if with_prior:
        low = prior.base_dist.low
        assert bool((cov.samples >= low).all()), "a kept draw lies outside the box"
        # the first round (96 unrejected draws per observation) loses some, not all, draws of an observation
        first = _post(mode, None, x, th).sample_batched(x_o, (int(S * 1.5),))
        inside = (first >= low).all(-1).sum(1)
        print(f"{mode}: first-round draws inside the box per observation = {inside.tolist()} of {int(S * 1.5)}")
        assert bool(((inside > 0) & (inside < int(S * 1.5))).any())


def test_self_consistency():
    """Truths drawn from the estimator itself are exchangeable with its draws, so every column's
    rank is uniform on {0..63} whatever the weights are: each of the d_theta + 2 distances from the
    discrete uniform must be below 1.95 / sqrt(256) = 0.122 (alpha = 0.001; conservative for a
    discrete statistic).  Seeds fixed before the first run."""
    x, th, x_o, _ = _data(M_SELF)
    prior = _box(th, 0.1)
    post = _post("ensemble", prior, x, th)
    torch.manual_seed(11)
    truths = post.sample_batched(x_o, (1,), oversample_factor=8.0)[:, 0]
    cov = post.coverage_batched(truths, x_o, num_posterior_samples=S_SELF)
    assert cov.samples is None and bool(((cov.less + cov.equal) <= S_SELF).all())
    ks = rank_ks_statistic(cov.less.cpu(), S_SELF)
    names = [f"sbc_{k}" for k in range(DTH)] + ["hpd", "tarp"]
    print(f"rank KS per column = {dict(zip(names, ks.tolist()))} (critical {KS_BOUND:.4f})")
    if PARITY_OUT:
        json.dump({"observations": M_SELF, "num_samples": S_SELF, "bound": KS_BOUND,
                   "rank_ks_statistic": dict(zip(names, ks.tolist())),
                   "ties": int(cov.equal.sum())}, open(PARITY_OUT, "w"), indent=1)
    assert float(ks.max()) < KS_BOUND, ks


def test_leakage_correction_on_the_engine():
    x, th, x_o, th_o = _data(M_OBS)
    prior = _box(th, 0.3)
    post, twin = _post("ensemble", prior, x, th), _post("ensemble", prior, x, th)
    theta = th_o.clone()
    theta[:, 0] = prior.base_dist.low[0] + 0.5       # inside the box
    theta[1, 0] = prior.base_dist.low[0] - 0.5       # outside
    got = post.log_prob_batched(theta, x_o, leakage_correction=True, num_rejection_samples=512)
    frac = twin.support_fraction(x_o, 512)
    assert post._model.sample_counter == twin._model.sample_counter == DTH
    lp = twin.log_prob_batched(theta, x_o)
    print(f"support fractions = {frac.tolist()}")
    assert frac.shape == (M_OBS,) and frac.is_cuda and bool(((frac > 0) & (frac <= 1)).all())
    keep = torch.tensor([0, 2, 3], device="cuda")
    assert torch.equal(got[keep], (lp - torch.log(frac).to(lp.dtype))[keep])
    assert float(got[1]) == float("-inf")
    assert torch.equal(post.log_prob_batched(theta, x_o), lp)           # the default is unchanged
    given = post.log_prob_batched(theta, x_o, leakage_correction=True, support_fraction=frac)
    assert torch.equal(given, got) and post._model.sample_counter == DTH
