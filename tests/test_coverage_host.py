"""Coverage diagnostics on the CPU: rank_accumulate_host against brute-force loops, the rank
statistics, NPE_PFN_Core.coverage_batched on the numpy oracle as ``tabpfn.TabPFNRegressor`` (the
fixture pattern of tests/test_log_prob_batched_host.py), the orchestration-only checks and the
leakage correction of log_prob / log_prob_batched on a stub regressor that costs nothing, and the C
entry point's host-side argument checks."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from npe_pfn.diagnostics import (CoverageRanks, expected_coverage, rank_accumulate_host, rank_ks_statistic)
from oracle.tabpfn_oracle import OracleRegressor
from test_abi import declared_functions, declared_prototypes

N_CTX, DX, DTH, M, S = 60, 3, 2, 3, 8


# ------------------------------------------------------------------ rank_accumulate_host
def brute_counts(theta, logp, take, n_obs, per, theta_true, logp_true, ref, inv_scale, init=None):
    """The definition, one row and one column at a time, in numpy float64 / Python ints."""
    dim = theta.shape[1]
    counts = np.zeros((n_obs, dim + 2, 2), dtype=np.int64) if init is None else init.copy()
    for m in range(n_obs):
        for s in range(per):
            i = m * per + s
            if take is not None and not take[i]:
                continue
            for k in range(dim):
                counts[m, k, 0] += int(theta[i, k] < theta_true[m, k])
                counts[m, k, 1] += int(theta[i, k] == theta_true[m, k])
            if logp is not None:
                counts[m, dim, 0] += int(logp[i] > logp_true[m])
                counts[m, dim, 1] += int(logp[i] == logp_true[m])
            if ref is not None:
                d2 = d2t = np.float64(0.0)
                for k in range(dim):
                    a = (np.float64(theta[i, k]) - np.float64(ref[m, k])) * np.float64(inv_scale[k])
                    b = (np.float64(theta_true[m, k]) - np.float64(ref[m, k])) * np.float64(inv_scale[k])
                    d2 = d2 + a * a
                    d2t = d2t + b * b
                counts[m, dim + 1, 0] += int(d2 < d2t)
                counts[m, dim + 1, 1] += int(d2 == d2t)
    return counts


def grid_case(dim, n_obs=3, per=7, seed=0):
    """Multiples of 1/8 in a narrow range and power-of-two scales: ties really occur."""
    rng = np.random.default_rng(seed + dim)
    g = lambda *shape: (rng.integers(-4, 5, size=shape) / 8.0).astype(np.float32)  # noqa: E731
    c = dict(theta=g(n_obs * per, dim), logp=g(n_obs * per), take=rng.random(n_obs * per) < 0.7, n_obs=n_obs,
             per=per, theta_true=g(n_obs, dim), logp_true=g(n_obs), ref=g(n_obs, dim),
             inv_scale=(2.0 ** rng.integers(-2, 3, size=dim)).astype(np.float32))
    # every observation's first draw is its truth (and is taken): a tie in every column, whatever dim
    c["theta"][::per] = c["theta_true"]
    c["logp"][::per] = c["logp_true"]
    c["take"][::per] = True
    return c


def host_counts(c, init=None, **override):
    c = {**c, **override}
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a))  # noqa: E731
    counts = torch.zeros((c["n_obs"], c["theta"].shape[1] + 2, 2), dtype=torch.int64) if init is None \
        else torch.from_numpy(init.copy())
    rank_accumulate_host(t(c["theta"]), t(c["logp"]), t(c["take"]), c["n_obs"], c["per"], t(c["theta_true"]),
                         t(c["logp_true"]), t(c["ref"]), t(c["inv_scale"]), counts)
    return counts.numpy()


def brute(c, init=None, **override):
    c = {**c, **override}
    return brute_counts(c["theta"], c["logp"], c["take"], c["n_obs"], c["per"], c["theta_true"], c["logp_true"],
                        c["ref"], c["inv_scale"], init)


@pytest.mark.parametrize("dim", [1, 5])
def test_rank_accumulate_host_is_the_definition(dim):
    c = grid_case(dim)
    want = brute(c)
    assert want[:, :, 1].sum() > 0 and want[:, dim + 1, 1].sum() > 0, "the grid case has no ties"
    assert np.array_equal(host_counts(c), want)
    assert np.array_equal(host_counts(c, take=None), brute(c, take=None))
    # a nullable pair absent: its column keeps the caller's values
    init = np.arange(3 * (dim + 2) * 2, dtype=np.int64).reshape(3, dim + 2, 2) + 5
    no_lp = host_counts(c, init, logp=None, logp_true=None)
    assert np.array_equal(no_lp, brute(c, init, logp=None, logp_true=None))
    assert np.array_equal(no_lp[:, dim], init[:, dim])
    no_ref = host_counts(c, init, ref=None, inv_scale=None)
    assert np.array_equal(no_ref, brute(c, init, ref=None, inv_scale=None))
    assert np.array_equal(no_ref[:, dim + 1], init[:, dim + 1])


@pytest.mark.parametrize("dim", [1, 5])
def test_rank_accumulate_host_nan_counts_nowhere(dim):
    c = grid_case(dim)
    c["take"] = None
    clean = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c["theta"][3, 0] = np.nan
    c["logp"][3] = np.nan
    got = host_counts(c)
    assert np.array_equal(got, brute(c))
    # row 3 drops out of column 0, of the HPD column and (its distance is NaN) of the TARP column
    without = host_counts(clean, take=np.arange(3 * c["per"]) != 3)
    for col in (0, dim, dim + 1):
        assert np.array_equal(got[:, col], without[:, col])
    assert np.array_equal(got[:, 1:dim], host_counts(clean)[:, 1:dim])


@pytest.mark.parametrize("dim", [1, 5])
def test_two_calls_accumulate_to_the_concatenation(dim):
    a, b = grid_case(dim, per=7, seed=1), grid_case(dim, per=4, seed=2)
    for key in ("theta_true", "logp_true", "ref", "inv_scale"):
        b[key] = a[key]
    both = dict(a, per=11)
    for key, width in (("theta", dim), ("logp", None), ("take", None)):
        ra = a[key].reshape(3, 7, *([width] if width else []))
        rb = b[key].reshape(3, 4, *([width] if width else []))
        both[key] = np.concatenate([ra, rb], 1).reshape(33, *([width] if width else []))
    assert np.array_equal(host_counts(b, host_counts(a)), host_counts(both))
    assert np.array_equal(host_counts(both), brute(both))


def test_rank_accumulate_host_refuses_bad_shapes():
    c = grid_case(5)
    with pytest.raises(ValueError):
        host_counts(c, theta=c["theta"][:-1])
    with pytest.raises(ValueError):
        host_counts(c, logp=None)                       # half a pair
    with pytest.raises(ValueError):
        host_counts(c, inv_scale=None)
    with pytest.raises(ValueError):
        host_counts(c, theta_true=c["theta_true"][:, :4])
    with pytest.raises(ValueError):
        host_counts(c, take=c["take"][:-1])


# ------------------------------------------------------------------ statistics of ranks
def test_rank_ks_statistic():
    s = 9
    once = torch.arange(s + 1)
    assert float(rank_ks_statistic(once, s)) == 0.0
    assert float(rank_ks_statistic(torch.zeros(17, dtype=torch.int64), s)) == pytest.approx(s / (s + 1), abs=1e-15)
    both = rank_ks_statistic(torch.stack([once, torch.zeros(s + 1, dtype=torch.int64)], 1), s)
    assert both.shape == (2,) and float(both[0]) == 0.0 and float(both[1]) == pytest.approx(s / (s + 1), abs=1e-15)
    with pytest.raises(ValueError):
        rank_ks_statistic(torch.tensor([0, s + 1]), s)


def test_expected_coverage():
    s = 10
    ranks = torch.arange(s)
    levels = (torch.arange(s, dtype=torch.float64) + 1) / s
    lv, ecp = expected_coverage(ranks, s, levels)
    assert torch.equal(lv, levels) and torch.equal(ecp, levels)
    lv, ecp = expected_coverage(torch.stack([ranks, ranks], 1), s)
    assert lv.shape == (21,) and ecp.shape == (21, 2) and float(ecp[0].max()) == 0.0 and float(ecp[-1].min()) == 1.0


def test_coverage_ranks_views():
    less = torch.arange(12).reshape(3, 4)
    r = CoverageRanks(less, torch.ones_like(less), 20, torch.zeros(3), torch.zeros(3, 2), torch.ones(2))
    assert torch.equal(r.sbc_ranks, less[:, :2]) and torch.equal(r.hpd_ranks, less[:, 2])
    assert torch.equal(r.tarp_ranks, less[:, 3]) and torch.equal(r.midranks(), less.double() + 0.5)
    assert r.samples is None and r.sample_log_probs is None


# ------------------------------------------------------------------ coverage_batched on the oracle
@pytest.fixture(scope="module", autouse=True)
def oracle_as_tabpfn():
    from npe_pfn.weights import ModelConfig, synthetic_weights, weights_digest
    import npe_pfn.npe_pfn as mod

    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    cfg = ModelConfig(**meta["config"])
    w = synthetic_weights(cfg, seed=meta["weights_seed"])
    assert weights_digest(w, cfg) == meta["weights_digest"], "synthetic weight generator drifted from the fixtures"
    saved_w, saved_cls = OracleRegressor.default_weights, mod.TabPFNRegressor
    OracleRegressor.default_weights = w
    mod.TabPFNRegressor = OracleRegressor
    yield
    OracleRegressor.default_weights, mod.TabPFNRegressor = saved_w, saved_cls


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    theta = rng.normal(size=(N_CTX, DTH)).astype(np.float32)
    x = np.concatenate([theta + 0.3 * rng.normal(size=(N_CTX, DTH)), rng.normal(size=(N_CTX, DX - DTH))], 1)
    th_o = rng.normal(size=(M, DTH)).astype(np.float32)
    x_o = np.concatenate([th_o + 0.3 * rng.normal(size=(M, DTH)), rng.normal(size=(M, DX - DTH))], 1)
    return (torch.from_numpy(theta), torch.from_numpy(x.astype(np.float32)), torch.from_numpy(th_o),
            torch.from_numpy(x_o.astype(np.float32)))


def box_prior(theta_ctx):
    """Cuts dimension 0 at the context's median: about half of the sampler's draws fall outside."""
    low = torch.tensor([float(theta_ctx[:, 0].median()), -1e3])
    return torch.distributions.Independent(torch.distributions.Uniform(low, torch.full((DTH,), 1e3)), 1)


class StubRegressor:
    """The tabpfn surface the generic loop drives, at no cost: every conditional is uniform on the
    fitted column's range whatever the features are; draw c of the estimator comes from a torch
    generator seeded with c, so two stubs at the same counter draw the same numbers."""

    def __init__(self):
        self.sample_counter = 0

    def fit(self, X, y):
        y = torch.as_tensor(y)
        self.lo, self.hi = float(y.min()), float(y.max())
        return self

    def predict(self, X, output_type="full", quantiles=None):
        return {"logits": torch.zeros(len(X), 4), "criterion": StubCriterion(self, self.lo, self.hi)}


class StubCriterion:
    def __init__(self, reg, lo, hi):
        self.reg, self.lo, self.hi = reg, lo, hi

    def sample(self, logits):
        gen = torch.Generator().manual_seed(1000 + self.reg.sample_counter)
        self.reg.sample_counter += 1
        return self.lo + (self.hi - self.lo) * torch.rand(logits.shape[0], generator=gen)

    def __call__(self, logits, y):
        y = torch.as_tensor(y, dtype=torch.float32)
        return math.log(self.hi - self.lo) + 0.125 * (y - self.lo).abs()   # some NLL that varies with y


def make_core(data, prior, stub=False):
    """NPE_PFN_Core on the oracle (1 estimator: every fit and predict is a numpy transformer
    forward), or on the free stub for the tests that are about the orchestration alone."""
    from npe_pfn.npe_pfn import NPE_PFN_Core

    c = NPE_PFN_Core(prior=prior, regressor_init_kwargs={"random_state": 3, "preprocessing": "none",
                                                         "n_estimators": 1})
    if stub:
        c._model = StubRegressor()
    return c.append_simulations(data[0], data[1])


def ranks_of(samples, sample_lp, theta_true, lp_true, ref, inv_scale):
    m, s, d = samples.shape
    counts = torch.zeros((m, d + 2, 2), dtype=torch.int64)
    rank_accumulate_host(samples.reshape(m * s, d), sample_lp.reshape(-1), None, m, s, theta_true, lp_true, ref,
                         inv_scale, counts)
    return counts


@pytest.fixture(scope="module", params=["no prior", "box prior"])
def runs(request, data, oracle_as_tabpfn):
    prior = box_prior(data[0]) if request.param == "box prior" else None
    theta_true, x = data[2], data[3]
    core, twin = make_core(data, prior), make_core(data, prior)
    torch.manual_seed(5)
    cov = core.coverage_batched(theta_true, x, num_posterior_samples=S, return_samples=True)
    lp_true = twin.log_prob_batched(theta_true, x)
    samples, sample_lp = twin.sample_batched(x, (S,), with_log_prob=True)
    return dict(prior=prior, core=core, twin=twin, cov=cov, lp_true=lp_true, samples=samples, sample_lp=sample_lp)


def test_coverage_batched_is_log_prob_batched_plus_sample_batched_plus_ranks(runs, data):
    cov, theta_true = runs["cov"], data[2]
    assert cov.num_samples == S and cov.less.shape == cov.equal.shape == (M, DTH + 2)
    assert cov.less.dtype == cov.equal.dtype == torch.int64
    assert torch.equal(cov.log_prob_true, runs["lp_true"])
    assert cov.samples.shape == (M, S, DTH) and torch.equal(cov.samples, runs["samples"])
    assert torch.equal(cov.sample_log_probs, runs["sample_lp"])
    assert runs["core"]._model.sample_counter == runs["twin"]._model.sample_counter
    want = ranks_of(runs["samples"], runs["sample_lp"], theta_true, runs["lp_true"], cov.references, cov.inv_scale)
    assert torch.equal(cov.less, want[:, :, 0]) and torch.equal(cov.equal, want[:, :, 1])
    assert bool(((cov.less + cov.equal) <= S).all()) and int(cov.less.min()) >= 0
    span = data[0].max(0).values - data[0].min(0).values
    assert torch.equal(cov.inv_scale, 1.0 / span) and cov.references.shape == (M, DTH)
    if runs["prior"] is not None:
        assert bool(runs["prior"].support.check(cov.samples).all()) and bool(
            runs["prior"].support.check(cov.references).all())
        assert runs["core"]._model.sample_counter > DTH, "one round sufficed: the mask path was not exercised"
    else:
        lo, hi = data[0].min(0).values, data[0].max(0).values
        assert bool(((cov.references >= lo) & (cov.references <= hi)).all())


def test_without_return_samples_the_ranks_are_the_same_and_nothing_is_kept(runs, data):
    core, twin = make_core(data, runs["prior"], stub=True), make_core(data, runs["prior"], stub=True)
    ref = runs["cov"].references
    kept = twin.coverage_batched(data[2], data[3], num_posterior_samples=S, references=ref, return_samples=True)
    cov = core.coverage_batched(data[2], data[3], num_posterior_samples=S, references=ref)
    assert cov.samples is None and cov.sample_log_probs is None and kept.samples.shape == (M, S, DTH)
    assert torch.equal(cov.less, kept.less) and torch.equal(cov.equal, kept.equal)
    assert torch.equal(cov.references, ref) and torch.equal(cov.log_prob_true, kept.log_prob_true)
    want = ranks_of(kept.samples, kept.sample_log_probs, data[2], kept.log_prob_true, ref, kept.inv_scale)
    assert torch.equal(cov.less, want[:, :, 0]) and torch.equal(cov.equal, want[:, :, 1])


def test_two_blocks_are_sequential_sample_batched_calls(runs, data):
    """max_sampling_batch_size = 2 * int(S * 1.5): blocks of 2 and 1 observations."""
    theta_true, x = data[2], data[3]
    core, twin = make_core(data, runs["prior"]), make_core(data, runs["prior"])
    cov = core.coverage_batched(theta_true, x, num_posterior_samples=S, references=runs["cov"].references,
                                max_sampling_batch_size=2 * int(S * 1.5), return_samples=True)
    for a, b in ((0, 2), (2, 3)):
        lp_true = twin.log_prob_batched(theta_true[a:b], x[a:b])
        samples, sample_lp = twin.sample_batched(x[a:b], (S,), with_log_prob=True)
        assert torch.equal(cov.log_prob_true[a:b], lp_true)
        assert torch.equal(cov.samples[a:b], samples) and torch.equal(cov.sample_log_probs[a:b], sample_lp)
        want = ranks_of(samples, sample_lp, theta_true[a:b], lp_true, cov.references[a:b], cov.inv_scale)
        assert torch.equal(cov.less[a:b], want[:, :, 0]) and torch.equal(cov.equal[a:b], want[:, :, 1])
    assert core._model.sample_counter == twin._model.sample_counter


def test_coverage_batched_errors(runs, data):
    from npe_pfn.npe_pfn import TabPFN_Based_Uncond_Estimator

    core, theta_true, x = runs["core"], data[2], data[3]
    before = core._model.sample_counter
    bad = theta_true.clone()
    bad[1, 0] = float("nan")
    with pytest.raises(ValueError):
        core.coverage_batched(bad, x, num_posterior_samples=S)
    bad[1, 0] = float("inf")
    with pytest.raises(ValueError):
        core.coverage_batched(bad, x, num_posterior_samples=S)
    with pytest.raises(ValueError):
        core.coverage_batched(theta_true[:-1], x, num_posterior_samples=S)        # M mismatch
    with pytest.raises(ValueError):
        core.coverage_batched(theta_true[:, :1], x, num_posterior_samples=S)      # d_theta mismatch
    with pytest.raises(ValueError):
        core.coverage_batched(theta_true, x, num_posterior_samples=S, references=torch.zeros(M, DTH + 1))
    with pytest.raises(ValueError):
        core.coverage_batched(theta_true, x, num_posterior_samples=0)
    assert core._model.sample_counter == before
    with pytest.raises(NotImplementedError):
        TabPFN_Based_Uncond_Estimator().coverage_batched(torch.zeros(2, 2), torch.zeros(2, 1))


def test_short_observation_raises_after_ten_rounds(data):
    """A box no draw can reach: RuntimeError like sample_batched's, after 10 rounds of DTH counters."""
    prior = torch.distributions.Independent(torch.distributions.Uniform(torch.full((DTH,), 1e6),
                                                                        torch.full((DTH,), 2e6)), 1)
    core = make_core(data, prior, stub=True)
    with pytest.raises(RuntimeError):
        core.coverage_batched(data[2][:1], data[3][:1], num_posterior_samples=2, references=torch.zeros(1, DTH))
    assert core._model.sample_counter == 10 * DTH


# ------------------------------------------------------------------ leakage correction
def test_leakage_defaults_change_nothing(data):
    prior = box_prior(data[0])
    core, twin = make_core(data, prior, True), make_core(data, prior, True)
    theta, x = data[2], data[3]
    assert torch.equal(core.log_prob(theta, x[0]), twin.log_prob(theta, x[0], leakage_correction=False))
    assert torch.equal(core.log_prob_batched(theta, x),
                       twin.log_prob_batched(theta, x, leakage_correction=False, support_fraction=None))
    assert core._model.sample_counter == twin._model.sample_counter == 0


def test_leakage_correction_with_a_given_fraction(data):
    prior = box_prior(data[0])
    core = make_core(data, prior, stub=True)
    theta, x = data[2].clone(), data[3]
    theta[:, 0] = torch.tensor([5.0, -5.0, 6.0])          # rows 0 and 2 inside the box, row 1 outside
    f = 0.25
    lp = core.log_prob(theta, x[0])
    got = core.log_prob(theta, x[0], leakage_correction=True, support_fraction=f)
    assert torch.equal(got[[0, 2]], (lp - torch.tensor(math.log(f), dtype=torch.float64).to(lp.dtype))[[0, 2]])
    assert got[1] == float("-inf")
    fb = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64)
    lpb = core.log_prob_batched(theta, x)
    gotb, steps = core.log_prob_batched(theta, x, return_steps=True, leakage_correction=True, support_fraction=fb)
    assert torch.equal(gotb[[0, 2]], (lpb - torch.log(fb).to(lpb.dtype))[[0, 2]]) and gotb[1] == float("-inf")
    assert gotb[2] == lpb[2] and steps.shape == (M, DTH)
    assert core._model.sample_counter == 0               # a given fraction draws nothing


def test_support_fraction_and_the_estimated_correction(data):
    prior = box_prior(data[0])
    core, twin = make_core(data, prior, True), make_core(data, prior, True)
    theta, x = data[2].clone(), data[3]
    theta[:, 0] = 5.0
    frac = twin.support_fraction(x, num_draws=16)
    assert frac.shape == (M,) and frac.dtype == torch.float64 and twin._model.sample_counter == DTH
    draws = make_core(data, None, True).sample_batched(x, (16,))     # the same draws, unrejected
    assert torch.equal(frac, prior.support.check(draws).double().mean(1))
    assert bool((frac > 0).all()) and bool((frac < 1).any())
    got = core.log_prob_batched(theta, x, leakage_correction=True, num_rejection_samples=16)
    assert core._model.sample_counter == DTH
    lpb = twin.log_prob_batched(theta, x)
    assert torch.equal(got, lpb - torch.log(frac).to(lpb.dtype))
    # one observation: the context of sample(), 16 draws in calls of 10 and 6
    one = twin.support_fraction(x[0], num_draws=16, max_sampling_batch_size=10)
    assert one.shape == (1,) and twin._model.sample_counter == 3 * DTH
    got1 = core.log_prob(theta[:2], x[0], leakage_correction=True, num_rejection_samples=16)
    f1 = make_core(data, prior, True)
    f1._model.sample_counter = DTH                         # the counter `core` was at
    want = f1.log_prob(theta[:2], x[0]) - torch.log(f1.support_fraction(x[0], 16)).to(torch.float32)
    assert torch.equal(got1, want)


def test_leakage_correction_errors(data):
    prior = box_prior(data[0])
    core, bare = make_core(data, prior, True), make_core(data, None, True)
    theta, x = data[2], data[3]
    with pytest.raises(ValueError):
        core.log_prob(theta, x[0], mode="ratio_based", leakage_correction=True, support_fraction=0.5)
    with pytest.raises(ValueError):
        bare.log_prob(theta, x[0], leakage_correction=True, support_fraction=0.5)
    with pytest.raises(ValueError):
        bare.log_prob_batched(theta, x, leakage_correction=True)
    with pytest.raises(ValueError):
        bare.support_fraction(x)
    with pytest.raises(ValueError):
        core.log_prob(theta, x[0], leakage_correction=True, support_fraction=0.0)
    with pytest.raises(ValueError):
        core.log_prob_batched(theta, x, leakage_correction=True, support_fraction=torch.tensor([0.5, 0.0, 0.5]))
    with pytest.raises(ValueError):
        core.log_prob_batched(theta, x, leakage_correction=True, support_fraction=torch.tensor([0.5, 0.5]))
    with pytest.raises(ValueError):
        core.support_fraction(x, num_draws=0)
    assert core._model.sample_counter == 0 and bare._model.sample_counter == 0


# ------------------------------------------------------------------ the C entry point
def test_library_exports_rank_accumulate():
    from npe_pfn.engine import SIGNATURES, load_library

    lib = load_library()
    name = "npfn_rank_accumulate"
    assert name in declared_functions()
    assert hasattr(lib, name), f"{name} is not exported by libnpfn.so"
    assert name in SIGNATURES, f"{name} has no ctypes signature"
    assert len(declared_prototypes()[name]) == 12 and len(SIGNATURES[name][1]) == 12
    assert SIGNATURES[name][1][3:6] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]   # n_obs, per, dim
    assert SIGNATURES[name][1][10] == ctypes.c_void_p                                      # counts


def test_rank_accumulate_refuses_bad_arguments_before_any_launch():
    """The argument checks run on the host: no device is touched (the pointers are never read)."""
    from npe_pfn.engine import load_library

    lib = load_library()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = lib.npfn_rank_accumulate
    assert fn(p, p, None, -1, 4, 2, p, p, p, p, p, None) == -1      # n_obs < 0
    assert b"rank_accumulate" in lib.npfn_last_error()
    assert fn(p, p, None, 2, -1, 2, p, p, p, p, p, None) == -1      # per < 0
    assert fn(p, p, None, 2, 4, 0, p, p, p, p, p, None) == -1       # dim < 1
    assert fn(None, p, None, 2, 4, 2, p, p, p, p, p, None) == -1    # theta missing
    assert fn(p, p, None, 2, 4, 2, None, p, p, p, p, None) == -1    # theta_true missing
    assert fn(p, p, None, 2, 4, 2, p, p, p, p, None, None) == -1    # counts missing
    assert fn(p, p, None, 2, 4, 2, p, None, p, p, p, None) == -1    # half of the log density pair
    assert fn(p, None, None, 2, 4, 2, p, p, p, p, p, None) == -1
    assert fn(p, p, None, 2, 4, 2, p, p, None, p, p, None) == -1    # half of the reference pair
    assert fn(p, p, None, 2, 4, 2, p, p, p, None, p, None) == -1
    assert b"rank_accumulate" in lib.npfn_last_error()
    assert fn(None, None, None, 0, 4, 2, None, None, None, None, None, None) == 0    # nothing to do
    assert fn(None, None, None, 3, 0, 2, None, None, None, None, None, None) == 0
