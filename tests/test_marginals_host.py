"""Posterior marginals on the CPU: PosteriorMarginals' arithmetic on hand-made bar distributions
(the fp64 host path of the summaries), NPE_PFN_Core.marginals through the generic dimension loop
with a stub regressor whose logits are known, and the C ABI of npfn_ar_marginals.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_abi import declared_functions, declared_prototypes

HM = 0.6744897501960817            # median of |N(0, 1)|
C = math.sqrt(2.0 / math.pi)       # mean of |N(0, 1)|


def _pm(probs, borders, **kw):
    from npe_pfn.marginals import PosteriorMarginals

    return PosteriorMarginals(torch.tensor(probs, dtype=torch.float32)[None, None],
                              torch.tensor(borders, dtype=torch.float32)[None], num_draws=1, **kw)


# ------------------------------------------------------------- hand-made bar distributions
def test_two_bars_closed_form():
    """Borders [0, 1, 3], masses [1/4, 3/4]: both bars are tail bars (half-normal means), the
    quantiles interpolate linearly."""
    pm = _pm([0.25, 0.75], [0.0, 1.0, 3.0])
    mean = 0.25 * (1.0 - (1.0 / HM) * C) + 0.75 * (1.0 + (2.0 / HM) * C)
    assert pm.mean().shape == (1, 1)
    assert abs(pm.mean().item() - mean) <= 1e-12
    assert abs(pm.median().item() - (1.0 + 2.0 / 3.0)) <= 1e-12
    iv = pm.interval(0.5)
    assert iv.shape == (1, 1, 2)
    assert abs(iv[0, 0, 0].item() - 1.0) <= 1e-12 and abs(iv[0, 0, 1].item() - (1.0 + 4.0 / 3.0)) <= 1e-12
    assert pm.mode().item() == 2.0      # densities 0.25 / 1 and 0.75 / 2: the centre of bar 1
    assert math.isnan(pm.support_fraction.item()) and pm.samples is None


def test_two_bars_mode_is_the_denser_bar():
    assert _pm([0.25, 0.75], [0.0, 1.0, 2.0]).mode().item() == 1.5    # 0.25 vs 0.75 per unit


def test_five_bars_closed_form():
    """Borders [-2, -1, 0, 1, 2, 4], masses [.1, .2, .4, .2, .1]."""
    pm = _pm([0.1, 0.2, 0.4, 0.2, 0.1], [-2.0, -1.0, 0.0, 1.0, 2.0, 4.0])
    mean = 0.1 * (-1.0 - (1.0 / HM) * C) + 0.2 * -0.5 + 0.4 * 0.5 + 0.2 * 1.5 + 0.1 * (2.0 + (2.0 / HM) * C)
    assert abs(pm.mean().item() - mean) <= 1e-7          # the masses are fp32 values
    assert abs(pm.median().item() - 0.5) <= 1e-7
    assert pm.quantile(0.5).item() == pm.median().item()
    iv = pm.interval(0.8)                                # the quantiles 0.1 and 0.9: the borders -1 and 2
    assert abs(iv[0, 0, 0].item() + 1.0) <= 1e-6 and abs(iv[0, 0, 1].item() - 2.0) <= 1e-6
    assert pm.mode().item() == 0.5
    q = pm.quantile([0.2, 0.5, 0.8])
    assert q.shape == (3, 1, 1)
    assert abs(q[0].item() + 0.5) <= 1e-6 and abs(q[2].item() - 1.5) <= 1e-6
    # pointwise: theta [d_theta], [M, d_theta] and [M, K, d_theta]
    assert abs(pm.cdf(torch.tensor([0.5])).item() - 0.5) <= 1e-7
    pts = torch.tensor([[[-0.5], [0.5], [1.5]]])
    np.testing.assert_allclose(pm.cdf(pts)[0, :, 0].numpy(), [0.2, 0.5, 0.8], atol=1e-7)
    np.testing.assert_allclose(pm.log_prob(pts)[0, :, 0].numpy(), np.log([0.2, 0.4, 0.2]), atol=1e-7)
    assert pm.cdf(torch.tensor([[0.5]])).shape == (1, 1) and pm.log_prob(pts).shape == (1, 3, 1)
    # the right tail bar: the half-normal density hanging right from 2
    s1 = 2.0 / HM
    want = math.log(0.1) + math.log(C / s1) - 1.0 / (2 * s1 * s1)
    assert abs(pm.log_prob(torch.tensor([3.0])).item() - want) <= 1e-6


def test_zero_mass_bars_are_never_returned():
    """Masses [.5, 0, 0, .5] on [0, 1, 2, 3, 4]: the median is the right border of bar 0, not a
    point of the empty bars; the CDF is flat over them and their log density is -inf."""
    pm = _pm([0.5, 0.0, 0.0, 0.5], [0.0, 1.0, 2.0, 3.0, 4.0])
    assert pm.median().item() == 1.0
    assert abs(pm.quantile(0.75).item() - 3.5) <= 1e-12
    assert pm.quantile(0.500001).item() > 3.0
    assert pm.quantile(0.0).item() == 0.0 and pm.quantile(1.0).item() == 4.0
    np.testing.assert_allclose(pm.cdf(torch.tensor([[[1.5], [2.5]]]))[0, :, 0].numpy(), [0.5, 0.5], atol=1e-12)
    assert pm.log_prob(torch.tensor([1.5])).item() == float("-inf")
    leading = _pm([0.0, 0.5, 0.5, 0.0], [0.0, 1.0, 2.0, 3.0, 4.0])
    assert leading.quantile(0.0).item() == 1.0           # bar 0 has no mass: the first bar that has


def test_bad_arguments():
    from npe_pfn.marginals import PosteriorMarginals

    with pytest.raises(ValueError):
        PosteriorMarginals(torch.ones(2, 3), torch.ones(3, 4), 1)
    with pytest.raises(ValueError):
        PosteriorMarginals(torch.ones(1, 2, 3), torch.ones(2, 3), 1)
    pm = _pm([0.5, 0.5], [0.0, 1.0, 2.0])
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError):
            pm.interval(bad)
    with pytest.raises(ValueError):
        pm.quantile(1.5)
    with pytest.raises(ValueError):
        pm.cdf(torch.zeros(1, 2))          # d_theta is 1


# ------------------------------------------------------------- marginals() with a stub regressor
NB = 12


class StubCriterion:
    def __init__(self, reg, borders):
        self._reg = reg
        self.borders = borders

    def sample(self, logits):
        """Deterministic 'draws' that differ by row and by call: the centre of the row's heaviest
        bar, moved by the row index and by the number of sample calls so far."""
        self._reg.n_samples += 1
        j = logits.argmax(1)
        mid = (self.borders[j] + self.borders[j + 1]) / 2
        return mid + 0.01 * torch.arange(logits.shape[0]) + 0.03 * self._reg.n_samples


class StubRegressor:
    """tabpfn's fit / predict surface with logits known in closed form: row i's logits peak at a
    bar chosen by the sum of its features; the borders widen with the number of features."""

    def __init__(self, **kwargs):
        self.n_samples = 0
        self.F = None

    def fit(self, X, y):
        self.F = X.shape[1]
        return self

    def predict(self, X, output_type="full", quantiles=None):
        assert output_type == "full" and X.shape[1] == self.F
        centre = (X.sum(1) * 1.7) % NB
        b = torch.arange(NB, dtype=torch.float32)
        logits = -((b[None, :] - centre[:, None]) ** 2) / (1.0 + 0.5 * self.F)
        borders = torch.linspace(-3.0 - self.F, 3.0 + self.F, NB + 1)
        return {"logits": logits, "criterion": StubCriterion(self, borders)}


@pytest.fixture()
def stub_core(monkeypatch):
    import npe_pfn.npe_pfn as mod

    monkeypatch.setattr(mod, "TabPFNRegressor", StubRegressor)
    rng = np.random.default_rng(5)
    theta = torch.from_numpy(rng.normal(size=(20, 2)).astype(np.float32))
    x = torch.from_numpy(rng.normal(size=(20, 3)).astype(np.float32))
    low, high = torch.tensor([-4.455, -2.0]), torch.tensor([5.615, 6.0])   # cuts the stub's first dimension
    prior = torch.distributions.Independent(torch.distributions.Uniform(low, high), 1)
    core = mod.NPE_PFN_Core(prior=prior)
    core.append_simulations(theta, x)
    return core, theta, x, (low, high)


def _expected(theta_ctx, x_ctx, x_obs, chunks):
    """The stub driven by hand: every row's softmax of every call, averaged over ALL rows of an
    observation at once (fp64) -- the definition, with no chunk weights in it."""
    reg = StubRegressor()
    joint = torch.cat([x_ctx, theta_ctx], 1)
    dx, dth, M = x_ctx.shape[1], theta_ctx.shape[1], x_obs.shape[0]
    rows = [[[] for _ in range(dth)] for _ in range(M)]
    draws = [[] for _ in range(M)]
    borders = []
    for d in chunks:
        feats = x_obs.repeat_interleave(d, 0)
        for k in range(dth):
            reg.fit(joint[:, : dx + k], joint[:, dx + k])
            pred = reg.predict(feats)
            p = torch.softmax(pred["logits"].double(), -1)
            for m in range(M):
                rows[m][k].append(p[m * d: (m + 1) * d])
            if len(borders) < dth:
                borders.append(pred["criterion"].borders)
            feats = torch.cat([feats, pred["criterion"].sample(pred["logits"])[:, None]], 1)
        for m in range(M):
            draws[m].append(feats[m * d: (m + 1) * d, dx:])
    probs = torch.stack([torch.stack([torch.cat(rows[m][k]).mean(0) for k in range(dth)]) for m in range(M)])
    naive = torch.stack([torch.stack([torch.stack([c.mean(0) for c in rows[m][k]]).mean(0) for k in range(dth)])
                         for m in range(M)])      # the unweighted mean of the calls' means
    return probs, torch.stack(borders), torch.stack([torch.cat(dr) for dr in draws]), naive


@pytest.mark.parametrize("n_obs,num_draws,cap,chunks", [
    (1, 7, 3, [3, 3, 1]),        # one observation, an unequal last call
    (1, 5, 10_000, [5]),         # one call
    (2, 5, 4, [2, 2, 1]),        # two observations: 4 // 2 = 2 draws each per call
])
def test_marginals_through_the_generic_loop(stub_core, n_obs, num_draws, cap, chunks):
    core, theta, x, (low, high) = stub_core
    x_obs = x[:n_obs] + 0.25
    pm = core.marginals(x_obs, num_draws=num_draws, max_sampling_batch_size=cap, return_samples=True)
    want_p, want_b, want_draws, naive = _expected(theta, x, x_obs, chunks)
    assert core._model.n_samples == 2 * len(chunks)
    assert pm.probs.shape == (n_obs, 2, NB) and pm.probs.dtype == torch.float32
    assert pm.borders.shape == (2, NB + 1) and torch.equal(pm.borders, want_b)
    assert pm.num_draws == num_draws
    assert torch.equal(pm.samples, want_draws)
    # fp64 sums in two different orders, rounded to fp32 once
    np.testing.assert_allclose(pm.probs.double().numpy(), want_p.numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(pm.probs.sum(-1).numpy(), 1.0, atol=1e-6)
    inside = ((want_draws >= low) & (want_draws <= high)).all(-1).sum(1).double() / num_draws
    assert pm.support_fraction.dtype == torch.float64 and torch.equal(pm.support_fraction, inside)
    assert 0.0 < float(inside.mean()) < 1.0              # the box cuts some of the draws, not all
    # a plain mean of the calls' means is NOT the answer when the last call is smaller
    if len(chunks) > 1:
        assert (naive - want_p).abs().max() > 1e-4
    # the summaries run on the host path
    assert pm.mean().shape == (n_obs, 2) and pm.interval(0.9).shape == (n_obs, 2, 2)
    med = pm.median()
    iv = pm.interval(0.9)
    assert (iv[..., 0] <= med).all() and (med <= iv[..., 1]).all()


def test_marginals_without_a_prior_and_flat_x(stub_core):
    core, theta, x, _ = stub_core
    core.prior = None
    pm = core.marginals(x[0], num_draws=3)               # x [dx]
    assert pm.probs.shape == (1, 2, NB) and pm.samples is None
    assert torch.isnan(pm.support_fraction).all()
    with pytest.raises(ValueError):
        core.marginals(x[0], num_draws=0)


def test_unconditional_estimator_and_process_groups(stub_core, monkeypatch):
    import npe_pfn.distributed as nd
    from npe_pfn.npe_pfn import TabPFN_Based_Uncond_Estimator

    with pytest.raises(NotImplementedError):
        TabPFN_Based_Uncond_Estimator().marginals(torch.zeros(1, 1))
    core, _, x, _ = stub_core
    assert nd.marginals_single_rank(core, x[:1], num_draws=2).probs.shape == (1, 2, NB)   # no group: one rank
    monkeypatch.setattr(nd, "_rank_world", lambda group=None: (0, 2))
    with pytest.raises(NotImplementedError, match="2 ranks"):
        nd.marginals_single_rank(core, x[:1], num_draws=2)


# ------------------------------------------------------------- the C ABI
def test_library_exports_ar_marginals():
    from npe_pfn.engine import SIGNATURES, load_library

    lib = load_library()
    name = "npfn_ar_marginals"
    assert name in declared_functions()
    assert hasattr(lib, name), f"{name} is not exported by libnpfn.so"
    assert name in SIGNATURES, f"{name} has no ctypes signature"
    proto = declared_prototypes()[name]
    assert len(proto) == 17
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert SIGNATURES[name][1] == [vp, vp, vp, i64, i32, i32, vp, i64, i64, ctypes.c_uint64, i64, vp, vp,
                                   ctypes.c_float, vp, vp, vp]
    # npfn_ar_sample_repeated's arguments with marg_out and borders_out in front of the stream
    rep = SIGNATURES["npfn_ar_sample_repeated"][1]
    assert SIGNATURES[name][1] == rep[:-1] + [vp, vp] + rep[-1:]


def test_bad_arguments_are_refused_before_any_launch():
    """n_unique, n_rows and the two new outputs are checked on the host before the engine is
    looked at: no device is touched (the engine handle is NULL here)."""
    from npe_pfn.engine import load_library

    lib = load_library()
    buf = (ctypes.c_float * 8)()
    out = ctypes.cast(buf, ctypes.c_void_p)

    def call(n_unique, n_rows, marg, borders):
        return lib.npfn_ar_marginals(None, None, None, 4, 1, 1, None, n_unique, n_rows, 0, 0, None, None, 1e-15,
                                     marg, borders, None)

    assert call(0, 4, out, out) == -1                     # n_unique < 1
    assert b"ar_marginals" in lib.npfn_last_error()
    assert call(3, 4, out, out) == -1                     # 3 does not divide 4
    assert call(4, 0, out, out) == -1                     # no rows to average
    assert call(2, 4, None, out) == -1                    # marg_out NULL
    assert b"marg_out" in lib.npfn_last_error()
    assert call(2, 4, out, None) == -1                    # borders_out NULL
    assert call(2, 4, out, out) == -1                     # all of that fine: the NULL engine is refused
    assert b"null engine" in lib.npfn_last_error()
