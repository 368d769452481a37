"""NPE_PFN_Core.log_prob_batched / pit_batched on the CPU: the build's orchestration drives the
numpy oracle as ``tabpfn.TabPFNRegressor`` (as tests/test_orchestration.py does) through the
generic dimension loop -- the path of every estimator without a fused ``ar_score``."""
import json
import os

import numpy as np
import pytest
import torch

from bar_cdf_ref import bar_cdf_ref
from conftest import GOLDEN
from oracle.tabpfn_oracle import OracleRegressor

N_CTX, DX, DTH, M = 60, 3, 2, 5


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


@pytest.fixture(scope="module")
def core(data, oracle_as_tabpfn):
    from npe_pfn.npe_pfn import NPE_PFN_Core

    c = NPE_PFN_Core(regressor_init_kwargs={"random_state": 3, "preprocessing": "none"})
    c.append_simulations(data[0], data[1])
    return c


@pytest.fixture(scope="module")
def flat(core, data):
    """One log_prob_batched call over the M pairs, with its steps and the oracle's call record."""
    core._model.calls.clear()
    lp, steps = core.log_prob_batched(data[2], data[3], return_steps=True)
    return lp, steps, list(core._model.calls)


def test_equals_log_prob_row_by_row(core, data, flat):
    """rtol = atol = 2e-5, the golden tests' tolerance: numpy matmuls are not row-batch-invariant."""
    lp, _, _ = flat
    assert lp.shape == (M,)
    for m in range(M):
        one = core.log_prob(data[2][m: m + 1], data[3][m])
        np.testing.assert_allclose(lp[m].item(), one.item(), rtol=2e-5, atol=2e-5)


def test_one_fit_and_one_predict_per_dimension(flat):
    _, _, calls = flat
    assert [c[0] for c in calls] == ["fit", "predict"] * DTH
    assert [c[1] for c in calls if c[0] == "fit"] == [(N_CTX, DX + k) for k in range(DTH)]
    assert [c[1] for c in calls if c[0] == "predict"] == [(M, DX + k) for k in range(DTH)]


def test_return_steps_sums_to_the_total(core, data, flat):
    lp, steps, _ = flat
    assert steps.shape == (M, DTH)
    acc = torch.zeros(M)
    for k in range(DTH):
        acc += steps[:, k]
    assert torch.equal(acc, lp)


def test_three_dimensional_theta_is_the_flat_form_on_repeated_rows(core, data, flat):
    theta, x = data[2], data[3]
    th3 = torch.stack([theta, theta.flip(0), theta + 0.25], 1)   # [M, 3, DTH]
    core._model.calls.clear()
    lp3, st3 = core.log_prob_batched(th3, x, return_steps=True)
    assert lp3.shape == (M, 3) and st3.shape == (M, 3, DTH)
    assert [c[1] for c in core._model.calls if c[0] == "predict"] == [(3 * M, DX + k) for k in range(DTH)]
    lpf, stf = core.log_prob_batched(th3.reshape(3 * M, DTH), x.repeat_interleave(3, 0), return_steps=True)
    np.testing.assert_allclose(lp3.reshape(-1).numpy(), lpf.numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(st3.reshape(-1, DTH).numpy(), stf.numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(lp3[:, 0].numpy(), flat[0].numpy(), rtol=2e-5, atol=2e-5)


def test_pit_batched_is_the_restatement_step_by_step(core, data):
    theta_ctx, x_ctx, theta, x = data
    core._model.calls.clear()
    pit = core.pit_batched(theta, x)
    assert pit.shape == (M, DTH)
    assert [c[0] for c in core._model.calls] == ["fit", "predict"] * DTH
    joint = torch.cat([x_ctx, theta_ctx], 1)
    test = torch.cat([x, theta], 1)
    reg = core._model
    for k in range(DTH):
        reg.fit(joint[:, : DX + k], joint[:, DX + k])
        pred = reg.predict(test[:, : DX + k], output_type="full", quantiles=[])
        ref = bar_cdf_ref(pred["logits"].numpy(), pred["criterion"].borders, theta[:, k].numpy())
        assert np.abs(pit[:, k].numpy() - ref).max() <= 1e-12
    assert float(pit.min()) >= 0.0 and float(pit.max()) <= 1.0


def test_bad_shapes_raise(core, data):
    theta, x = data[2], data[3]
    for fn in (core.log_prob_batched, core.pit_batched):
        with pytest.raises(ValueError):
            fn(theta[:-1], x)                      # M mismatch
        with pytest.raises(ValueError):
            fn(theta[0], x)                        # theta.ndim == 1
        with pytest.raises(ValueError):
            fn(theta[:, None, None, :], x)         # theta.ndim == 4
        with pytest.raises(ValueError):
            fn(torch.stack([theta, theta], 1)[:-1], x)


def test_unconditional_estimator_has_no_batched_scores(oracle_as_tabpfn):
    from npe_pfn.npe_pfn import TabPFN_Based_Uncond_Estimator

    est = TabPFN_Based_Uncond_Estimator()
    with pytest.raises(NotImplementedError):
        est.log_prob_batched(torch.zeros(2, 2), torch.zeros(2, 1))
    with pytest.raises(NotImplementedError):
        est.pit_batched(torch.zeros(2, 2), torch.zeros(2, 1))
