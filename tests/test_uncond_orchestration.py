"""TabPFN_Based_Uncond_Estimator's host orchestration vs the REFERENCE's own class.

tests/golden/make_golden_uncond.py ran the reference's TabPFN_Based_Uncond_Estimator (loaded by
path) with the oracle as ``tabpfn.TabPFNRegressor`` and the K13 restatement (tests/kmeans_ref.py)
as its ``KMeans``.  Here the build's class drives the same oracle (the generic estimator path,
host k-means): the same labels, the same fit/predict call log and the same numbers are required
under the same seeds (CPU, no GPU needed).  Tolerances: those of tests/test_orchestration.py.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.tabpfn_oracle import OracleRegressor


@pytest.fixture(scope="module", autouse=True)
def oracle_as_tabpfn():
    from npe_pfn.weights import ModelConfig, synthetic_weights, weights_digest
    import npe_pfn.npe_pfn as mod

    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    cfg = ModelConfig(**meta["config"])
    w = synthetic_weights(cfg, seed=meta["weights_seed"])
    assert weights_digest(w, cfg) == meta["weights_digest"], "synthetic weight generator drifted from the fixtures"
    saved_w, saved = OracleRegressor.default_weights, mod.TabPFNRegressor
    OracleRegressor.default_weights = w
    mod.TabPFNRegressor = OracleRegressor
    yield
    OracleRegressor.default_weights, mod.TabPFNRegressor = saved_w, saved


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "uncond.npz"))


def _fitted(g, num_clusters):
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    torch.manual_seed(int(g["torch_seed"]))
    np.random.seed(int(g["numpy_seed"]))
    est = TabPFN_Based_Uncond_Estimator(num_clusters=num_clusters,
                                        regressor_init_kwargs={"random_state": int(g["random_state"])})
    return est.append_simulations(torch.from_numpy(g["theta"]))


@pytest.mark.parametrize("case,num_clusters", [("k3", 3), ("k1", 1)])
def test_reproduces_the_reference_class(golden, case, num_clusters):
    g = golden
    est = _fitted(g, num_clusters)
    np.testing.assert_array_equal(est._theta_train.numpy(), g[f"{case}_theta_perm"])
    np.testing.assert_array_equal(est._x_train.numpy(), g[f"{case}_x_dummy"])
    np.testing.assert_array_equal(est.kmeans.labels_.numpy(), g[f"{case}_labels"])
    np.testing.assert_array_equal(est.counts, g[f"{case}_counts"])
    n = int(g["n_samples"])
    s, lp = est.sample(torch.Size([n, 1]), with_log_prob=True)
    assert s.shape == (n, 2) and lp.shape == (n,) and est.cluster_state == 0
    np.testing.assert_allclose(s.numpy(), g[f"{case}_samples"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(lp.numpy(), g[f"{case}_log_probs"], rtol=2e-5, atol=2e-5)
    lp2 = est.log_prob(torch.from_numpy(g[f"{case}_samples"]))
    np.testing.assert_allclose(lp2.numpy(), g[f"{case}_log_prob_of_samples"], rtol=2e-5, atol=2e-5)
    calls = [[c[0], list(c[1]), c[2] if not isinstance(c[2], tuple) else list(c[2])] for c in est._model.calls]
    assert calls == json.loads(str(g[f"{case}_calls"]))


def test_fixture_draws_come_from_their_clusters(golden):
    """The fixture's own record: every draw of the three-blob case lies in the blob of the
    cluster it was drawn for (the blobs are 7 apart, the draws within ~2 of their centre)."""
    import kmeans_ref

    g = golden
    np.testing.assert_array_equal(kmeans_ref.assign(g["k3_samples"], g["k3_centers"]), g["k3_sample_cluster"])


def test_one_cluster_per_row_is_refused():
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    theta = torch.arange(12, dtype=torch.float32).reshape(6, 2) ** 2
    with pytest.raises(AssertionError, match="Too few samples"):
        TabPFN_Based_Uncond_Estimator(num_clusters=6).append_simulations(theta)


def test_non_finite_thetas_are_refused():
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    theta = torch.randn(10, 2)
    theta[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        TabPFN_Based_Uncond_Estimator().append_simulations(theta)


def test_ratio_based_is_not_provided(golden):
    est = _fitted(golden, 1)
    with pytest.raises(NotImplementedError, match="ratio_based"):
        est.log_prob(torch.zeros(3, 2), mode="ratio_based")
    with pytest.raises(ValueError, match="Invalid mode"):
        est.log_prob(torch.zeros(3, 2), mode="something")


def test_pickle_round_trip(golden):
    est = _fitted(golden, 3)
    est2 = pickle.loads(pickle.dumps(est))
    assert est2._model is not None and est2._model is not est._model
    assert torch.equal(est2._theta_train, est._theta_train) and torch.equal(est2._x_train, est._x_train)
    assert torch.equal(est2.kmeans.labels_, est.kmeans.labels_) and torch.equal(est2.kmeans.centers, est.kmeans.centers)
    np.testing.assert_array_equal(est2.counts, est.counts)
    q = torch.from_numpy(golden["k3_samples"][:7])
    assert torch.equal(est2.kmeans.predict(q), est.kmeans.predict(q))
    assert est2.context_size == 10_000 and est2.num_clusters == 3


def test_public_name():
    import npe_pfn
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    assert "TabPFN_Based_Uncond_Estimator" in npe_pfn.__all__
    est = TabPFN_Based_Uncond_Estimator.__new__(TabPFN_Based_Uncond_Estimator)
    assert isinstance(est, npe_pfn.NPE_PFN_Core)
    for name in ("set_cluster_state", "get_context", "append_simulations", "sample", "log_prob"):
        assert callable(getattr(TabPFN_Based_Uncond_Estimator, name))
