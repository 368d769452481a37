"""TabPFN_Based_Uncond_Estimator on the GPU: device k-means (K13) + the fused AR sampler.

* paired draws against tests/golden/uncond.npz (the reference's class driving the CPU oracle,
  tests/golden/make_golden_uncond.py) under the same seeds and random_state: labels and counts
  equal exactly; per cluster and dimension median |theta_gpu - theta_ref| <= 2 % of that
  cluster's golden std; median |delta log-prob| <= 0.05 for the sampled log-probs and for
  log_prob() of the golden draws (the paired bounds of tests/test_gpu_posterior.py);
* the reference's own parametrised cases (reference tests/test_npe_pfn.py:279-317), restated;
* routing: draws land in populated clusters, and log_prob of a batch is the concatenation of
  per-cluster calls made by hand.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "uncond.npz"))


def _estimator(num_clusters, random_state=0):
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    return TabPFN_Based_Uncond_Estimator(num_clusters=num_clusters,
                                         regressor_init_kwargs={"random_state": random_state, "device": DEV})


@pytest.mark.parametrize("case,num_clusters", [("k3", 3), ("k1", 1)])
def test_paired_draws_match_reference(golden, case, num_clusters):
    g = golden
    torch.manual_seed(int(g["torch_seed"]))
    np.random.seed(int(g["numpy_seed"]))
    est = _estimator(num_clusters, int(g["random_state"]))
    est.append_simulations(torch.from_numpy(g["theta"]).to(DEV))
    assert est.kmeans.labels_.is_cuda and est.kmeans.centers.is_cuda
    np.testing.assert_array_equal(est._theta_train.cpu().numpy(), g[f"{case}_theta_perm"])
    np.testing.assert_array_equal(est.kmeans.labels_.cpu().numpy(), g[f"{case}_labels"])
    np.testing.assert_array_equal(est.counts, g[f"{case}_counts"])
    n = int(g["n_samples"])
    s, lp = est.sample(torch.Size([n, 1]), with_log_prob=True)
    assert s.shape == (n, 2) and lp.shape == (n,)
    s, lp = s.cpu().numpy(), lp.cpu().numpy()
    ref, ref_lp, cluster = g[f"{case}_samples"], g[f"{case}_log_probs"], g[f"{case}_sample_cluster"]
    for c in range(num_clusters):
        m = cluster == c
        med = np.median(np.abs(s[m] - ref[m]), 0)
        sd = ref[m].std(0)
        print(f"{case} cluster {c}: {int(m.sum())} draws, median |gpu - ref| {med}, 2 % of std {0.02 * sd}")
        assert (med <= 0.02 * sd).all(), (c, med, sd)
    d_lp = np.median(np.abs(lp - ref_lp))
    lp2 = est.log_prob(torch.from_numpy(ref).to(DEV)).cpu().numpy()
    d_lp2 = np.median(np.abs(lp2 - g[f"{case}_log_prob_of_samples"]))
    print(f"{case}: median |delta log-prob| sampled {d_lp:.4f}, log_prob(golden draws) {d_lp2:.4f}")
    assert d_lp <= 0.05, d_lp
    assert d_lp2 <= 0.05, d_lp2


@pytest.mark.parametrize("n_samples,n_posterior,feature_dim,num_clusters",
                         [(10, 100, 1, 1), (10, 100, 3, 1), (1000, 1000, 4, 5), (2000, 12000, 5, 1),
                          (2000, 12000, 5, 3)])
def test_sampling_and_log_prob_unconditional_TabPFN(n_samples, n_posterior, feature_dim, num_clusters):
    torch.manual_seed(n_samples + feature_dim + num_clusters)
    np.random.seed(0)
    theta = torch.distributions.Normal(torch.zeros(feature_dim), torch.ones(feature_dim)).sample((n_samples,))
    est = _estimator(num_clusters)
    est.append_simulations(theta.to(DEV))
    theta_posterior = est.sample(sample_shape=torch.Size([n_posterior, 1]), max_sampling_batch_size=10_000)
    assert theta_posterior.shape == (n_posterior, feature_dim)
    log_prob = est.log_prob(theta_posterior)
    assert log_prob.shape == torch.Size([n_posterior])
    assert not torch.isnan(log_prob).any()
    assert not torch.isinf(log_prob).any()


def test_routing_of_draws_and_log_prob():
    torch.manual_seed(5)
    np.random.seed(5)
    which = torch.arange(600) % 3
    centres = torch.tensor([[-6.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 9.0, 0.0]])
    theta = (centres[which] + torch.randn(600, 3)).to(DEV)
    est = _estimator(3, random_state=2)
    est.append_simulations(theta)
    draws = est.sample(torch.Size([500, 1]))
    assert draws.device == theta.device and est.cluster_state == 0
    labels = est.kmeans.predict(draws, engine=est._model.engine).cpu().numpy()
    assert (est.counts[labels] > 0).all()
    # log_prob of a mixed batch = the per-cluster calls made by hand, under the same dummy-x draws
    batch = est._theta_train[:200]
    lab = est.kmeans.predict(batch, engine=est._model.engine).cpu()
    assert len(set(lab.tolist())) == 3
    torch.manual_seed(11)
    whole = est.log_prob(batch)
    torch.manual_seed(11)
    by_hand = torch.zeros(batch.shape[0])
    log_w = np.log(est.counts / est.counts.sum())
    for c in range(3):
        est.set_cluster_state(c)
        rows = (lab == c).nonzero(as_tuple=True)[0]
        part = est._autoregressive_log_prob(batch[rows.to(DEV)], torch.randn(rows.numel(), 1), repeat_x=False)
        by_hand[rows] = part.cpu() + float(log_w[c])
    est.set_cluster_state()
    # the same kernels on the same inputs, with (log_prob) and without (by hand) a fit token:
    # a few fp32 roundings of a log density of magnitude ~10 at the most
    assert torch.isfinite(whole).all()
    torch.testing.assert_close(whole, by_hand, rtol=1e-5, atol=1e-5)
