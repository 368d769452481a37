"""Golden vectors of the unconditional estimator: the REFERENCE's TabPFN_Based_Uncond_Estimator
driving the oracle, with its ``KMeans`` replaced by the K13 restatement (tests/kmeans_ref.py).

Run on the development machine only (the reference is not on the GPU box):

    python tests/golden/make_golden_uncond.py

The reference module is loaded by path as in make_golden.py; its module-level name ``KMeans``
(sklearn's, unseeded in the reference) is replaced by ``kmeans_ref.KMeansShim`` seeded with the
regressor's ``random_state``, which is the clustering the build's class runs.  The reference then
makes its own sequence of host draws (randperm, randn, multinomial) under fixed
``torch.manual_seed`` / ``np.random.seed``; the multinomial counts and the final permutation
are recorded on the way, so that the fixture can say which cluster every draw came from.
Writes tests/golden/uncond.npz (two cases: ``k3_*`` and ``k1_*``; model table and weights of
tests/golden/meta.json).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import OracleRegressor, _load_weights_module, install_reference  # noqa: E402

import kmeans_ref  # noqa: E402

RANDOM_STATE = 6
TORCH_SEED = 2025
NUMPY_SEED = 77
N_THETA = 150
N_SAMPLES = 300
BLOB_CENTRES = np.array([[-4.0, 0.0], [4.0, 1.0], [0.0, 6.0]], dtype=np.float32)


def blob_thetas() -> torch.Tensor:
    """150 thetas in 2-D: three blobs of 50 (std 0.5) around BLOB_CENTRES, interleaved."""
    rng = np.random.default_rng(11)
    which = np.arange(N_THETA) % 3
    return torch.from_numpy((BLOB_CENTRES[which] + 0.5 * rng.standard_normal((N_THETA, 2))).astype(np.float32))


def run_case(ref, theta: torch.Tensor, num_clusters: int) -> dict:
    rec = {}
    real_multinomial, real_randperm = np.random.multinomial, torch.randperm

    def multinomial(n, p):
        rec["per_cluster"] = real_multinomial(n, p)
        return rec["per_cluster"]

    def randperm(n, *a, **kw):
        rec["perm"] = real_randperm(n, *a, **kw)
        return rec["perm"]

    torch.manual_seed(TORCH_SEED)
    np.random.seed(NUMPY_SEED)
    est = ref.TabPFN_Based_Uncond_Estimator(num_clusters=num_clusters,
                                            regressor_init_kwargs={"random_state": RANDOM_STATE})
    est.append_simulations(theta)
    np.random.multinomial, ref.torch.randperm = multinomial, randperm
    try:
        s, lp = est.sample(torch.Size([N_SAMPLES, 1]), with_log_prob=True)
    finally:
        np.random.multinomial, ref.torch.randperm = real_multinomial, real_randperm
    lp_of_samples = est.log_prob(s)
    cluster = np.repeat(np.arange(num_clusters), rec["per_cluster"])[rec["perm"].numpy()]
    return dict(theta_perm=est._theta_train.numpy(), x_dummy=est._x_train.numpy(),
                labels=est.kmeans.labels_.astype(np.int64), counts=np.asarray(est.counts, dtype=np.int64),
                centers=est.kmeans.cluster_centers_, samples=s.numpy(), log_probs=lp.numpy(),
                sample_cluster=cluster.astype(np.int64), log_prob_of_samples=lp_of_samples.numpy(),
                calls=json.dumps(est._model.calls))


def main():
    W = _load_weights_module()
    meta = json.load(open(os.path.join(HERE, "meta.json")))
    cfg = W.ModelConfig(**meta["config"])
    OracleRegressor.default_weights = W.synthetic_weights(cfg, seed=meta["weights_seed"])
    assert W.weights_digest(OracleRegressor.default_weights, cfg) == meta["weights_digest"], \
        "the weights are not those of tests/golden/meta.json"
    mods, _ = install_reference()
    ref = mods["npe_pfn"]
    kmeans_ref.KMeansShim.seed = RANDOM_STATE
    ref.KMeans = kmeans_ref.KMeansShim
    theta = blob_thetas()
    out = dict(theta=theta.numpy(), random_state=RANDOM_STATE, torch_seed=TORCH_SEED, numpy_seed=NUMPY_SEED,
               n_samples=N_SAMPLES)
    for name, k in (("k3", 3), ("k1", 1)):
        for key, val in run_case(ref, theta, k).items():
            out[f"{name}_{key}"] = val
    np.savez_compressed(os.path.join(HERE, "uncond.npz"), **out)
    print("wrote uncond.npz:", {k: getattr(v, "shape", v) for k, v in out.items() if not k.endswith("calls")})


if __name__ == "__main__":
    main()
