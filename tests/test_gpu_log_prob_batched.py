"""GPU: TabPFN_Based_NPE_PFN.log_prob_batched / pit_batched on device tensors (the fused
npfn_ar_score path): shapes, bit-equality with Engine.ar_score, and agreement with one log_prob
call per observation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_CTX, DX, DTH, M, K = 200, 3, 2, 16, 3


@pytest.fixture(scope="module")
def setup():
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    rng = np.random.default_rng(17)
    theta = rng.normal(size=(N_CTX + M, DTH)).astype(np.float32)
    x = np.concatenate([theta + 0.3 * rng.normal(size=(N_CTX + M, DTH)), rng.normal(size=(N_CTX + M, DX - DTH))], 1)
    theta, x = torch.from_numpy(theta).cuda(), torch.from_numpy(x.astype(np.float32)).cuda()
    post = TabPFN_Based_NPE_PFN(regressor_init_kwargs={"random_state": 4, "device": "cuda:0"})
    post.append_simulations(theta[:N_CTX], x[:N_CTX])
    theta_o, x_o = theta[N_CTX:], x[N_CTX:]        # M true pairs
    lp, steps = post.log_prob_batched(theta_o, x_o, return_steps=True)
    return post, theta[:N_CTX], x[:N_CTX], theta_o, x_o, lp, steps


def test_shapes_and_devices(setup):
    post, _, _, theta_o, x_o, lp, steps = setup
    assert lp.shape == (M,) and steps.shape == (M, DTH) and lp.is_cuda and steps.is_cuda
    assert torch.isfinite(lp).all()
    only = post.log_prob_batched(theta_o, x_o)
    assert torch.equal(only, lp)
    th3 = torch.stack([theta_o, theta_o.flip(0), theta_o + 0.25], 1)
    lp3, st3 = post.log_prob_batched(th3, x_o, return_steps=True)
    assert lp3.shape == (M, K) and st3.shape == (M, K, DTH)
    assert torch.equal(st3[..., 0] + st3[..., 1], lp3)
    pit = post.pit_batched(theta_o, x_o)
    pit3 = post.pit_batched(th3, x_o)
    assert pit.shape == (M, DTH) and pit3.shape == (M, K, DTH) and pit.is_cuda
    assert bool(((pit >= 0) & (pit <= 1)).all()) and bool(((pit3 >= 0) & (pit3 <= 1)).all())
    # a CPU x gets its results on the CPU
    assert not post.log_prob_batched(theta_o.cpu(), x_o.cpu()).is_cuda


def test_bit_equal_to_engine_ar_score(setup):
    post, theta_c, x_c, theta_o, x_o, lp, steps = setup
    s, c = post._model.engine.ar_score(x_c, theta_c, x_o, theta_o)
    acc = torch.zeros(M, device="cuda")
    for k in range(DTH):
        acc += s[:, k]
    assert torch.equal(steps, s) and torch.equal(lp, acc)
    assert torch.equal(post.pit_batched(theta_o, x_o), c)
    th3 = torch.stack([theta_o, theta_o.flip(0), theta_o + 0.25], 1)
    s3, c3 = post._model.engine.ar_score(x_c, theta_c, x_o, th3.reshape(M * K, DTH))
    lp3, st3 = post.log_prob_batched(th3, x_o, return_steps=True)
    assert torch.equal(st3.reshape(M * K, DTH), s3)
    assert torch.equal(post.pit_batched(th3, x_o).reshape(M * K, DTH), c3)


def test_equals_looped_log_prob(setup):
    """One log_prob call per observation (the per-observation filter keeps all 200 rows, in its
    own order) against the batched pass: the d_rep tolerance of tests/test_gpu_preprocess.py --
    median 1e-2, 95th percentile 0.1."""
    post, _, _, theta_o, x_o, lp, _ = setup
    loop = torch.stack([post.log_prob(theta_o[m: m + 1], x_o[m])[0] for m in range(M)])
    d = (lp.cpu() - loop).abs().numpy()
    print(f"median |batched - looped| = {np.median(d):.3e}, 95th percentile = {np.quantile(d, 0.95):.3e}")
    assert np.median(d) <= 1e-2 and np.quantile(d, 0.95) <= 0.1, (np.median(d), np.quantile(d, 0.95))
