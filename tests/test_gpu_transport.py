"""GPU: npfn_w2_assign against its host definition (assignment_solve_host on transport_costs_host's
integer costs) bit for bit where the definition is quick enough, against the dual certificates and
scipy's optimal cost where it is not, its return codes and refusals, and
NPE_PFN_Core.wasserstein_batched on a tiny fitted estimator.

The block-size rule of npfn_transport.hip is the smallest power of two of threads in 64..1024 that
is >= n / 2 (two columns per thread): the exact cases cross 1 -> 2 columns per thread at n = 64 | 65
and 64 -> 128 -> 256 threads at n = 128 | 129 and 256 | 257, the certificate cases 512 -> 1024
threads at n = 1024 | 1025.  a stays in LDS beside b while both fit in 159 KiB: at the cap n = 2048
that holds for d = 2 and not for d = 16.
"""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from npe_pfn.diagnostics import (assignment_solve_host, transport_costs_host, transport_scale,
                                 wasserstein_batched)

pytestmark = pytest.mark.gpu

N_CTX, DX, DTH = 150, 3, 3   # the estimator shapes of tests/test_gpu_two_sample.py
SEED = 2


def draws(n, d, M=1, seed=0, shift=0.5):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + d)
    return torch.randn(M, n, d, generator=g), torch.randn(M, n, d, generator=g) + shift


def tie_grid(n, M=1, seed=0):
    """Points on an 8 x 8 integer grid: many equal costs and many zeros."""
    g = torch.Generator().manual_seed(seed + n)
    return (torch.randint(0, 8, (M, n, 2), generator=g).float(), torch.randint(0, 8, (M, n, 2), generator=g).float())


def ladder(n):
    a = torch.arange(float(n))[None, :, None]
    return a, a + n // 2


def gpu_assign(a, b, scale=None):
    from npe_pfn.engine import w2_assign

    a, b = a.cuda(), b.cuda()
    scale = transport_scale(a, b)[0] if scale is None else scale.cuda()
    return tuple(t.cpu() for t in w2_assign(a, b, scale))


def certify(cq, assign, duals, cost_sum):
    """The dual certificate of optimality, on the host's integer costs."""
    M, n, _ = cq.shape
    for m in range(M):
        u, v = duals[m, 0], duals[m, 1]
        assert bool((u[:, None] + v[None, :] <= cq[m]).all()), m
        assert int(u.sum() + v.sum()) == int(cost_sum[m]), m
        asg = assign[m].to(torch.int64)
        assert sorted(asg.tolist()) == list(range(n)), m
        assert int(cq[m][torch.arange(n), asg].sum()) == int(cost_sum[m]), m


def check_exact(a, b, what):
    cq, scale, bad = transport_costs_host(a, b)
    assert int(bad.sum()) == 0, what
    want = assignment_solve_host(cq)
    got = gpu_assign(a, b, scale)
    assert got[0].dtype == torch.int32 and all(t.dtype == torch.int64 for t in got[1:4]), what
    assert got[4].tolist() == [0] * a.shape[0], (what, got[4])
    for name, g, w in zip(("assign", "duals", "cost_sum", "steps"), got, want):
        assert torch.equal(g, w), (what, name)
    certify(cq, got[0], got[1], got[2])
    return got


# ------------------------------------------------------------------ device == definition, exactly
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 256, 257])
def test_equals_the_definition_d3(n):
    a, b = draws(n, 3, M=2)
    _, _, _, steps, _ = check_exact(a, b, n)
    assert bool((steps >= n).all()) and bool((steps <= n * (n + 1) // 2).all())


@pytest.mark.parametrize("d", [1, 64])
def test_equals_the_definition_n512(d):
    check_exact(*draws(512, d), (512, d))


def test_equals_the_definition_on_the_tie_grid():
    check_exact(*tie_grid(256, M=2), "grid")


def test_ladder_takes_the_full_step_bound():
    a, b = ladder(256)
    _, _, cost_sum, steps, _ = check_exact(a, b, "ladder")
    assert steps.tolist() == [256 * 257 // 2]
    r = wasserstein_batched(a.cuda(), b.cuda())
    assert r.wasserstein.tolist() == [128.0] and r.steps.tolist() == [256 * 257 // 2]


def test_row_permutation_costs_nothing():
    a, _ = draws(257, 3, M=2, seed=3)
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(1))
    b = a[:, perm]
    assign, _, cost_sum, _, _ = check_exact(a, b, "perm")
    assert cost_sum.tolist() == [0, 0]
    assert torch.equal(perm[assign[0].to(torch.int64)], torch.arange(257))


# ------------------------------------------------------------------ certificates and scipy's optimum
@pytest.mark.parametrize("n,d", [(1000, 10), (1024, 4), (1025, 4), (2048, 2), (2048, 16)])
def test_certificates_and_scipy_cost(n, d):
    a, b = draws(n, d)
    cq, scale, bad = transport_costs_host(a, b)
    assign, duals, cost_sum, steps, gbad = gpu_assign(a, b, scale)
    assert gbad.tolist() == [0] and bad.tolist() == [0]
    certify(cq, assign, duals, cost_sum)
    c = cq[0].numpy()
    rows, cols = linear_sum_assignment(c)
    assert int(c[rows, cols].sum()) == int(cost_sum[0])
    assert n <= int(steps[0]) <= n * (n + 1) // 2
    print(f"n={n} d={d}: steps {int(steps[0])} of at most {n * (n + 1) // 2}")


# ------------------------------------------------------------------ reproducibility, return codes
def test_same_bits_alone_among_others_and_twice():
    a, b = draws(129, 3, M=5, seed=5)
    once, twice = gpu_assign(a, b), gpu_assign(a, b)
    assert all(torch.equal(x, y) for x, y in zip(once, twice))
    for m in range(5):
        alone = gpu_assign(a[m: m + 1], b[m: m + 1])
        assert all(torch.equal(x[0], y[m]) for x, y in zip(alone, once)), m


def test_nan_marks_its_observation_only():
    a, b = draws(65, 3, M=3, seed=6)
    clean = gpu_assign(a, b)
    a[1, 64, 2] = float("nan")
    got = gpu_assign(a, b)
    assert got[4].tolist() == [0, 1, 0]
    for m in (0, 2):
        assert all(torch.equal(x[m], y[m]) for x, y in zip(got, clean)), m
    r = wasserstein_batched(a.cuda(), b.cuda())
    assert torch.isnan(r.wasserstein).tolist() == [False, True, False]
    assert bool((r.assignment[1] == -1).all()) and sorted(r.assignment[0].tolist()) == list(range(65))
    _, _, hbad = transport_costs_host(a, b)
    assert hbad.tolist() == [0, 1, 0]
    b[2, 0, 0] = float("inf")
    assert gpu_assign(a, b)[4].tolist() == [0, 1, 1]


def test_too_large_scale_is_a_return_code():
    a, b = draws(65, 3, M=3, seed=7)
    scale = transport_scale(a, b)[0]
    clean = gpu_assign(a, b, scale)
    big = scale.clone()
    big[1] = big[1] * 2.0 ** 8
    got = gpu_assign(a, b, big)
    assert got[4].tolist() == [0, 2, 0]
    for m in (0, 2):
        assert all(torch.equal(x[m], y[m]) for x, y in zip(got, clean)), m


def test_rejected_arguments():
    from npe_pfn.engine import load_library

    lib = load_library()
    a = torch.zeros((2, 8, 3), device="cuda")
    scale = torch.ones(2, dtype=torch.float64, device="cuda")
    assign = torch.full((2, 8), 7, dtype=torch.int32, device="cuda")
    duals = torch.full((2, 2, 8), 7, dtype=torch.int64, device="cuda")
    cost_sum = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    steps = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    bad = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    good = dict(a=a.data_ptr(), b=a.data_ptr(), n_obs=2, n=8, dim=3, scale=scale.data_ptr(), assign=assign.data_ptr(),
                duals=duals.data_ptr(), cost_sum=cost_sum.data_ptr(), steps=steps.data_ptr(), bad=bad.data_ptr())

    def call(**kw):
        g = dict(good, **kw)
        vp = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
        ip = lambda p: ctypes.cast(vp(p), ctypes.POINTER(ctypes.c_int32)) if p else None  # noqa: E731
        rc = lib.npfn_w2_assign(vp(g["a"]), vp(g["b"]), g["n_obs"], g["n"], g["dim"], vp(g["scale"]), ip(g["assign"]),
                                vp(g["duals"]), vp(g["cost_sum"]), vp(g["steps"]), ip(g["bad"]), None)
        return rc, (lib.npfn_last_error() or b"").decode()

    for kw in (dict(n_obs=-1), dict(n=0), dict(n=2049), dict(dim=0), dict(dim=65), dict(n=2048, dim=17),
               dict(n=513, dim=64), dict(a=0), dict(b=0), dict(scale=0), dict(assign=0), dict(cost_sum=0), dict(bad=0)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("w2_assign"), (kw, rc, msg)   # NPFN_EINVAL
    torch.cuda.synchronize()
    untouched = lambda: (int((assign != 7).sum()) == 0 and int((duals != 7).sum()) == 0  # noqa: E731
                         and cost_sum.tolist() == [7, 7] and steps.tolist() == [7, 7] and bad.tolist() == [7, 7])
    assert untouched()                                          # nothing ran
    assert call(n_obs=0)[0] == 0
    torch.cuda.synchronize()
    assert untouched()
    assert call(duals=0, steps=0)[0] == 0                       # both optional; the call zeroes the rest itself
    torch.cuda.synchronize()
    assert assign.tolist() == [list(range(8))] * 2 and cost_sum.tolist() == [0, 0] and bad.tolist() == [0, 0]
    assert int((duals != 7).sum()) == 0 and steps.tolist() == [7, 7]
    assert call()[0] == 0
    torch.cuda.synchronize()
    # all costs equal: insertion i walks the columns 0..i in order (the lowest column of every tie)
    assert int(duals.abs().sum()) == 0 and steps.tolist() == [36, 36]


def test_python_entry_refuses_bad_shapes():
    from npe_pfn.engine import Engine, w2_assign
    from npe_pfn.weights import ModelConfig, synthetic_weights

    cfg = ModelConfig()
    eng = Engine(cfg, synthetic_weights(cfg, seed=0), device=torch.device("cuda", 0), random_state=SEED)
    a, b = draws(9, 3, M=2)
    one = torch.ones(2, dtype=torch.float64)
    for fn in (w2_assign, eng.w2_assign):
        for args in ((a.cuda()[0], b.cuda()[0], one), (a.cuda(), b.cuda()[:, :8], one), (a.cuda(), b.cuda()[:1], one),
                     (a.cuda(), b.cuda()[:, :, :2], one), (a.cuda(), b.cuda(), one[:1]),
                     (torch.zeros(1, 4, 65).cuda(), torch.zeros(1, 4, 65).cuda(), one[:1]),
                     (torch.zeros(1, 2049, 1).cuda(), torch.zeros(1, 2049, 1).cuda(), one[:1]),
                     (torch.zeros(1, 2048, 17).cuda(), torch.zeros(1, 2048, 17).cuda(), one[:1])):
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        w2_assign(a, b, one)                                    # CPU tensors: not this entry's business
    cq, scale, _ = transport_costs_host(a, b)
    want = assignment_solve_host(cq)
    for got in (eng.w2_assign(a, b, scale), w2_assign(a.cuda(), b.cuda(), scale.cuda())):
        assert all(g.is_cuda and torch.equal(g.cpu(), w) for g, w in zip(got[:4], want))


def test_function_on_the_gpu_equals_the_cpu_path():
    a, b = draws(200, 5, M=3, seed=8)
    got, want = wasserstein_batched(a.cuda(), b.cuda()), wasserstein_batched(a, b)
    assert got.wasserstein.is_cuda and got.assignment.dtype == torch.int64 and got.n == 200
    assert torch.equal(got.cost_sum.cpu(), want.cost_sum) and torch.equal(got.scale.cpu(), want.scale)
    # equal integers and scales; the fp64 division and root on either device are good to an ulp
    assert torch.allclose(got.w2_squared.cpu(), want.w2_squared, rtol=2.0 ** -51, atol=0.0)
    assert torch.allclose(got.wasserstein.cpu(), want.wasserstein, rtol=2.0 ** -51, atol=0.0)
    assert want.steps.tolist() == [-1] * 3 and bool((got.steps > 0).all())
    z = wasserstein_batched(a.cuda(), b.cuda(), z_score=True)
    mu, sd = a.mean(1, keepdim=True), a.std(1, keepdim=True)
    zw = wasserstein_batched(((a - mu) / sd).cuda(), ((b - mu) / sd).cuda())
    assert torch.allclose(z.wasserstein, zw.wasserstein, rtol=1e-5) and not torch.equal(z.wasserstein, got.wasserstein)


# ------------------------------------------------------------------ on the estimator
def test_estimator_method_is_the_two_step_call():
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    m, T = 5, 40
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX + m, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX + m, DX))).astype(np.float32)
    x, th, x_o = (torch.from_numpy(v).cuda() for v in (x[:N_CTX], th[:N_CTX], x[N_CTX:]))
    kw = {"random_state": SEED, "device": "cuda:0", "preprocessing": "none"}
    post = TabPFN_Based_NPE_PFN(prior=None, regressor_init_kwargs=kw).append_simulations(th, x)
    twin = TabPFN_Based_NPE_PFN(prior=None, regressor_init_kwargs=kw).append_simulations(th, x)
    theta_ref = torch.from_numpy(np.random.default_rng(3).normal(size=(m, T, DTH)).astype(np.float32)).cuda()
    got = post.wasserstein_batched(theta_ref, x_o, num_posterior_samples=T)
    want = wasserstein_batched(twin.sample_batched(x_o, (T,)), theta_ref)
    assert post._model.sample_counter == twin._model.sample_counter
    assert got.n == want.n == T and got.wasserstein.shape == (m,) and bool((got.wasserstein > 0).all())
    for name in ("wasserstein", "w2_squared", "assignment", "cost_sum", "scale", "steps"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.is_cuda and torch.equal(g, w), name
    with pytest.raises(ValueError):
        post.wasserstein_batched(theta_ref, x_o, num_posterior_samples=T - 1)
    with pytest.raises(ValueError):
        post.wasserstein_batched(theta_ref[:, :, :2], x_o)
    with pytest.raises(ValueError):
        post.wasserstein_batched(theta_ref[:3], x_o)
