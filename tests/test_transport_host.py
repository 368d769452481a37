"""CPU: transport_costs_host / assignment_solve_host / wasserstein_batched against brute force, against
scipy's linear_sum_assignment on the same integer costs, and against their own certificates and
exact identities.  No GPU, no engine.
"""
import itertools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from npe_pfn import TransportResult, assignment_solve_host, transport_costs_host, wasserstein_batched
from npe_pfn.diagnostics import transport_scale


def draws(n, d, M=1, seed=0, shift=0.5):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + d)
    return torch.randn(M, n, d, generator=g), torch.randn(M, n, d, generator=g) + shift


def tie_grid(n, M=1, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    return (torch.randint(0, 8, (M, n, 2), generator=g).float(), torch.randint(0, 8, (M, n, 2), generator=g).float())


def certify(cq, assign, duals, cost_sum, steps):
    M, n, _ = cq.shape
    for m in range(M):
        u, v = duals[m, 0], duals[m, 1]
        assert bool((u[:, None] + v[None, :] <= cq[m]).all())
        assert int(u.sum() + v.sum()) == int(cost_sum[m])
        asg = assign[m].to(torch.int64)
        assert sorted(asg.tolist()) == list(range(n))
        assert int(cq[m][torch.arange(n), asg].sum()) == int(cost_sum[m])
        assert n <= int(steps[m]) <= n * (n + 1) // 2


def test_brute_force_up_to_six_points():
    for n in range(1, 7):
        for kind in ("normal", "grid"):
            a, b = draws(n, 2, M=3, seed=n) if kind == "normal" else tie_grid(n, M=3, seed=n)
            cq, scale, bad = transport_costs_host(a, b)
            assign, duals, cost_sum, steps = assignment_solve_host(cq)
            assert assign.dtype == torch.int32 and duals.dtype == cost_sum.dtype == steps.dtype == torch.int64
            certify(cq, assign, duals, cost_sum, steps)
            for m in range(3):
                c = cq[m]
                best = min(sum(int(c[i, p[i]]) for i in range(n)) for p in itertools.permutations(range(n)))
                assert int(cost_sum[m]) == best, (n, kind, m)


@pytest.mark.parametrize("n,d,kind", [(65, 10, "normal"), (256, 2, "grid"), (1000, 10, "normal")])
def test_scipy_cost_and_certificates(n, d, kind):
    a, b = draws(n, d) if kind == "normal" else tie_grid(n)
    cq, scale, bad = transport_costs_host(a, b)
    assert cq.dtype == torch.int64 and scale.dtype == torch.float64 and bad.tolist() == [0]
    assign, duals, cost_sum, steps = assignment_solve_host(cq)
    certify(cq, assign, duals, cost_sum, steps)
    c = cq[0].numpy()
    rows, cols = linear_sum_assignment(c)
    assert int(c[rows, cols].sum()) == int(cost_sum[0])
    r = wasserstein_batched(a, b)
    assert isinstance(r, TransportResult) and r.n == n and r.steps.tolist() == [-1]
    assert r.cost_sum.tolist() == cost_sum.tolist() and sorted(r.assignment[0].tolist()) == list(range(n))
    assert float(r.wasserstein[0]) == float(np.sqrt(int(cost_sum[0]) / float(scale[0]) / n))
    assert torch.equal(r.w2_squared, r.wasserstein ** 2) or torch.allclose(r.w2_squared, r.wasserstein ** 2, rtol=1e-15)
    # the reference's number, in fp64 on the real-valued costs: d2's fp32 rounding is (d + 2) 2^-24
    # relative and the integer grid 2^-40 of the cost bound, on the cost; half of that on its root
    d2 = ((a[0].double()[:, None, :] - b[0].double()[None, :, :]) ** 2).sum(-1).numpy()
    rr, cc = linear_sum_assignment(d2)
    want = float(np.sqrt(d2[rr, cc].sum() / n))
    assert abs(float(r.wasserstein[0]) - want) <= want * (d + 3) * 2.0 ** -24, (float(r.wasserstein[0]), want)


def test_ladder_is_the_worst_case():
    a = torch.arange(256.0)[None, :, None]
    b = a + 128
    cq, scale, _ = transport_costs_host(a, b)
    assign, duals, cost_sum, steps = assignment_solve_host(cq)
    assert steps.tolist() == [256 * 257 // 2]
    certify(cq, assign, duals, cost_sum, steps)
    assert wasserstein_batched(a, b).wasserstein.tolist() == [128.0]


def test_translated_copy_is_matched_to_itself():
    a, _ = draws(65, 3, seed=4)
    t = torch.tensor([0.75, -1.5, 2.0])
    b = a + t
    cq, scale, _ = transport_costs_host(a, b)
    assign, _, cost_sum, _ = assignment_solve_host(cq)
    assert assign[0].tolist() == list(range(65))
    r = wasserstein_batched(a, b)
    norm = float(t.double().norm())
    # every d2(i, i) is |t|^2 up to the fp32 rounding of b = a + t (2^-24 of |b_k| per coordinate, against
    # t_k) and of the chain ((d + 2) 2^-24 relative)
    slack = float((2.0 ** -24 * (b.abs().max() / t.abs().min()) * 2 + 5 * 2.0 ** -24))
    assert abs(float(r.wasserstein[0]) - norm) <= norm * slack, (float(r.wasserstein[0]), norm)
    assert r.assignment[0].tolist() == list(range(65))


def test_one_dimension_is_the_sorted_matching():
    a, b = draws(200, 1, seed=5)
    cq, _, _ = transport_costs_host(a, b)
    assign, _, cost_sum, _ = assignment_solve_host(cq)
    ia, ib = torch.argsort(a[0, :, 0]), torch.argsort(b[0, :, 0])
    sorted_cost = int(cq[0][ia, ib].sum())
    assert int(cost_sum[0]) == sorted_cost
    want = torch.empty(200, dtype=torch.int64)
    want[ia] = ib
    assert assign[0].tolist() == want.tolist()      # strictly convex cost, distinct points: the optimum is unique


def test_scale_is_a_power_of_two_of_the_observation_alone():
    a, b = draws(33, 4, M=4, seed=6)
    a[1] *= 1e-3
    b[1] *= 1e-3
    a[2] *= 1e6
    b[2] *= 1e6
    a[3] = 0.0
    b[3] = 0.0
    cq, scale, bad = transport_costs_host(a, b)
    assert bad.tolist() == [0, 0, 0, 0] and float(scale[3]) == 1.0 and int(cq[3].abs().sum()) == 0
    mant, _ = torch.frexp(scale)
    assert mant.tolist() == [0.5] * 4
    assert int(cq.min()) >= 0 and int(cq.max()) <= 2 ** 41
    assert int(cq[:3].amax((1, 2)).min()) >= 2 ** 30     # the grid is fine in every observation
    for m in range(4):
        cq1, scale1, _ = transport_costs_host(a[m: m + 1], b[m: m + 1])
        assert torch.equal(scale1[0], scale[m]) and torch.equal(cq1[0], cq[m])
    s, nonfinite = transport_scale(a, b)
    assert torch.equal(s, scale) and nonfinite.tolist() == [False] * 4


def test_costs_stay_below_the_bound_over_nine_decades():
    g = torch.Generator().manual_seed(7)
    for lo, hi in ((1e-3, 1e6), (1e-3, 1e-3), (1e6, 1e6)):
        mag = torch.exp(torch.rand(3, 50, 5, generator=g) * (np.log(hi) - np.log(lo)) + np.log(lo))
        a = mag * torch.sign(torch.randn(3, 50, 5, generator=g))
        b = a.flip(1) * 0.5
        cq, scale, bad = transport_costs_host(a, b)
        assert bad.tolist() == [0, 0, 0] and 0 <= int(cq.min()) and int(cq.max()) <= 2 ** 41


def test_non_finite_input_gives_nan():
    a, b = draws(20, 3, M=3, seed=8)
    ok = wasserstein_batched(a[:1], b[:1])
    a[1, 3, 2] = float("nan")
    b[2, 0, 0] = float("inf")
    cq, scale, bad = transport_costs_host(a, b)
    assert bad.tolist() == [0, 1, 1] and scale[1:].tolist() == [1.0, 1.0] and int(cq[1:].abs().sum()) == 0
    r = wasserstein_batched(a, b)
    assert torch.isnan(r.wasserstein).tolist() == [False, True, True]
    assert torch.isnan(r.w2_squared).tolist() == [False, True, True]
    assert bool((r.assignment[1:] == -1).all())
    assert torch.equal(r.wasserstein[:1], ok.wasserstein) and torch.equal(r.assignment[:1], ok.assignment)


def test_two_dimensional_inputs_and_z_score():
    a, b = draws(30, 3, M=2, seed=9)
    r2, r3 = wasserstein_batched(a[0], b[0]), wasserstein_batched(a[:1], b[:1])
    assert r2.wasserstein.shape == (1,) and torch.equal(r2.wasserstein, r3.wasserstein)
    a = a * torch.tensor([1.0, 30.0, 0.01]) + 4.0
    b = b * torch.tensor([1.0, 30.0, 0.01]) + 4.0
    a[1, :, 2] = 2.5                      # a zero std counts as 1
    mu, sd = a.mean(1, keepdim=True), a.std(1, keepdim=True)
    sd = torch.where(sd == 0, torch.ones_like(sd), sd)
    want = wasserstein_batched((a - mu) / sd, (b - mu) / sd)
    got = wasserstein_batched(a, b, z_score=True)
    assert torch.equal(got.wasserstein, want.wasserstein) and bool(torch.isfinite(got.wasserstein).all())
    assert not torch.equal(got.wasserstein, wasserstein_batched(a, b).wasserstein)


def test_value_errors():
    a, b = draws(6, 3, M=2)
    with pytest.raises(ValueError, match="unequal size is not an assignment.*reference harness"):
        wasserstein_batched(a, b[:, :5])
    with pytest.raises(ValueError, match="unequal size"):
        transport_costs_host(a, b[:, :5])
    for x, y in ((a, b[:1]), (a, b[:, :, :2]), (a[0], b), (a[:, :0], b[:, :0]), (a[0, 0], b[0, 0]),
                 (torch.zeros(1, 6, 65), torch.zeros(1, 6, 65)), (torch.zeros(1, 2049, 1), torch.zeros(1, 2049, 1)),
                 (torch.zeros(1, 2048, 17), torch.zeros(1, 2048, 17))):
        with pytest.raises(ValueError):
            wasserstein_batched(x, y)
    with pytest.raises(ValueError):
        wasserstein_batched(a[:, :1], b[:, :1], z_score=True)
    for cq in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(1, 3, 4, dtype=torch.int64),
               torch.zeros(1, 0, 0, dtype=torch.int64)):
        with pytest.raises(ValueError):
            assignment_solve_host(cq)
    out = assignment_solve_host(torch.zeros(0, 4, 4, dtype=torch.int64))
    assert [tuple(t.shape) for t in out] == [(0, 4), (0, 2, 4), (0,), (0,)]


def test_estimator_method_is_the_two_step_call():
    """NPE_PFN_Core.wasserstein_batched draws T per observation with sample_batched and hands the
    draws and the reference draws to the function; the unconditional estimator refuses."""
    from npe_pfn.npe_pfn import NPE_PFN_Core, TabPFN_Based_Uncond_Estimator

    M, T, dth = 3, 17, 2
    a, ref = draws(T, dth, M=M, seed=10)
    calls = []

    class Stub(NPE_PFN_Core):
        def __init__(self):
            self._theta_train = torch.zeros(5, dth)

        def _fused(self):
            return False

        def sample_batched(self, x, sample_shape, **kw):
            calls.append((tuple(x.shape), tuple(sample_shape)))
            return a

    core = Stub()
    x = torch.zeros(M, 4)
    got, want = core.wasserstein_batched(ref, x), wasserstein_batched(a, ref)
    assert calls == [((M, 4), (T,))]
    for name in ("wasserstein", "w2_squared", "assignment", "cost_sum", "scale", "steps"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    z = core.wasserstein_batched(ref, x, num_posterior_samples=T, z_score=True)
    assert torch.equal(z.wasserstein, wasserstein_batched(a, ref, z_score=True).wasserstein)
    for bad_call in (lambda: core.wasserstein_batched(ref, x, num_posterior_samples=T + 1),
                     lambda: core.wasserstein_batched(ref[:, :, :1], x), lambda: core.wasserstein_batched(ref[:2], x)):
        with pytest.raises(ValueError):
            bad_call()
    assert len(calls) == 2                                      # a refused call draws nothing
    with pytest.raises(NotImplementedError):
        TabPFN_Based_Uncond_Estimator.wasserstein_batched(object.__new__(TabPFN_Based_Uncond_Estimator), ref)
