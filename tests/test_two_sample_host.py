"""CPU: mmd_batched / mmd_sums_host / permutation_labels against the reference's MMD formula in fp64
(tests/two_sample_ref.py) and against their own exact identities.  No GPU, no engine.
"""
import json
import os

import pytest
import torch

from npe_pfn import TwoSampleResult, mmd_batched, mmd_sums_host, permutation_labels
from npe_pfn.diagnostics import mmd_p_value
from two_sample_ref import BANDWIDTHS, mmd2

# NPFN_TWO_SAMPLE_PARITY_OUT=<file>: the parity test merges its measured maxima into that JSON
# file (profiles/two_sample/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_TWO_SAMPLE_PARITY_OUT")
SHAPES = ((65, 65, 3), (65, 63, 3), (129, 64, 20))


def merge_json(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def draws(n, m, d, shift, seed=0, M=1):
    g = torch.Generator().manual_seed(100 * seed + n + m + d)
    return torch.randn(M, n, d, generator=g), torch.randn(M, m, d, generator=g) + shift


# ------------------------------------------------------------------ parity with the reference formula
def test_parity_with_the_reference_formula():
    """|mmd2_biased - fp64 reference| <= 4 B (d + 3) 2^-24: a kernel value moves by at most max_t(t
    e^-t) < 1 times the relative error of the fp32 d2, (d + 2) 2^-24, plus one ulp of the kernel
    itself (the 2^-28 quantisation is far below); B bandwidths; the three means enter with
    weights 1, 1 and 2."""
    measured = {}
    for kernel in ("rbf", "multiscale"):
        B = len(BANDWIDTHS[kernel])
        for n, m, d in SHAPES:
            for shift in (0.0, 0.5):
                a, b = draws(n, m, d, shift)
                got = mmd_batched(a, b, kernel=kernel)
                assert isinstance(got, TwoSampleResult) and got.mmd2_biased.shape == (1,)
                assert got.mmd2_biased.dtype == torch.float64 and got.p_value is None and got.null.shape == (1, 0)
                assert (got.n, got.m, got.kernel, got.bandwidths) == (n, m, kernel, BANDWIDTHS[kernel])
                want = mmd2(a[0], b[0], kernel)
                err, bound = abs(float(got.mmd2_biased[0]) - want), 4 * B * (d + 3) * 2.0 ** -24
                print(f"{kernel} n={n} m={m} d={d} shift={shift}: mmd2={want:.6e} |diff|={err:.3e} bound={bound:.3e}")
                measured[f"{kernel}_n{n}_m{m}_d{d}_shift{shift}"] = {"abs_diff": err, "bound": bound}
                assert err <= bound, (kernel, n, m, d, shift, err, bound)
                if shift:
                    assert want > 100 * bound, "the shifted case does not exercise the formula"
    if PARITY_OUT:
        merge_json(PARITY_OUT, "host_vs_fp64_reference", measured)


# ------------------------------------------------------------------ exact identities
@pytest.mark.parametrize("kernel", ["rbf", "multiscale"])
def test_identical_sets_give_exactly_zero(kernel):
    a, _ = draws(65, 65, 3, 0.0, M=2)
    r = mmd_batched(a, a.clone(), kernel=kernel)
    assert r.mmd2_biased.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("kernel", ["rbf", "multiscale"])
def test_row_order_and_swap_leave_the_bits_alone(kernel):
    a, b = draws(65, 63, 3, 0.5, M=2)
    r = mmd_batched(a, b, kernel=kernel)
    g = torch.Generator().manual_seed(5)
    s = mmd_batched(a[:, torch.randperm(65, generator=g)], b[:, torch.randperm(63, generator=g)], kernel=kernel)
    assert torch.equal(r.mmd2_biased, s.mmd2_biased) and torch.equal(r.mmd2_unbiased, s.mmd2_unbiased)
    assert torch.equal(r.null, s.null) and s.p_value is None
    t = mmd_batched(b, a, kernel=kernel)
    assert torch.equal(r.mmd2_biased, t.mmd2_biased) and (t.n, t.m) == (63, 65)
    # the sums themselves: the same pooled points under swapped labels swap the two slots
    z = torch.cat([a, b], 1)
    lab = permutation_labels(65, 63, 3, seed=1)
    s0, t0, _ = mmd_sums_host(z, lab, kernel, BANDWIDTHS[kernel])
    s1, t1, _ = mmd_sums_host(z, 1 - lab, kernel, BANDWIDTHS[kernel])
    assert torch.equal(s0, s1.flip(-1)) and torch.equal(t0, t1)


def test_sums_by_hand():
    """Three points on a line, one bandwidth, multiscale with a = 1: k = 1 / (1 + d2)."""
    z = torch.tensor([[[0.0], [1.0], [3.0]]])
    lab = torch.tensor([[1, 1, 0], [1, 0, 1], [0, 0, 0]], dtype=torch.uint8)
    sums, total, bad = mmd_sums_host(z, lab, "multiscale", [1.0])
    one = 2 ** 28
    q = lambda d2: round(float(torch.tensor(1.0) / (torch.tensor(1.0) + torch.tensor(float(d2)))) * one)  # noqa: E731
    q01, q02, q12 = q(1), q(9), q(4)
    assert sums.dtype == torch.int64 and total.dtype == torch.int64 and bad.dtype == torch.int32
    assert sums[0].tolist() == [[2 * one + 2 * q01, one], [2 * one + 2 * q02, one],
                                [0, 3 * one + 2 * (q01 + q02 + q12)]]
    assert total.tolist() == [3 * one + 2 * (q01 + q02 + q12)] and bad.tolist() == [0]


# ------------------------------------------------------------------ permutation_labels
def test_permutation_labels():
    lab = permutation_labels(5, 9, 40, seed=3)
    assert lab.shape == (41, 14) and lab.dtype == torch.uint8 and lab.device.type == "cpu"
    assert lab[0].tolist() == [1] * 5 + [0] * 9
    assert lab.sum(1).tolist() == [5] * 41 and int(lab.max()) == 1
    assert torch.equal(lab, permutation_labels(5, 9, 40, seed=3))
    assert not torch.equal(lab, permutation_labels(5, 9, 40, seed=4))
    assert len({tuple(r) for r in lab[1:].tolist()}) > 30, "the permutations repeat"
    # row p is the p-th randperm of the seeded generator
    g = torch.Generator().manual_seed(3)
    for p in (1, 2):
        want = torch.zeros(14, dtype=torch.uint8)
        want[torch.randperm(14, generator=g)[:5]] = 1
        assert torch.equal(lab[p], want)
    assert permutation_labels(2, 1, 0).tolist() == [[1, 1, 0]]
    for bad in ((0, 3, 1), (3, 0, 1), (3, 3, -1)):
        with pytest.raises(ValueError):
            permutation_labels(*bad)


# ------------------------------------------------------------------ the statistics
def test_p_value_formula():
    obs = torch.tensor([0.5, 0.1, 2.0, float("nan")], dtype=torch.float64)
    null = torch.tensor([[0.1, 0.5, 0.7, 0.2], [0.2, 0.3, 0.4, 0.5], [0.1, 0.2, 0.3, 0.4], [0.1, 0.2, 0.3, 0.4]],
                        dtype=torch.float64)
    p = mmd_p_value(obs, null)
    assert p[:3].tolist() == [3 / 5, 5 / 5, 1 / 5] and bool(torch.isnan(p[3]))


@pytest.mark.parametrize("kernel", ["rbf", "multiscale"])
def test_null_and_p_value_follow_the_labels(kernel):
    a, b = draws(30, 21, 2, 3.0, M=2)
    P = 19
    r = mmd_batched(a, b, kernel=kernel, num_permutations=P, seed=7)
    assert r.null.shape == (2, P) and r.p_value.shape == (2,)
    z, lab = torch.cat([a, b], 1), permutation_labels(30, 21, P, seed=7)
    for p in (1, P):   # the relabelled sets, through the plain call
        x, y = z[:, lab[p] == 1], z[:, lab[p] == 0]
        assert torch.equal(mmd_batched(x, y, kernel=kernel).mmd2_biased, r.null[:, p - 1])
    assert torch.equal(r.p_value, mmd_p_value(r.mmd2_biased, r.null))
    assert r.p_value.tolist() == [1 / (P + 1)] * 2     # a shift of three sigma at these sizes
    same = mmd_batched(a, b, kernel=kernel, num_permutations=P, seed=7)
    assert torch.equal(same.null, r.null)
    assert not torch.equal(mmd_batched(a, b, kernel=kernel, num_permutations=P, seed=8).null, r.null)


@pytest.mark.parametrize("kernel", ["rbf", "multiscale"])
def test_unbiased_formula_at_unequal_sizes(kernel):
    from two_sample_ref import kernel_sum

    a, b = draws(40, 23, 3, 0.5)
    r = mmd_batched(a, b, kernel=kernel)
    bw = BANDWIDTHS[kernel]
    x, y = a[0].double(), b[0].double()
    kxx, kyy, kxy = kernel_sum(x, x, kernel, bw), kernel_sum(y, y, kernel, bw), kernel_sum(x, y, kernel, bw)
    want = float((kxx.sum() - kxx.diag().sum()) / (40 * 39) + (kyy.sum() - kyy.diag().sum()) / (23 * 22)
                 - 2 * kxy.mean())
    # the off-diagonal means carry the same per-value error as the biased ones
    assert abs(float(r.mmd2_unbiased[0]) - want) <= 4 * len(bw) * (3 + 3) * 2.0 ** -24
    assert float(r.mmd2_unbiased[0]) < float(r.mmd2_biased[0])
    one = mmd_batched(a[:, :1], b, kernel=kernel)
    assert bool(torch.isnan(one.mmd2_unbiased).all()) and bool(torch.isfinite(one.mmd2_biased).all())


def test_z_score():
    a, b = draws(50, 40, 3, 0.5, M=2)
    a = a * torch.tensor([1.0, 30.0, 0.01]) + 4.0
    b = b * torch.tensor([1.0, 30.0, 0.01]) + 4.0
    a[1, :, 2] = 2.5                      # a zero std counts as 1
    mu, sd = a.mean(1, keepdim=True), a.std(1, keepdim=True)
    sd = torch.where(sd == 0, torch.ones_like(sd), sd)
    want = mmd_batched((a - mu) / sd, (b - mu) / sd, num_permutations=5)
    got = mmd_batched(a, b, num_permutations=5, z_score=True)
    assert torch.equal(got.mmd2_biased, want.mmd2_biased) and torch.equal(got.null, want.null)
    assert bool(torch.isfinite(got.mmd2_biased).all())
    assert not torch.equal(got.mmd2_biased, mmd_batched(a, b).mmd2_biased)


def test_two_dimensional_inputs_mean_one_observation():
    a, b = draws(20, 30, 4, 0.3)
    r2, r3 = mmd_batched(a[0], b[0], num_permutations=3), mmd_batched(a, b, num_permutations=3)
    assert r2.mmd2_biased.shape == (1,) and torch.equal(r2.mmd2_biased, r3.mmd2_biased)
    assert torch.equal(r2.null, r3.null) and torch.equal(r2.p_value, r3.p_value)


def test_non_finite_input_gives_nan():
    a, b = draws(20, 30, 4, 0.3, M=3)
    a[1, 3, 2] = float("nan")
    b[2, 0, 0] = float("inf")
    r = mmd_batched(a, b, num_permutations=4)
    ok = mmd_batched(a[:1], b[:1], num_permutations=4)
    for t in (r.mmd2_biased, r.mmd2_unbiased, r.p_value):
        assert bool(torch.isnan(t[1:]).all()) and bool(torch.isfinite(t[0]))
    assert bool(torch.isnan(r.null[1:]).all())
    assert torch.equal(r.mmd2_biased[:1], ok.mmd2_biased) and torch.equal(r.null[:1], ok.null)
    _, _, bad = mmd_sums_host(torch.cat([a, b], 1), permutation_labels(20, 30, 0), "rbf", [1.0])
    assert bad.tolist() == [0, 1, 1]


def test_value_errors():
    a, b = draws(6, 7, 3, 0.0, M=2)
    for kw in (dict(kernel="linear"), dict(bandwidths=[]), dict(bandwidths=[1.0] * 9), dict(bandwidths=[1.0, 0.0]),
               dict(bandwidths=[-1.0]), dict(bandwidths=[float("inf")]), dict(bandwidths=[float("nan")]),
               dict(num_permutations=-1), dict(num_permutations=4096)):
        with pytest.raises(ValueError):
            mmd_batched(a, b, **kw)
    for x, y in ((a, b[:1]), (a, b[:, :, :2]), (a[0], b), (a[:, :0], b), (a, b[:, :0]), (a[0, 0], b[0, 0]),
                 (torch.zeros(1, 6, 65), torch.zeros(1, 6, 65)), (torch.zeros(1, 32768, 1), torch.zeros(1, 1, 1))):
        with pytest.raises(ValueError):
            mmd_batched(x, y)
    with pytest.raises(ValueError):
        mmd_batched(a[:, :1], b, z_score=True)
    z, lab = torch.cat([a, b], 1), permutation_labels(6, 7, 2)
    for args in ((z[0], lab, "rbf", [1.0]), (z, lab[:, :-1], "rbf", [1.0]), (z, lab[0], "rbf", [1.0]),
                 (z, lab, 2, [1.0]), (z, lab, "rbf", [0.0]), (z, lab, "rbf", [1.0] * 9),
                 (z, torch.zeros(4097, 13, dtype=torch.uint8), "rbf", [1.0])):
        with pytest.raises(ValueError):
            mmd_sums_host(*args)
    s, t, bad = mmd_sums_host(z[:0], lab, "multiscale", [1.0])
    assert s.shape == (0, 3, 2) and t.shape == (0,) and bad.shape == (0,)
