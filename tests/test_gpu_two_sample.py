"""GPU: npfn_mmd_sums against its torch definition (multiscale exactly, rbf to expf's last bit), its
refusals, its memory footprint, and mmd_batched on the estimator's own draws (calibration of the
permutation p-values, power against a shift, NPE_PFN_Core.mmd_batched).

The estimator tests use the shapes of tests/test_gpu_coverage.py's self-consistency test: 150 context
rows, dim_x = dim_theta = 3, synthetic weights, 256 observations x 63 draws, preprocessing "none".
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from npe_pfn.diagnostics import mmd_batched, mmd_sums_host, permutation_labels, pit_ks_statistic
from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
T = 64        # points per tile edge (npfn_mmd.hip kTile)
SLAB = 256    # labellings per workgroup (npfn_mmd.hip kSlab)
# (n, m): one point each; a tile and a point; a tile less one and two (N = T + 1); two full tiles; the
# group boundary inside a tile at N = 2 T; N = 2 T + 2; three tiles and two points
SIZES = ((1, 1), (1, T), (T - 1, 2), (T, T), (T + 1, T - 1), (T + 1, T + 1), (2 * T + 1, 1))
DIMS = (1, 3, 20, 64)
# (n_bw, n_label, n_obs): every n_bw in {1, 4, 8}, n_label in {1, 2, 200, one past the slab}, n_obs in {1, 3}
COMBOS = ((1, 1, 1), (4, 2, 3), (8, 200, 1), (4, SLAB + 1, 3))
BW = {"rbf": (10.0, 15.0, 20.0, 50.0, 0.7, 3.0, 120.0, 1.5), "multiscale": (0.2, 0.5, 0.9, 1.3, 0.05, 2.0, 7.0, 0.33)}
N_CTX, DX, DTH = 150, 3, 3
M_SELF, S_SELF, P_SELF = 256, 63, 199
SEED = 2
KS_BOUND = 1.95 / np.sqrt(M_SELF) + 1.0 / (P_SELF + 1)   # alpha = 0.001 plus the p-values' grid step
# NPFN_TWO_SAMPLE_PARITY_OUT=<file>: the estimator tests merge their statistics into that JSON file
# (profiles/two_sample/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_TWO_SAMPLE_PARITY_OUT")


def merge_json(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def gpu_sums(z, labels, kernel, bw):
    from npe_pfn.engine import mmd_sums

    return tuple(t.cpu() for t in mmd_sums(z.cuda(), labels.cuda(), kernel, bw))


# ------------------------------------------------------------------ the kernel
def case(n, m, d, n_label, n_obs, kind, seed=0):
    """(z [n_obs, n + m, d], labels [n_label, n + m]) on the CPU.  "grid": multiples of 1/8, so many
    distances tie and many are 0; "normal": random normals."""
    rng = np.random.default_rng(seed + 7 * n + 11 * m + 13 * d + 17 * n_label)
    if kind == "grid":
        z = (rng.integers(-4, 5, size=(n_obs, n + m, d)) / 8.0).astype(np.float32)
    else:
        z = rng.normal(size=(n_obs, n + m, d)).astype(np.float32)
    return torch.from_numpy(z), permutation_labels(n, m, n_label - 1, seed=seed + n_label)


def check(kernel, z, lab, bw, what):
    want_s, want_t, want_b = mmd_sums_host(z, lab, kernel, bw)
    got_s, got_t, got_b = gpu_sums(z, lab, kernel, bw)
    assert got_s.dtype == torch.int64 and got_t.dtype == torch.int64 and got_b.dtype == torch.int32
    assert torch.equal(got_b, want_b) and int(want_b.sum()) == 0, what
    if kernel == "multiscale":
        assert torch.equal(got_s, want_s) and torch.equal(got_t, want_t), what
    else:
        # expf on either side is good to 1 ulp, so two k_b differ by at most 2^-23 = 32 units of
        # 2^-28; twice that per bandwidth and ordered pair of the counter
        ones = (lab != 0).sum(1).to(torch.int64)
        N = z.shape[1]
        pairs = torch.stack([ones * ones, (N - ones) * (N - ones)], 1)
        assert bool(((got_s - want_s).abs() <= 64 * len(bw) * pairs[None]).all()), what
        assert bool(((got_t - want_t).abs() <= 64 * len(bw) * N * N).all()), what
    return got_s, got_t


@pytest.mark.parametrize("kernel", ["multiscale", "rbf"])
@pytest.mark.parametrize("n,m", SIZES)
def test_kernel_against_the_definition(kernel, n, m):
    for d in DIMS:
        for n_bw, n_label, n_obs in COMBOS:
            for kind in ("normal", "grid"):
                z, lab = case(n, m, d, n_label, n_obs, kind)
                bw = BW[kernel][:n_bw]
                what = (kernel, n, m, d, n_bw, n_label, n_obs, kind)
                check(kernel, z, lab, bw, what)


@pytest.mark.parametrize("kernel", ["multiscale", "rbf"])
def test_same_bits_alone_among_others_and_twice(kernel):
    z, lab = case(T + 1, T - 1, 20, SLAB + 1, 3, "normal", seed=3)
    bw = BW[kernel][:4]
    s, t, _ = gpu_sums(z, lab, kernel, bw)
    s2, t2, _ = gpu_sums(z, lab, kernel, bw)
    assert torch.equal(s, s2) and torch.equal(t, t2)
    for u in range(3):
        su, tu, _ = gpu_sums(z[u: u + 1], lab, kernel, bw)
        assert torch.equal(su[0], s[u]) and torch.equal(tu[0], t[u]), u
    # a labelling's sums do not depend on the labellings around it
    s1, _, _ = gpu_sums(z, lab[SLAB - 1: SLAB + 1], kernel, bw)
    assert torch.equal(s1, s[:, SLAB - 1: SLAB + 1])
    # the diagonal is exact: a single point
    s0, t0, _ = gpu_sums(z[:, :1], lab[:1, :1], kernel, bw)
    assert s0[:, 0].tolist() == [[4 * 2 ** 28, 0]] * 3 and t0.tolist() == [4 * 2 ** 28] * 3


def test_non_finite_coordinates_raise_bad():
    z, lab = case(T + 1, T + 1, 3, 2, 3, "normal", seed=4)
    z[0, 2 * T + 1, 2] = float("nan")    # the last point of the last tile
    z[2, 5, 0] = float("-inf")
    s, t, bad = gpu_sums(z, lab, "multiscale", [1.0])
    assert bad.tolist() == [1, 0, 1]
    ws, wt, _ = mmd_sums_host(z[1:2], lab, "multiscale", [1.0])
    assert torch.equal(s[1:2], ws) and torch.equal(t[1:2], wt)
    r = mmd_batched(z[:, : T + 1].cuda(), z[:, T + 1:].cuda(), kernel="multiscale", num_permutations=3)
    for v in (r.mmd2_biased, r.mmd2_unbiased, r.p_value, r.null[:, 0]):
        assert torch.isnan(v).tolist() == [True, False, True]


def test_rejected_arguments():
    from npe_pfn.engine import load_library

    lib = load_library()
    z = torch.zeros((2, 8, 3), device="cuda")
    lab = torch.ones((2, 8), dtype=torch.uint8, device="cuda")
    sums = torch.full((2, 2, 2), 7, dtype=torch.int64, device="cuda")
    total = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    bad = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    good = dict(z=z.data_ptr(), n_obs=2, n_pool=8, dim=3, kernel=0, bw=[1.0, 2.0], n_bw=None, labels=lab.data_ptr(),
                n_label=2, sums=sums.data_ptr(), total=total.data_ptr(), bad=bad.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        bw = (ctypes.c_float * max(1, len(a["bw"])))(*a["bw"]) if a["bw"] is not None else None
        n_bw = len(a["bw"]) if a["n_bw"] is None else a["n_bw"]
        vp = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
        rc = lib.npfn_mmd_sums(vp(a["z"]), a["n_obs"], a["n_pool"], a["dim"], a["kernel"],
                               ctypes.cast(bw, ctypes.c_void_p) if bw is not None else None, n_bw, vp(a["labels"]),
                               a["n_label"], vp(a["sums"]), vp(a["total"]),
                               ctypes.cast(vp(a["bad"]), ctypes.POINTER(ctypes.c_int32)) if a["bad"] else None, None)
        return rc, (lib.npfn_last_error() or b"").decode()

    inf, nan = float("inf"), float("nan")
    for kw in (dict(n_obs=-1), dict(n_pool=0), dict(n_pool=32769), dict(dim=0), dict(dim=65), dict(kernel=2),
               dict(kernel=-1), dict(bw=[1.0], n_bw=0), dict(bw=[1.0] * 9), dict(bw=[1.0, 0.0]), dict(bw=[-2.0]),
               dict(bw=[inf]), dict(bw=[nan, 1.0]), dict(n_label=0), dict(n_label=4097), dict(z=0), dict(bw=None, n_bw=1),
               dict(labels=0), dict(sums=0), dict(total=0), dict(bad=0)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("mmd_sums"), (kw, rc, msg)   # NPFN_EINVAL
    torch.cuda.synchronize()
    assert int((sums != 7).sum()) == 0 and total.tolist() == [7, 7] and bad.tolist() == [7, 7]   # nothing ran
    assert call(n_obs=0)[0] == 0
    torch.cuda.synchronize()
    assert int((sums != 7).sum()) == 0
    assert call()[0] == 0                                       # the call zeroes its outputs itself
    torch.cuda.synchronize()
    assert sums[:, :, 0].tolist() == [[2 * 64 * 2 ** 28] * 2] * 2 and int(sums[:, :, 1].abs().sum()) == 0
    assert total.tolist() == [2 * 64 * 2 ** 28] * 2 and bad.tolist() == [0, 0]


def test_python_entry_refuses_bad_shapes():
    from npe_pfn.engine import Engine, mmd_sums

    eng = Engine(CFG, synthetic_weights(CFG, seed=0), device=torch.device("cuda", 0), random_state=SEED)
    z, lab = case(5, 4, 3, 3, 2, "normal")
    for fn in (mmd_sums, eng.mmd_sums):
        for args in ((z.cuda()[0], lab, "rbf", [1.0]), (z.cuda(), lab[:, :-1], "rbf", [1.0]),
                     (z.cuda(), lab, "cauchy", [1.0]), (z.cuda(), lab, "rbf", []), (z.cuda(), lab, "rbf", [0.0]),
                     (torch.zeros(1, 4, 65).cuda(), lab[:, :4], "rbf", [1.0])):
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        mmd_sums(z, lab, "rbf", [1.0])                           # CPU tensors: not this entry's business
    want = mmd_sums_host(z, lab, "multiscale", [0.5, 2.0])
    for got in (eng.mmd_sums(z, lab, "multiscale", [0.5, 2.0]), eng.mmd_sums(z.cuda(), lab.bool(), 1, [0.5, 2.0])):
        assert all(g.is_cuda and torch.equal(g.cpu(), w) for g, w in zip(got, want))


def test_no_dense_matrix():
    """8 observations x 4096 pooled points x 65 labellings: the call may allocate its pooled copy,
    labels and outputs; a dense N x N fp32 matrix would be 64 MB per observation."""
    M, n, d, P = 8, 2048, 10, 64
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(M, n, d, generator=g).cuda(), torch.randn(M, n, d, generator=g).cuda()
    mmd_batched(a[:, :8], b[:, :8], num_permutations=1)          # the library is loaded before the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = mmd_batched(a, b, num_permutations=P)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    inputs, pooled, labels = 2 * M * n * d * 4, M * 2 * n * d * 4, (P + 1) * 2 * n
    outputs = M * (P + 1) * 2 * 8 + M * 8 + M * 4
    budget = inputs + pooled + labels + outputs + (1 << 20)
    print(f"peak rise {rise} bytes, budget {budget}; one dense matrix = {4 * (2 * n) ** 2}")
    assert rise <= budget < 4 * (2 * n) ** 2
    assert r.null.shape == (M, P) and bool(torch.isfinite(r.mmd2_biased).all())
    assert bool((r.mmd2_biased > 0).all()) and bool(((r.p_value > 0) & (r.p_value <= 1)).all())


# ------------------------------------------------------------------ on the estimator
def _data(m):
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX + m, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX + m, DX))).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (x[:N_CTX], th[:N_CTX], x[N_CTX:]))


def _post(x, th):
    from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN

    post = TabPFN_Based_NPE_PFN(prior=None, regressor_init_kwargs={"random_state": SEED, "device": "cuda:0",
                                                                   "preprocessing": "none"})
    return post.append_simulations(th, x)


@pytest.fixture(scope="module")
def two_draws():
    """Two successive sample_batched calls of one estimator: the sample counter advances between
    them, so they are independent draws of one distribution per observation."""
    x, th, x_o = _data(M_SELF)
    post = _post(x, th)
    a = post.sample_batched(x_o, (S_SELF,))
    b = post.sample_batched(x_o, (S_SELF,))
    assert a.shape == b.shape == (M_SELF, S_SELF, DTH) and a.is_cuda and not torch.equal(a, b)
    return a, b


@pytest.mark.parametrize("kernel", ["rbf", "multiscale"])
def test_p_values_are_calibrated_and_the_test_has_power(two_draws, kernel):
    """Same distribution: the permutation p-values are uniform on {1/200 .. 1}, so their KS
    distance from the uniform distribution stays below 1.95 / sqrt(256) + 1 / 200 (alpha = 0.001
    plus the grid step).  Shifted by two standard deviations: every p-value is the smallest
    possible one, 1 / 200."""
    a, b = two_draws
    r = mmd_batched(a, b, kernel=kernel, num_permutations=P_SELF, seed=1)
    assert r.p_value.shape == (M_SELF,) and r.p_value.is_cuda and r.null.shape == (M_SELF, P_SELF)
    ks = float(pit_ks_statistic(r.p_value[:, None].cpu())[0])
    shifted = mmd_batched(a, b + 2 * a.std(1, keepdim=True), kernel=kernel, num_permutations=P_SELF, seed=1)
    ratio = float((shifted.mmd2_biased / shifted.null.max(1).values).min())
    print(f"{kernel}: KS of {M_SELF} p-values = {ks:.4f} (bound {KS_BOUND:.4f}); shifted: smallest observed / "
          f"largest permuted statistic = {ratio:.2f}")
    if PARITY_OUT:
        merge_json(PARITY_OUT, f"estimator_{kernel}", {
            "observations": M_SELF, "draws_per_set": S_SELF, "permutations": P_SELF, "p_value_ks": ks,
            "ks_bound": KS_BOUND, "shift_in_std": 2.0, "min_observed_over_max_null": ratio})
    assert ks <= KS_BOUND, ks
    assert bool((shifted.p_value == 1.0 / (P_SELF + 1)).all()), shifted.p_value


def test_estimator_method_is_the_two_step_call():
    m, s = 5, 40
    x, th, x_o = _data(m)
    post, twin = _post(x, th), _post(x, th)
    theta_ref = torch.from_numpy(np.random.default_rng(3).normal(size=(m, 33, DTH)).astype(np.float32)).cuda()
    got = post.mmd_batched(theta_ref, x_o, num_posterior_samples=s, kernel="multiscale", num_permutations=9, seed=4)
    draws = twin.sample_batched(x_o, (s,))
    want = mmd_batched(draws, theta_ref, kernel="multiscale", num_permutations=9, seed=4)
    assert post._model.sample_counter == twin._model.sample_counter
    assert (got.n, got.m, got.kernel, got.bandwidths) == (s, 33, "multiscale", want.bandwidths)
    for name in ("mmd2_biased", "mmd2_unbiased", "null", "p_value"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.is_cuda and torch.equal(g, w), name
    dflt = post.mmd_batched(theta_ref, x_o)                      # T draws, rbf, no permutations
    assert (dflt.n, dflt.m, dflt.kernel, dflt.p_value) == (33, 33, "rbf", None)
    with pytest.raises(ValueError):
        post.mmd_batched(theta_ref[:, :, :2], x_o)
    with pytest.raises(ValueError):
        post.mmd_batched(theta_ref[:3], x_o)
