"""npfn_c2st_fit (npe_pfn.diagnostics.c2st_batched on the GPU) against its host definition
(c2st_fit_host at float64), its reproducibility, refusals and bad flags, three cases with a known
answer, and the estimator methods.  The parity cases and their bounds: tests/c2st_cases.py."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import c2st_cases as cc
from npe_pfn.diagnostics import c2st_batched
from npe_pfn.weights import ModelConfig

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
N_CTX, DX, DTH = 150, 3, 3   # the tiny fitted estimator of tests/test_gpu_two_sample.py
SEED = 2
# NPFN_C2ST_PARITY_OUT=<file>: the parity tests merge their ratios into that JSON file
# (profiles/c2st/parity.json was written this way)
PARITY_OUT = os.environ.get("NPFN_C2ST_PARITY_OUT")


def merge_json(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    json.dump(doc, open(path, "w"), indent=1, sort_keys=True)


def gpu_fit(z, n_first, fold, order, widths, init, epochs, batch, lr, wd, **kw):
    from npe_pfn.engine import c2st_fit

    out = c2st_fit(z.cuda(), n_first, fold, order, widths, init, epochs, batch, lr, wd, return_probs=True,
                   return_params=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


# ------------------------------------------------------------------ the kernel against the definition
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_kernel_against_the_definition(name):
    """loss and prob within 16 max(|host float32 - host float64|, 2^-24) of the float64 host;
    correct equal to the float64 host's count, the points within the prob bound of 0.5 set aside."""
    args = cc.inputs(name)
    z, n, fold, widths, init = args[0], args[1], args[2], args[4], args[5]
    h = cc.host(name)
    correct, loss, prob, params, bad = gpu_fit(*args)
    assert bad.tolist() == [0] * cc.N_OBS
    err = {"loss": float((loss.double() - h["f64"][1]).abs().max()), "prob": float((prob.double() - h["f64"][2]).abs().max())}
    ratio = {k: err[k] / h["bound"][k] for k in err}
    print(f"{name}: |device - f64| loss {err['loss']:.3g} prob {err['prob']:.3g}; |f32 - f64| loss {h['y']['loss']:.3g} "
          f"prob {h['y']['prob']:.3g}; device / bound loss {ratio['loss']:.3f} prob {ratio['prob']:.3f}")
    if PARITY_OUT:
        merge_json(PARITY_OUT, name, {"host_f32_minus_f64": h["y"], "device_minus_f64": err, "bound": h["bound"],
                                      "device_over_bound": ratio, "margin": cc.MARGIN})
    assert ratio["loss"] <= 1.0 and ratio["prob"] <= 1.0, (err, h["bound"])

    und = cc.undecided(name)
    label = torch.arange(z.shape[1]) >= n
    decided_equal = ((prob > 0.5) == (h["f64"][2] > 0.5)) | und
    assert bool(decided_equal.all())
    for f in range(int(fold.max()) + 1):
        slack = und[:, fold == f].sum(1)
        assert int(slack.max()) <= 1
        diff = (correct[:, f] - h["f64"][0][:, f]).abs()
        assert bool((diff <= slack).all()), (name, f, correct[:, f], h["f64"][0][:, f], slack)
        # the count is the count of the device's own predictions
        sure = ~und[:, fold == f]
        mine = (((prob[:, fold == f] > 0.5) == label[fold == f]) & sure).sum(1)
        assert bool(((correct[:, f] - mine) >= 0).all() and ((correct[:, f] - mine) <= slack).all())

    if name == "dead_layer":
        # no ReLU of the dead layer fires: exactly zero gradients up to and including the weights that
        # read its outputs, so those parameters are the init to the bit in every fold
        sl = cc.layer_slices(widths)
        frozen = torch.cat([torch.arange(init.numel())[s] for l in range(cc.DEAD_LAYER + 1) for s in sl[l]]
                           + [torch.arange(init.numel())[sl[cc.DEAD_LAYER + 1][0]]])
        assert torch.equal(params[:, :, frozen], init[frozen].expand(cc.N_OBS, params.shape[1], -1))
        moved = torch.arange(init.numel())[sl[-1][1]]
        assert not torch.equal(params[:, :, moved], init[moved].expand(cc.N_OBS, params.shape[1], -1))


def test_same_bits_twice_alone_and_among_others():
    d, n, m, epochs, batch = 3, 23, 17, 2, 16
    g = torch.Generator().manual_seed(5)
    z = torch.randn((3, n + m, d), generator=g)
    z[:, n:] += 0.5
    from npe_pfn.diagnostics import c2st_folds, c2st_init, c2st_order, c2st_widths

    widths = c2st_widths("mlp", d)
    rest = (n, c2st_folds(n, m, 5, 1), c2st_order(n + m, epochs, 1), widths, c2st_init(widths, 1), epochs, batch, 1e-2, 0.0)
    first, second = gpu_fit(z, *rest), gpu_fit(z, *rest)
    assert first[4].tolist() == [0, 0, 0] and float(first[3].abs().sum()) > 0
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for u in range(3):
        alone = gpu_fit(z[u:u + 1], *rest)
        for a, b in zip(first, alone):
            assert torch.equal(a[u:u + 1], b), u


def test_non_finite_coordinates_raise_bad():
    d, n, m, epochs, batch = 2, 12, 11, 2, 16
    g = torch.Generator().manual_seed(6)
    z = torch.randn((4, n + m, d), generator=g)
    from npe_pfn.diagnostics import c2st_folds, c2st_init, c2st_order, c2st_widths

    widths = c2st_widths("mlp_small", d)
    rest = (n, c2st_folds(n, m, 5, 1), c2st_order(n + m, epochs, 1), widths, c2st_init(widths, 1), epochs, batch, 1e-2, 0.0)
    clean = gpu_fit(z, *rest)
    z2 = z.clone()
    z2[1, 3, 1], z2[2, n + m - 1, 0] = float("nan"), float("inf")
    got = gpu_fit(z2, *rest)
    assert got[4].tolist() == [0, 1, 1, 0] and clean[4].tolist() == [0, 0, 0, 0]
    for a, b in zip(got[:4], clean[:4]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    r = c2st_batched(z2[:, :n].cuda(), z2[:, n:].cuda(), epochs=2, batch_size=16, model="mlp_small", z_score=False,
                     return_probs=True)
    assert r.c2st.is_cuda and torch.isnan(r.c2st).tolist() == [False, True, True, False]
    assert bool(torch.isnan(r.probs[1]).all() and torch.isnan(r.train_loss[2]).all() and torch.isnan(r.fold_accuracy[1]).all())
    assert bool(torch.isfinite(r.probs[0]).all() and torch.isfinite(r.train_loss[3]).all())


def test_rejected_arguments():
    from npe_pfn.engine import C2ST_MAX_PARAMS, c2st_param_count, load_library

    lib = load_library()
    n_obs, n_pool, dim, n_folds, epochs, ld = 2, 10, 3, 2, 2, 5
    z = torch.zeros((n_obs, n_pool, 64), device="cuda")
    init = torch.zeros((C2ST_MAX_PARAMS + 8192,), device="cuda")
    fold = torch.tensor([0, 1] * 5, dtype=torch.uint8, device="cuda")
    order = torch.arange(ld, dtype=torch.int32, device="cuda").repeat(n_folds, epochs, 1).contiguous()
    adam = torch.ones((epochs * 2, 2), device="cuda")           # two batches per epoch
    correct = torch.full((n_obs, n_folds), 7, dtype=torch.int32, device="cuda")
    loss = torch.full((n_obs, n_folds, epochs), 7.0, device="cuda")
    prob = torch.full((n_obs, n_pool), 7.0, device="cuda")
    bad = torch.full((n_obs,), 7, dtype=torch.int32, device="cuda")
    good = dict(z=z.data_ptr(), n_obs=n_obs, n_pool=n_pool, n_first=5, dim=dim, widths=[3, 4, 2], n_layers=None,
                init=init.data_ptr(), fold=fold.data_ptr(), n_folds=n_folds, order=order.data_ptr(), n_train=[5, 5],
                order_ld=ld, epochs=epochs, batch=4, adam=adam.data_ptr(), correct=correct.data_ptr(),
                loss=loss.data_ptr(), prob=prob.data_ptr(), bad=bad.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        vp = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
        ip = lambda p: ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_int32)) if p else None  # noqa: E731
        arr = lambda v: (ctypes.c_int32 * len(v))(*v) if v is not None else None  # noqa: E731
        n_layers = len(a["widths"]) - 1 if a["n_layers"] is None else a["n_layers"]
        rc = lib.npfn_c2st_fit(vp(a["z"]), a["n_obs"], a["n_pool"], a["n_first"], a["dim"], arr(a["widths"]), n_layers,
                               vp(a["init"]), vp(a["fold"]), a["n_folds"], ip(a["order"]), arr(a["n_train"]),
                               a["order_ld"], a["epochs"], a["batch"], vp(a["adam"]), 0.9, 0.999, 1e-8, 0.0,
                               ip(a["correct"]), vp(a["loss"]), vp(a["prob"]), None, ip(a["bad"]), None)
        return rc, (lib.npfn_last_error() or b"").decode()

    wide = [64, 128, 128, 2]
    assert c2st_param_count(wide) > C2ST_MAX_PARAMS
    for kw in (dict(n_obs=-1), dict(dim=0, widths=[0, 4, 2]), dict(dim=65, widths=[65, 2]), dict(n_pool=1),
               dict(n_pool=32769), dict(n_first=0), dict(n_first=10), dict(widths=[3], n_layers=0),
               dict(widths=[3, 4, 4, 4, 4, 4, 2]), dict(widths=[3, 4, 3]), dict(widths=[4, 4, 2]),
               dict(widths=[3, 129, 2]), dict(widths=[3, 0, 2]), dict(dim=64, widths=wide), dict(n_folds=1),
               dict(n_folds=17, n_train=[5] * 17), dict(epochs=0), dict(batch=0), dict(batch=4097),
               dict(n_train=[5, 6]), dict(n_train=[0, 5]), dict(z=0), dict(widths=None, n_layers=2), dict(init=0),
               dict(fold=0), dict(order=0), dict(n_train=None), dict(adam=0), dict(correct=0), dict(loss=0), dict(bad=0)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("c2st_fit"), (kw, rc, msg)   # NPFN_EINVAL
    torch.cuda.synchronize()
    untouched = lambda: (int((correct != 7).sum()) + int((loss != 7).sum()) + int((prob != 7).sum())  # noqa: E731
                         + int((bad != 7).sum())) == 0
    assert untouched()                                          # nothing ran
    assert call(n_obs=0)[0] == 0
    torch.cuda.synchronize()
    assert untouched()
    assert call(prob=0)[0] == 0                                 # prob may be missing; the call zeroes the rest
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0] and int((prob != 7).sum()) == 0 and int((loss == 7).sum()) == 0
    assert bool(((correct >= 0) & (correct <= 5)).all())


def test_python_entry_refuses_what_the_call_refuses():
    from npe_pfn.engine import c2st_fit

    args = cc.inputs("d3")
    with pytest.raises(ValueError):
        c2st_fit(*args)                                         # CPU tensors: not this entry's business
    z = args[0].cuda()
    for bad_args in ((z[0],) + args[1:], (z, 0) + args[2:], (z, args[1], args[2][:-1]) + args[3:],
                     (z,) + args[1:3] + (args[3][:1],) + args[4:], (z,) + args[1:5] + (args[5][:-1],) + args[6:],
                     (z,) + args[1:7] + (5000,) + args[8:]):
        with pytest.raises(ValueError):
            c2st_fit(*bad_args)
    with pytest.raises(ValueError, match="16384"):
        c2st_batched(torch.zeros(1, 20, 12).cuda(), torch.zeros(1, 20, 12).cuda())


# ------------------------------------------------------------------ three cases with a known answer
def test_known_answers_on_the_device():
    """The three cases of tests/test_c2st_host.py, same data and bounds, through the kernel."""
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((500, 2), generator=g), torch.randn((500, 2), generator=g)
    same = c2st_batched(a.cuda(), b.cuda())
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((100, 2), generator=g), torch.randn((100, 2), generator=g)
    b[:, 0] += 6.0
    far = c2st_batched(a.cuda(), b.cuda(), return_probs=True)
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((500, 1), generator=g), torch.randn((500, 1), generator=g) + 1.0
    near = c2st_batched(a.cuda(), b.cuda())
    bayes = 0.5 * (1 + math.erf(0.5 / math.sqrt(2)))
    print(f"same {float(same.c2st[0]):.4f}, six sigma {float(far.c2st[0]):.4f}, one sigma {float(near.c2st[0]):.4f} "
          f"(Phi(0.5) = {bayes:.4f})")
    if PARITY_OUT:
        merge_json(PARITY_OUT, "known_answers", {"same_distribution": float(same.c2st[0]), "six_sigma": float(far.c2st[0]),
                                                 "one_sigma": float(near.c2st[0]), "bayes_one_sigma": bayes})
    assert same.c2st.is_cuda and same.c2st.dtype == torch.float64 and same.train_loss.shape == (1, 5, 100)
    assert abs(float(same.c2st[0]) - 0.5) <= 5 * math.sqrt(0.25 / 1000)
    assert float(far.c2st[0]) >= 0.95 and far.probs.shape == (1, 200)
    assert abs(float(near.c2st[0]) - bayes) <= 4 * math.sqrt(0.69 * 0.31 / 1000) + 0.02


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


def test_estimator_method_is_the_two_step_call():
    m, s = 4, 40
    x, th, x_o = _data(m)
    post, twin = _post(x, th), _post(x, th)
    theta_ref = torch.from_numpy(np.random.default_rng(3).normal(size=(m, 33, DTH)).astype(np.float32)).cuda()
    kw = dict(epochs=10, batch_size=32, seed=4, return_probs=True)
    got = post.c2st_batched(theta_ref, x_o, num_posterior_samples=s, **kw)
    draws = twin.sample_batched(x_o, (s,))
    want = c2st_batched(draws, theta_ref, **kw)
    assert post._model.sample_counter == twin._model.sample_counter
    assert (got.n, got.m, got.model, got.seed) == (s, 33, "mlp", 4)
    assert got.c2st.shape == (m,) and got.fold_accuracy.shape == (m, 5) and got.train_loss.shape == (m, 5, 10)
    assert got.probs.shape == (m, s + 33) and torch.equal(got.fold, want.fold)
    for name in ("c2st", "fold_accuracy", "train_loss", "probs"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.is_cuda and torch.equal(g, w), name
    assert bool(((got.c2st >= 0) & (got.c2st <= 1)).all())
    dflt = post.c2st_batched(theta_ref, x_o, epochs=2)          # T draws per observation
    assert (dflt.n, dflt.m, dflt.probs) == (33, 33, None)
    with pytest.raises(ValueError):
        post.c2st_batched(theta_ref[:, :, :2], x_o)
    with pytest.raises(ValueError):
        post.c2st_batched(theta_ref[:3], x_o)


def test_unconditional_estimator_points_to_the_function():
    from npe_pfn.npe_pfn import TabPFN_Based_Uncond_Estimator

    with pytest.raises(NotImplementedError, match="c2st_batched"):
        TabPFN_Based_Uncond_Estimator.c2st_batched(object(), torch.zeros(1, 4, 3))
