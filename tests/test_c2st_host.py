"""The host definition of the classifier two-sample test (npe_pfn.diagnostics.c2st_*): folds, order,
init, c2st_fit_host against an independent restatement with torch modules, torch.optim.Adam and
autograd, and c2st_batched on CPU tensors at three cases with a known answer.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from npe_pfn.diagnostics import (c2st_adam_table, c2st_batched, c2st_fit_host, c2st_folds, c2st_init, c2st_order,
                                 c2st_widths)
from npe_pfn.engine import (C2ST_MAX_BATCH, C2ST_MAX_DIM, C2ST_MAX_FOLDS, C2ST_MAX_LAYERS, C2ST_MAX_PARAMS,
                            C2ST_MAX_POOL, C2ST_MAX_WIDTH, c2st_param_count, check_c2st_args)


# ------------------------------------------------------------------ folds, order, init
@pytest.mark.parametrize("n,m,n_folds", [(23, 17, 5), (50, 50, 5), (7, 9, 2), (16, 33, 16)])
def test_folds_are_stratified_and_balanced(n, m, n_folds):
    fold = c2st_folds(n, m, n_folds, seed=1)
    assert fold.dtype == torch.uint8 and fold.shape == (n + m,) and int(fold.max()) == n_folds - 1
    for part in (fold, fold[:n], fold[n:]):
        sizes = torch.bincount(part.long(), minlength=n_folds)
        assert int(sizes.max() - sizes.min()) <= 1, sizes
    assert torch.equal(fold, c2st_folds(n, m, n_folds, seed=1))
    assert not torch.equal(fold, c2st_folds(n, m, n_folds, seed=2))


def test_folds_refuse_too_few_points_and_fold_counts():
    for args in ((4, 17, 5), (23, 4, 5), (23, 17, 1), (23, 17, C2ST_MAX_FOLDS + 1)):
        with pytest.raises(ValueError):
            c2st_folds(*args)


def test_order_rows_are_permutations():
    order = c2st_order(40, 7, seed=3)
    assert order.dtype == torch.int32 and order.shape == (7, 40)
    assert torch.equal(order.sort(1).values, torch.arange(40, dtype=torch.int32).expand(7, 40))
    assert not torch.equal(order[0], order[1])
    assert torch.equal(order, c2st_order(40, 7, seed=3)) and not torch.equal(order, c2st_order(40, 7, seed=4))


@pytest.mark.parametrize("model,count", [("mlp", lambda d: 132 * d * d + 32 * d + 2),
                                         ("mlp_small", lambda d: 20 * d * d + 16 * d + 2),
                                         ("linear", lambda d: 2 * d + 2)])
@pytest.mark.parametrize("d", [1, 3, 10])
def test_init_layout_and_bounds(model, count, d):
    widths = c2st_widths(model, d)
    assert widths[0] == d and widths[-1] == 2
    init = c2st_init(widths, seed=5)
    assert init.dtype == torch.float32 and init.shape == (count(d),) == (c2st_param_count(widths),)
    off = 0
    for fan_in, out in zip(widths[:-1], widths[1:]):
        part = init[off:off + out * (fan_in + 1)]
        assert float(part.abs().max()) <= 1.0 / math.sqrt(fan_in)
        if part.numel() >= 64:   # it fills the range: a layer scaled by another layer's fan_in would not
            assert float(part.abs().max()) > 0.8 / math.sqrt(fan_in)
        off += out * (fan_in + 1)
    assert off == init.numel()
    assert torch.equal(init, c2st_init(widths, seed=5)) and not torch.equal(init, c2st_init(widths, seed=6))


def test_widths_are_the_reference_registry():
    assert c2st_widths("mlp", 10) == [10, 40, 80, 80, 40, 2] and c2st_param_count(c2st_widths("mlp", 10)) == 13522
    assert c2st_widths("mlp_small", 3) == [3, 12, 12, 2] and c2st_widths("linear", 7) == [7, 2]
    with pytest.raises(ValueError):
        c2st_widths("forest", 3)


def test_adam_table():
    t = c2st_adam_table(1e-3, 5)
    assert t.dtype == torch.float32 and t.shape == (5, 2)
    want = [[1e-3 / (1 - 0.9 ** k), 1 / math.sqrt(1 - 0.999 ** k)] for k in range(1, 6)]
    assert torch.equal(t, torch.tensor(want, dtype=torch.float64).to(torch.float32))


# ------------------------------------------------------------------ c2st_fit_host against autograd
def restated(z, n_first, fold, order, widths, init, epochs, batch_size, lr, weight_decay):
    """The same training with torch.nn.Linear modules loaded from init, torch.optim.Adam,
    F.cross_entropy and autograd, in float64: (correct [M, F], loss [M, F, E], prob [M, N])."""
    z = z.to(torch.float64)
    M, N, _ = z.shape
    n_folds = int(fold.max()) + 1
    label = (torch.arange(N) >= n_first).long()
    correct = torch.zeros((M, n_folds), dtype=torch.int32)
    loss = torch.zeros((M, n_folds, epochs), dtype=torch.float64)
    prob = torch.zeros((M, N), dtype=torch.float64)
    for u in range(M):
        for f in range(n_folds):
            layers, off = [], 0
            for i, o in zip(widths[:-1], widths[1:]):
                lin = torch.nn.Linear(i, o).double()
                with torch.no_grad():
                    lin.weight.copy_(init[off:off + o * i].view(o, i))
                    lin.bias.copy_(init[off + o * i:off + o * i + o])
                off += o * i + o
                layers += [lin, torch.nn.ReLU()]
            net = torch.nn.Sequential(*layers[:-1])
            opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=weight_decay)
            for e in range(epochs):
                row = order[e].long()
                row = row[fold[row] != f]
                total = 0.0
                for b0 in range(0, row.numel(), batch_size):
                    idx = row[b0:b0 + batch_size]
                    opt.zero_grad()
                    ls = F.cross_entropy(net(z[u, idx]), label[idx])
                    ls.backward()
                    opt.step()
                    total += float(ls.detach()) * idx.numel()
                loss[u, f, e] = total / row.numel()
            held = torch.nonzero(fold == f).reshape(-1)
            with torch.no_grad():
                logits = net(z[u, held])
            prob[u, held] = torch.softmax(logits, 1)[:, 1]
            correct[u, f] = int((logits.argmax(1) == label[held]).sum())
    return correct, loss, prob


HOST_CASES = {
    # d, n, m, model, n_folds, epochs, batch, weight_decay
    "short_last_batch": (3, 50, 45, "mlp", 5, 4, 32, 0.0),
    "batch_above_n_train": (3, 23, 17, "mlp", 5, 5, 64, 0.0),
    "weight_decay": (3, 50, 45, "mlp", 5, 4, 32, 0.01),
    "mlp_small": (4, 40, 40, "mlp_small", 5, 4, 16, 0.0),
    "linear": (5, 40, 30, "linear", 5, 6, 16, 0.0),
    "two_folds": (2, 30, 31, "mlp", 2, 4, 16, 0.0),
    "one_epoch": (3, 50, 45, "mlp", 5, 1, 32, 0.0),
}


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_fit_host_float64_equals_autograd_and_torch_adam(name):
    d, n, m, model, n_folds, epochs, batch, wd = HOST_CASES[name]
    g = torch.Generator().manual_seed(11)
    M = 2
    z = torch.randn((M, n + m, d), generator=g, dtype=torch.float64)
    z[:, n:] += 0.7
    fold, order = c2st_folds(n, m, n_folds, seed=1), c2st_order(n + m, epochs, seed=1)
    widths = c2st_widths(model, d)
    init = c2st_init(widths, seed=1)
    lr = 1e-2
    got = c2st_fit_host(z, n, fold, order, widths, init, epochs, batch, lr, wd, dtype=torch.float64)
    want = restated(z, n, fold, order, widths, init.double(), epochs, batch, lr, wd)
    n_train = (n + m) - torch.bincount(fold.long())
    if name == "short_last_batch":
        assert all(int(t) % batch != 0 and int(t) > batch for t in n_train)
    if name == "batch_above_n_train":
        assert all(int(t) < batch for t in n_train)
    e_loss, e_prob = float((got[1] - want[1]).abs().max()), float((got[2] - want[2]).abs().max())
    print(f"{name}: max |loss diff| {e_loss:.3g}, max |prob diff| {e_prob:.3g}")
    assert got[1].dtype == torch.float64 and got[1].shape == (M, n_folds, epochs) and got[2].shape == (M, n + m)
    assert e_loss <= 1e-9 and e_prob <= 1e-9
    assert torch.equal(got[0], want[0]) and got[3].tolist() == [0, 0]


def test_device_parity_cases_pin_their_predictions():
    """The cases of tests/test_gpu_c2st.py, float64 host alone: at most one held-out point per
    (observation, fold) lies within the case's prob bound of 0.5, and the shapes are what the case
    names say."""
    import c2st_cases as cc

    for name in sorted(cc.CASES):
        z, n, fold, order, widths, init, epochs, batch, lr, wd = cc.inputs(name)
        und = cc.undecided(name)
        for f in range(int(fold.max()) + 1):
            per_obs = und[:, fold == f].sum(1)
            assert int(per_obs.max()) <= 1, (name, f, per_obs)
        h = cc.host(name)
        assert h["f64"][3].tolist() == [0] * cc.N_OBS and bool(torch.isfinite(h["f64"][1]).all())
        print(f"{name}: y(loss) {h['y']['loss']:.3g}, y(prob) {h['y']['prob']:.3g}, undecided {int(und.sum())}")
    n_train = lambda name: sorted(set((cc.inputs(name)[2].numel() - torch.bincount(cc.inputs(name)[2].long())).tolist()))  # noqa: E731
    assert n_train("n_train_at_and_above_batch") == [32, 33] and cc.CASES["n_train_at_and_above_batch"][6] == 32
    assert n_train("n_train_below_and_at_batch") == [32, 33] and cc.CASES["n_train_below_and_at_batch"][6] == 33
    assert max(n_train("batch_above_n_train")) < cc.CASES["batch_above_n_train"][6]
    assert cc.inputs("d11_parameter_cap")[5].numel() == 16326 <= C2ST_MAX_PARAMS < c2st_param_count(c2st_widths("mlp", 12))


# ------------------------------------------------------------------ c2st_batched on CPU tensors
def test_same_distribution_scores_one_half():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((500, 2), generator=g), torch.randn((500, 2), generator=g)
    r = c2st_batched(a, b)
    print(f"same distribution: c2st = {float(r.c2st[0]):.4f}")
    assert r.c2st.shape == (1,) and r.c2st.dtype == torch.float64 and r.fold_accuracy.shape == (1, 5)
    assert r.train_loss.shape == (1, 5, 100) and r.probs is None and (r.n, r.m, r.model, r.seed) == (500, 500, "mlp", 1)
    assert abs(float(r.c2st[0]) - 0.5) <= 5 * math.sqrt(0.25 / 1000)


def test_six_sigma_apart_is_told_apart():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((100, 2), generator=g), torch.randn((100, 2), generator=g)
    b[:, 0] += 6.0
    r = c2st_batched(a, b, return_probs=True)
    print(f"six sigma apart: c2st = {float(r.c2st[0]):.4f}")
    assert float(r.c2st[0]) >= 0.95
    assert r.probs.shape == (1, 200) and float(r.probs[0, :100].mean()) < 0.1 < 0.9 < float(r.probs[0, 100:].mean())


def test_one_sigma_apart_reaches_the_bayes_accuracy():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((500, 1), generator=g), torch.randn((500, 1), generator=g) + 1.0
    r = c2st_batched(a, b)
    bayes = 0.5 * (1 + math.erf(0.5 / math.sqrt(2)))   # Phi(0.5)
    print(f"one sigma apart: c2st = {float(r.c2st[0]):.4f}, Phi(0.5) = {bayes:.4f}")
    assert abs(float(r.c2st[0]) - bayes) <= 4 * math.sqrt(0.69 * 0.31 / 1000) + 0.02


def test_nan_marks_its_observation_only_and_constant_columns_are_kept():
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn((3, 30, 3), generator=g), torch.randn((3, 25, 3), generator=g)
    a[:, :, 2] = 1.5                                   # zero std: counts as 1
    kw = dict(epochs=3, batch_size=16, model="mlp_small", return_probs=True)
    clean = c2st_batched(a, b, **kw)
    assert bool(torch.isfinite(clean.c2st).all()) and bool(torch.isfinite(clean.probs).all())
    a2 = a.clone()
    a2[1, 4, 0] = float("nan")
    r = c2st_batched(a2, b, **kw)
    assert torch.isnan(r.c2st).tolist() == [False, True, False]
    assert bool(torch.isnan(r.fold_accuracy[1]).all() and torch.isnan(r.train_loss[1]).all()
                and torch.isnan(r.probs[1]).all())
    for u in (0, 2):
        assert torch.equal(r.c2st[u], clean.c2st[u]) and torch.equal(r.probs[u], clean.probs[u])
        assert torch.equal(r.train_loss[u], clean.train_loss[u])
    one = c2st_batched(a[0], b[0], **kw)               # 2-D inputs: M = 1
    assert torch.equal(one.c2st, clean.c2st[:1])


def test_check_c2st_args_refuses_each_cap():
    ok = dict(z_shape=(2, 40, 3), n_first=20, widths=[3, 12, 2], n_folds=5, epochs=3, batch_size=16)
    assert check_c2st_args(**ok) == (2, 40, 3, 3 * 12 + 12 + 12 * 2 + 2)
    d_mlp = 12   # 'mlp' at d = 12 has 19394 parameters
    for kw in (dict(z_shape=(2, 40)), dict(z_shape=(2, 40, 0), widths=[0, 2]),
               dict(z_shape=(2, 40, C2ST_MAX_DIM + 1), widths=[C2ST_MAX_DIM + 1, 2]),
               dict(z_shape=(2, 1, 3)), dict(z_shape=(2, C2ST_MAX_POOL + 1, 3)), dict(n_first=0), dict(n_first=40),
               dict(widths=[3]), dict(widths=[3] + [4] * C2ST_MAX_LAYERS + [2]), dict(widths=[3, 12, 3]),
               dict(widths=[4, 12, 2]), dict(widths=[3, C2ST_MAX_WIDTH + 1, 2]), dict(widths=[3, 0, 2]),
               dict(z_shape=(2, 40, d_mlp), widths=c2st_widths("mlp", d_mlp)),
               dict(n_folds=1), dict(n_folds=C2ST_MAX_FOLDS + 1), dict(epochs=0), dict(batch_size=0),
               dict(batch_size=C2ST_MAX_BATCH + 1)):
        with pytest.raises(ValueError, match="c2st_fit"):
            check_c2st_args(**dict(ok, **kw))
    # the caps the documents state: 'mlp' to d = 11, 'mlp_small' to d = 28, 'linear' to d = 64
    for model, d in (("mlp", 11), ("mlp_small", 28), ("linear", 64)):
        assert check_c2st_args((1, 40, d), 20, c2st_widths(model, d), 5, 1, 128)[3] <= C2ST_MAX_PARAMS
    for model, d in (("mlp", 12), ("mlp_small", 29)):
        with pytest.raises(ValueError, match=str(C2ST_MAX_PARAMS)):
            c2st_batched(torch.zeros(1, 20, d), torch.zeros(1, 20, d), model=model)
