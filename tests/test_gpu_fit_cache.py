"""The fit cache (npfn_set_fit_cache): per-step fits kept across fit tokens, found again by the
content of the context table.

A call under a new token compares its context table with the cached sets of equal key, on the
32-bit patterns, and refits only what no set holds.  Whatever the cache decides, the results
must be bit for bit those of a fresh engine: every case compares target tokens
(npfn_ar_fit_begin / _step + npfn_forward_targets) or draws (npfn_ar_sample) with a fresh
engine's, with ``torch.equal``, and reads the cache's decisions from npfn_fit_cache_stats,
never from timing.  Sizes as in tests/test_gpu_fit_reuse.py."""
import numpy as np
import pytest
import torch

from npe_pfn.tasks import gaussian_linear_prior, gaussian_linear_task
from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
DEV = torch.device("cuda", 0)
_TOKENS = iter(range(5000, 10**9))


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(CFG, seed=0)


def _task(dth, n, seed):
    th, x, _ = gaussian_linear_task(dth, n, seed=seed)
    return x.to(DEV).contiguous(), th.to(DEV).contiguous()


def _engine(weights, pre="ensemble", sets=None, max_bytes=0):
    from npe_pfn.engine import Engine

    e = Engine(CFG, weights, device=DEV, random_state=3, preprocessing=pre)
    if sets is not None:
        e.set_fit_cache(sets, max_bytes)
    return e


def _bits(t):
    """bf16 tokens as integers: NaN tokens (a context with NaN cells) compare by pattern."""
    return t.view(torch.int16)


def _fresh(weights, x, theta, xq, pre="ensemble", est_set=None, steps=None):
    """Every step's tokens from a fresh engine's npfn_fit (no token, no cache)."""
    e = _engine(weights, pre)
    if est_set is not None:
        e.set_estimator_set(*est_set)
    joint = torch.cat([x, theta], 1)
    dx = x.shape[1]
    out = []
    for k in range(theta.shape[1] if steps is None else steps):
        e.fit(joint[:, : dx + k], joint[:, dx + k])
        out.append(e.forward_targets(torch.cat([xq, theta[: xq.shape[0], :k]], 1)))
    return out


def _steps(e, x, theta, xq, steps=None):
    """Every step's tokens through the per-step slots, under a new fit token."""
    e.set_fit_token(next(_TOKENS))
    try:
        e.ar_fit_begin(x, theta)
        out = []
        for k in range(theta.shape[1] if steps is None else steps):
            e.ar_fit_step(k)
            out.append(e.forward_targets(torch.cat([xq, theta[: xq.shape[0], :k]], 1)))
    finally:
        e.set_fit_token(0)
    return out


def _same(got, want):
    assert len(got) == len(want)
    return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))


def _hm(e):
    s = e.fit_cache_stats()
    return s["hits"], s["misses"]


def test_same_content_new_token_new_address_hits(weights):
    x, th = _task(2, 200, seed=1)
    xq = x[:40]
    e = _engine(weights)
    a = _steps(e, x, th, xq)
    assert _hm(e) == (0, 1)
    b = _steps(e, x.clone(), th.clone(), xq)
    assert _hm(e) == (1, 1)
    want = _fresh(weights, x, th, xq)
    assert _same(a, want) and _same(b, want)
    st = e.fit_cache_stats()
    assert st["sets"] == 1 and st["bytes"] > x.numel() * 4


def test_one_changed_cell_misses(weights):
    """The last cell of the table moved by one ulp; a +0.0 cell turned into -0.0."""
    x, th = _task(2, 200, seed=2)
    x[7, 1] = 0.0
    xq = x[:40]
    e = _engine(weights)
    _steps(e, x, th, xq)
    th2 = th.clone()
    th2[-1, -1] = float(np.nextafter(np.float32(th[-1, -1].item()), np.float32(np.inf)))
    assert th2[-1, -1] != th[-1, -1]
    got = _steps(e, x, th2, xq)
    assert _hm(e) == (0, 2)
    assert _same(got, _fresh(weights, x, th2, xq))
    _steps(e, x, th, xq)                       # back to the first table (one set: a miss)
    assert _hm(e) == (0, 3)
    x3 = x.clone()
    x3[7, 1] = -0.0
    assert torch.equal(x3, x) and not torch.equal(x3.view(torch.int32), x.view(torch.int32))
    got = _steps(e, x3, th, xq)
    assert _hm(e) == (0, 4)
    assert _same(got, _fresh(weights, x3, th, xq))


def test_nan_cells_hit_by_bit_pattern(weights):
    x, th = _task(2, 200, seed=3)
    x[3, 0] = float("nan")
    x[150, 1] = float("nan")
    xq = x[10:50]
    e = _engine(weights, pre="none")
    a = _steps(e, x, th, xq)
    b = _steps(e, x.clone(), th.clone(), xq)
    assert _hm(e) == (1, 1)
    want = _fresh(weights, x, th, xq, pre="none")
    assert _same(a, want) and _same(b, want)


def test_in_place_rewrite_misses(weights):
    """The same tensor objects, rewritten in place between two tokens: never keyed by address."""
    x, th = _task(1, 180, seed=4)
    x2, th2 = _task(1, 180, seed=5)
    xq = x[:30].clone()
    e = _engine(weights)
    _steps(e, x, th, xq)
    x.copy_(x2)
    th.copy_(th2)
    got = _steps(e, x, th, xq)
    assert _hm(e) == (0, 2)
    assert _same(got, _fresh(weights, x2, th2, xq))


@pytest.mark.parametrize("sets", [1, 2])
def test_alternating_contexts(weights, sets):
    xa, tha = _task(2, 200, seed=6)
    xb, thb = _task(2, 200, seed=7)
    xq = xa[:30]
    e = _engine(weights, sets=sets)
    a1 = _steps(e, xa, tha, xq)
    b = _steps(e, xb, thb, xq)
    a2 = _steps(e, xa, tha, xq)
    assert _hm(e) == ((0, 3) if sets == 1 else (1, 2))
    assert e.fit_cache_stats()["sets"] == sets
    want_a = _fresh(weights, xa, tha, xq)
    assert _same(a1, want_a) and _same(a2, want_a)
    assert _same(b, _fresh(weights, xb, thb, xq))


def test_byte_limit_evicts_least_recently_used(weights):
    xa, tha = _task(2, 200, seed=8)
    xb, thb = _task(2, 200, seed=9)
    xq = xa[:30]
    e = _engine(weights, sets=2)
    _steps(e, xa, tha, xq)
    one = e.fit_cache_stats()["bytes"]
    assert one > 0
    limit = one + one // 2                      # room for one set, not for two
    e.set_fit_cache(2, limit)
    b = _steps(e, xb, thb, xq)
    st = e.fit_cache_stats()
    assert 0 < st["bytes"] <= limit and st["sets"] == 1, st
    assert _hm(e) == (0, 2)
    b2 = _steps(e, xb, thb, xq)                 # B stayed ...
    assert _hm(e) == (1, 2)
    a = _steps(e, xa, tha, xq)                  # ... A, the least recently used, is gone
    assert _hm(e) == (1, 3)
    st = e.fit_cache_stats()
    assert 0 < st["bytes"] <= limit and st["sets"] == 1, st
    want_b = _fresh(weights, xb, thb, xq)
    assert _same(b, want_b) and _same(b2, want_b)
    assert _same(a, _fresh(weights, xa, tha, xq))


def test_partially_filled_set_fits_only_the_missing_step(weights):
    """Steps 0-1 of a 3-dimensional context under one token, steps 0-2 under the next.  With the
    live profiler on the fits run in order, so the first token leaves step 2 unfitted and the
    number of fits of the second token can be read from the kernel table."""
    x, th = _task(3, 250, seed=10)
    xq = x[:40]
    e = _engine(weights)
    e.prof_read()
    e.prof_enable(True)
    a = _steps(e, x, th, xq, steps=2)
    first = {p["name"]: p["launches"] for p in e.prof_read()}["k_col_stats+k_build_params"]
    b = _steps(e, x.clone(), th.clone(), xq)
    e.prof_enable(False)
    second = {p["name"]: p["launches"] for p in e.prof_read()}.get("k_col_stats+k_build_params", 0)
    assert _hm(e) == (1, 1)
    assert (first, second) == (2, 1), (first, second)
    want = _fresh(weights, x, th, xq)
    assert _same(a, want[:2]) and _same(b, want)
    # the same without the profiler: the first token's fits are queued ahead on the side streams
    e2 = _engine(weights)
    a = _steps(e2, x, th, xq, steps=2)
    b = _steps(e2, x.clone(), th.clone(), xq)
    assert _hm(e2) == (1, 1)
    assert _same(a, want[:2]) and _same(b, want)


def test_invalidation_by_preprocessing_estimator_set_and_pipelines(weights):
    x, th = _task(2, 200, seed=11)
    xq = x[:40]
    # preprocessing mode: every cached fit is forgotten
    e = _engine(weights)
    _steps(e, x, th, xq)
    e.set_preprocessing("quantile")
    got = _steps(e, x, th, xq)
    assert _hm(e) == (0, 2)
    assert _same(got, _fresh(weights, x, th, xq, pre="quantile"))
    # estimator set: part of the key -- another set misses, the first one is found again
    e = _engine(weights, sets=2)
    e.set_estimator_set(0, 4, 2)
    a1 = _steps(e, x, th, xq)
    e.set_estimator_set(1, 4, 2)
    b = _steps(e, x, th, xq)
    assert _hm(e) == (0, 2)
    e.set_estimator_set(0, 4, 2)
    a2 = _steps(e, x, th, xq)
    assert _hm(e) == (1, 2)
    want_a = _fresh(weights, x, th, xq, est_set=(0, 4, 2))
    assert _same(a1, want_a) and _same(a2, want_a)
    assert _same(b, _fresh(weights, x, th, xq, est_set=(1, 4, 2)))
    # regressor vs classifier pipelines (the ensemble's differ): a classifier fit in between
    from npe_pfn.engine import Engine
    from npe_pfn.weights import classifier_config, synthetic_classifier_weights

    ccfg = classifier_config(CFG.n_estimators, CFG.softmax_temperature)
    cw = synthetic_classifier_weights(ccfg, seed=1)
    joint = torch.cat([x, th], 1)
    dx = x.shape[1]

    def reg_tokens(eng, tokened):
        out = []
        if tokened:
            eng.set_fit_token(next(_TOKENS))
            eng.ar_fit_begin(x, th)
        for k in range(th.shape[1]):
            if tokened:
                eng.ar_fit_step(k)
            else:
                eng.fit(joint[:, : dx + k], joint[:, dx + k])
            out.append(eng.forward_targets(torch.cat([xq, th[: xq.shape[0], :k]], 1)))
        eng.set_fit_token(0)
        return out

    e = Engine(ccfg, cw, device=DEV, random_state=3)
    first = reg_tokens(e, True)
    e.fit_classes(x, (th[:, 0] > 0).to(torch.float32), 2)
    second = reg_tokens(e, True)
    assert _hm(e) == (0, 2)
    want = reg_tokens(Engine(ccfg, cw, device=DEV, random_state=3), False)
    assert _same(first, want) and _same(second, want)


def test_max_sets_zero_never_reuses_across_tokens(weights):
    x, th = _task(2, 200, seed=12)
    xq = x[:30]
    e = _engine(weights, sets=0)
    a = _steps(e, x, th, xq)
    b = _steps(e, x, th, xq)
    c = _steps(e, x, th, xq)
    assert _hm(e) == (0, 3)
    want = _fresh(weights, x, th, xq)
    assert _same(a, want) and _same(b, want) and _same(c, want)
    e.set_fit_cache(1)                          # switched on: the old set has no table to compare
    d = _steps(e, x, th, xq)
    f = _steps(e, x, th, xq)
    assert _hm(e) == (1, 4)
    assert _same(d, want) and _same(f, want)


def test_two_streams_without_host_synchronisation(weights):
    x, th = _task(3, 250, seed=13)
    xq = x[:50].contiguous()
    ref = _engine(weights)
    ref.set_fit_token(next(_TOKENS))
    want, want_lp = ref.ar_sample(x, th, xq, counter=2, with_log_prob=True)
    ref.set_fit_token(0)
    e = _engine(weights)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()                    # the inputs are complete; nothing below waits on the host
    with torch.cuda.stream(s1):
        e.set_fit_token(next(_TOKENS))
        a, a_lp = e.ar_sample(x, th, xq, counter=2, with_log_prob=True)
    with torch.cuda.stream(s2):
        e.set_fit_token(next(_TOKENS))
        b, b_lp = e.ar_sample(x.clone(), th.clone(), xq, counter=2, with_log_prob=True)
    e.set_fit_token(0)
    torch.cuda.synchronize()
    assert _hm(e) == (1, 1)
    assert torch.equal(a, want) and torch.equal(a_lp, want_lp)
    assert torch.equal(b, want) and torch.equal(b_lp, want_lp)


def test_public_sample_path(weights):
    from npe_pfn import TabPFN_Based_NPE_PFN

    def posterior(theta, x):
        p = TabPFN_Based_NPE_PFN(prior=gaussian_linear_prior(2, device=DEV),
                                 regressor_init_kwargs={"random_state": 3, "device": DEV})
        return p.append_simulations(theta, x)

    def draw(p, x_o):
        p._model.sample_counter = 0
        return p.sample((64,), x=x_o)

    th, x, x_o = (t.to(DEV) for t in gaussian_linear_task(2, 200, seed=14))
    th_more, x_more, _ = (t.to(DEV) for t in gaussian_linear_task(2, 230, seed=15))
    th_other, x_other, _ = (t.to(DEV) for t in gaussian_linear_task(2, 200, seed=16))
    post = posterior(th, x)
    eng = post._model.engine
    first = draw(post, x_o)
    assert _hm(eng) == (0, 1)
    second = draw(post, x_o)
    assert _hm(eng) == (1, 1)
    assert torch.equal(first, second)
    assert torch.equal(first, draw(posterior(th, x), x_o))
    post.append_simulations(th_more, x_more)           # more rows: a miss by shape
    got = draw(post, x_o)
    assert _hm(eng) == (1, 2)
    assert torch.equal(got, draw(posterior(th_more, x_more), x_o))
    post.append_simulations(th_other, x_other)         # same shape as the first: a miss by content
    got = draw(post, x_o)
    assert _hm(eng) == (1, 3)
    assert torch.equal(got, draw(posterior(th_other, x_other), x_o))


def test_unconditional_estimator_keeps_every_cluster(weights):
    from npe_pfn import TabPFN_Based_Uncond_Estimator

    torch.manual_seed(5)
    which = torch.arange(600) % 3
    centres = torch.tensor([[-6.0, 0.0], [6.0, 0.0], [0.0, 9.0]])
    theta = (centres[which] + torch.randn(600, 2)).to(DEV)
    est = TabPFN_Based_Uncond_Estimator(num_clusters=3, regressor_init_kwargs={"random_state": 2, "device": DEV})
    est.append_simulations(theta)
    eng = est._model.engine

    def draw():
        torch.manual_seed(7)
        np.random.seed(7)
        est._model.sample_counter = 0
        return est.sample(torch.Size([90, 1]), with_log_prob=True)

    s1, lp1 = draw()
    assert _hm(eng) == (0, 3)
    s2, lp2 = draw()
    assert _hm(eng) == (3, 3)
    assert torch.equal(s1, s2) and torch.equal(lp1, lp2)
    assert eng.fit_cache_stats()["sets"] == 3
    est.log_prob(s1)                                   # scoring finds the same clusters' fits
    assert _hm(eng)[1] == 3
    # the sizing lives on the regressor: an unpickled estimator rebuilds its engine with it
    import pickle

    est = pickle.loads(pickle.dumps(est))
    assert est._model._engine is None and est._model.fit_cache_sets == 3
    eng = est._model.engine
    s3, lp3 = draw()
    s4, lp4 = draw()
    assert _hm(eng) == (3, 3)
    assert torch.equal(s3, s1) and torch.equal(s4, s1) and torch.equal(lp4, lp1)
    # fit_cache_sets=0 is the caller's choice and stays: every cluster visit refits
    est = TabPFN_Based_Uncond_Estimator(num_clusters=3, regressor_init_kwargs={"random_state": 2, "device": DEV,
                                                                                "fit_cache_sets": 0})
    est.append_simulations(theta)
    eng = est._model.engine
    s5, _ = draw()
    s6, _ = draw()
    assert _hm(eng) == (0, 6)
    assert torch.equal(s5, s6)
