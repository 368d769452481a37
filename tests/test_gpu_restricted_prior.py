"""GPU tests of the restricted prior's device rejection round (include/npfn.h
``npfn_box_propose`` / ``npfn_predict_accept`` / ``npfn_restricted_box_round``) and of
``NPE_PFN_RestrictedPrior`` on the engine classifier (reference restricted_prior.py:8-97).

What is compared with what:
* proposals: bit for bit with the float32 numpy restatement (tests/restricted_ref.py);
* masks, appended rows, counters and the class's samples: exactly with ``npfn_predict_proba``
  on the same engine (itself pinned to the oracle in test_gpu_classifier.py).  With the
  synthetic classifier weights the last-class probability is nearly constant (all of it within
  0.01 of any useful threshold), so a mask comparison with the oracle at the project's 0.01
  tolerance would exclude nearly every row; thresholds are the median of the probabilities at
  hand so that both outcomes occur;
* ``prob_out`` with the bf16-emulating oracle: max |dp| <= 0.01, the bound of
  test_gpu_classifier.py for the same quantity.
"""
import numpy as np
import pytest
import torch
from torch.distributions import Independent, MultivariateNormal, Uniform

import restricted_ref as ref
from npe_pfn.weights import ModelConfig, classifier_config, synthetic_classifier_weights, synthetic_weights
from oracle.tabpfn_oracle import OracleTabPFN

pytestmark = pytest.mark.gpu

CFG = classifier_config()
SEED = 4
LOW = np.array([-1.0, -0.5], dtype=np.float32)
HIGH = np.array([1.0, 1.5], dtype=np.float32)


@pytest.fixture(scope="module")
def cweights():
    return synthetic_classifier_weights(CFG, seed=1)


@pytest.fixture(scope="module")
def cengine(cweights):
    from npe_pfn.engine import Engine

    return Engine(CFG, cweights, device=torch.device("cuda", 0), random_state=SEED, preprocessing="none")


def context(K=2, n=160, seed=0):
    """n rows in the box, label = ring index around the box centre (K = 2: inside a disc)."""
    rng = np.random.default_rng(seed)
    X = (LOW + rng.random((n, 2)).astype(np.float32) * (HIGH - LOW)).astype(np.float32)
    r = np.linalg.norm(X - 0.5 * (LOW + HIGH), axis=1)
    edges = {2: [0.7], 3: [0.5, 0.9]}[K]
    y = (K - 1 - np.digitize(r, edges)).astype(np.float32)  # the last class is the innermost
    assert len(np.unique(y)) == K
    return X, y


def fit(engine, K=2):
    X, y = context(K)
    engine.fit_classes(torch.from_numpy(X), torch.from_numpy(y), K)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def last_prob(engine, rows) -> np.ndarray:
    return engine.predict_proba(torch.from_numpy(np.ascontiguousarray(rows)))[:, -1].cpu().numpy()


# ------------------------------------------------------------------ 1. proposals
@pytest.mark.parametrize("n,dim", [(1, 1), (257, 3), (1000, 5)])
def test_box_propose_bit_equal_to_restatement(cengine, n, dim):
    rng = np.random.default_rng(dim)
    low = rng.uniform(-3, 1, dim).astype(np.float32)
    high = (low + rng.uniform(0.1, 4, dim).astype(np.float32)).astype(np.float32)
    if dim > 1:
        high[1] = low[1]  # a degenerate column
    row_base = 2**32 - 100  # the row's high word changes inside the larger batches
    got = cengine.box_propose(n, dim, torch.from_numpy(low), torch.from_numpy(high), counter=7, row_base=row_base)
    want = ref.proposals(low, high, n, SEED, 7, row_base)
    assert got.shape == (n, dim) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert (got >= low).all() and (got <= high).all()
    assert cengine.box_support(torch.from_numpy(got), torch.from_numpy(low), torch.from_numpy(high)).all()
    if dim > 1:
        assert (got[:, 1] == low[1]).all()
    # rows [a, b) with row_base = a are rows a..b-1 of the whole call; scalar bounds broadcast
    part = cengine.box_propose(n - n // 2, dim, torch.from_numpy(low), torch.from_numpy(high), counter=7,
                               row_base=row_base + n // 2)
    assert np.array_equal(bits(part.cpu().numpy()), bits(want[n // 2:]))
    sc = cengine.box_propose(n, dim, -1.0, 2.0, counter=1)
    assert np.array_equal(bits(sc.cpu().numpy()), bits(ref.proposals([-1.0] * dim, [2.0] * dim, n, SEED, 1)))


def test_box_propose_empty_and_errors(cengine):
    from npe_pfn.engine import EngineError

    assert cengine.box_propose(0, 3, -1.0, 1.0, counter=0).shape == (0, 3)
    with pytest.raises(EngineError, match="row_base"):
        cengine.box_propose(4, 2, -1.0, 1.0, counter=0, row_base=-1)


# ------------------------------------------------------------------ 2. the accept decision
@pytest.mark.parametrize("N,K,chunk", [(1, 2, None), (255, 2, None), (1000, 2, 256), (300, 3, None)])
def test_predict_accept_equals_predict_proba(cengine, N, K, chunk):
    fit(cengine, K)
    Xq = torch.from_numpy(ref.proposals(LOW, HIGH, N, SEED, 11 + K))
    try:
        if chunk:
            cengine.set_chunk_rows(chunk)  # 1000 rows: four chunks
        p = cengine.predict_proba(Xq)
        assert p.shape == (N, K)
        last = p[:, -1]
        thr = float(last.median())
        mask, prob = cengine.predict_accept(Xq, thr, return_prob=True)
        only_mask = cengine.predict_accept(Xq, thr)
        # one row's exact probability as the threshold: strict >, so that row is rejected
        i = N // 3
        at_row = cengine.predict_accept(Xq, float(last[i]))
    finally:
        if chunk:
            cengine.set_chunk_rows(16384)
    assert mask.dtype == torch.bool and mask.shape == (N,)
    assert torch.equal(prob, last)                       # bit-equal (no tolerance)
    assert torch.equal(mask, last > thr) and torch.equal(only_mask, mask)
    if N > 1:
        assert mask.any() and (~mask).any()
    assert not at_row[i] and torch.equal(at_row, last > last[i])
    # the chunked run is the unchunked one
    if chunk:
        assert torch.equal(cengine.predict_accept(Xq, thr), mask)


def test_predict_accept_honours_average_before_softmax(cengine):
    fit(cengine)
    Xq = torch.from_numpy(ref.proposals(LOW, HIGH, 200, SEED, 3))
    try:
        cengine.set_average_before_softmax(True)
        last = cengine.predict_proba(Xq)[:, -1]
        mask, prob = cengine.predict_accept(Xq, float(last.median()), return_prob=True)
    finally:
        cengine.set_average_before_softmax(False)
    assert torch.equal(prob, last) and torch.equal(mask, last > last.median())
    assert not torch.equal(cengine.predict_proba(Xq)[:, -1], last)


# ------------------------------------------------------------------ 3. against the oracle
def test_prob_out_matches_bf16_oracle(cengine, cweights):
    X, y = context(2)
    fit(cengine)
    Xq = ref.proposals(LOW, HIGH, 60, SEED, 5)
    _, prob = cengine.predict_accept(torch.from_numpy(Xq), 0.3, return_prob=True)
    orc = OracleTabPFN(cweights, CFG.n_estimators, CFG.softmax_temperature, seed=SEED, emulate_bf16=True)
    orc.fit_classes(X, y.astype(np.int64), 2)
    err = np.abs(prob.cpu().numpy() - orc.predict_proba(Xq)[:, -1]).max()
    print("max |dp| vs bf16 oracle:", err)
    assert err <= 0.01, err


# ------------------------------------------------------------------ 4. one round
SENTINEL = -7.0


def run_round(engine, thr, n, counter, row_base, theta_out, counts, capacity):
    engine.restricted_box_round(torch.from_numpy(LOW), torch.from_numpy(HIGH), thr, n, counter, row_base, theta_out,
                                counts, capacity=capacity)
    return theta_out.cpu().numpy(), counts.cpu().tolist()


@pytest.fixture(scope="module")
def round_case(cengine):
    """1000 proposals of counter 21, their predict_proba and the median threshold (shared)."""
    fit(cengine)
    rows = ref.proposals(LOW, HIGH, 1000, SEED, 21, 0)
    p = last_prob(cengine, rows)
    thr = float(np.median(p))
    mask = p > np.float32(thr)
    assert 3 < mask.sum() < 1000
    return rows, thr, mask


@pytest.mark.parametrize("cut", [0, 3, None], ids=["capacity=accepted", "capacity=accepted-3", "capacity=0"])
def test_round_appends_accepted_rows_in_order(cengine, round_case, cut):
    rows, thr, mask = round_case
    fit(cengine)
    acc = int(mask.sum())
    capacity = 0 if cut is None else acc - cut
    theta_out = torch.full((acc + 5, 2), SENTINEL, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got, cnt = run_round(cengine, thr, 1000, 21, 0, theta_out, counts, capacity)
    want, want_cnt = ref.append(np.full((acc + 5, 2), SENTINEL, np.float32), [0, 0], rows, mask, capacity)
    assert cnt == want_cnt == [capacity, acc]
    assert np.array_equal(bits(got), bits(want))          # stored rows and the untouched tail
    assert (got[capacity:] == SENTINEL).all()


def test_second_round_appends_behind_the_first(cengine, round_case):
    rows, thr, mask = round_case
    fit(cengine)
    rows2 = ref.proposals(LOW, HIGH, 1000, SEED, 21, 1000)
    mask2 = last_prob(cengine, rows2) > np.float32(thr)
    theta_out = torch.full((2000, 2), SENTINEL, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    run_round(cengine, thr, 1000, 21, 0, theta_out, counts, None)
    got, cnt = run_round(cengine, thr, 1000, 21, 1000, theta_out, counts, None)
    want, c1 = ref.append(np.full((2000, 2), SENTINEL, np.float32), [0, 0], rows, mask, 2000)
    want, c2 = ref.append(want, c1, rows2, mask2, 2000)
    assert cnt == c2 == [int(mask.sum() + mask2.sum())] * 2
    assert np.array_equal(bits(got), bits(want))
    # a full buffer: the round counts, theta_out stays; an empty round changes nothing
    full = torch.from_numpy(want[: c2[0]]).cuda().contiguous()
    counts = torch.tensor([c2[0], c2[0]], dtype=torch.int64, device="cuda")
    got, cnt = run_round(cengine, thr, 1000, 21, 0, full, counts, None)
    assert cnt == [c2[0], c2[0] + int(mask.sum())] and np.array_equal(bits(got), bits(want[: c2[0]]))
    got, cnt2 = run_round(cengine, thr, 0, 21, 0, full, counts, None)
    assert cnt2 == cnt and np.array_equal(bits(got), bits(want[: c2[0]]))


def test_round_of_2500_rows(cengine, round_case):
    _, thr, _ = round_case
    fit(cengine)
    rows = ref.proposals(LOW, HIGH, 2500, SEED, 33, 17)
    mask = last_prob(cengine, rows) > np.float32(thr)
    acc = int(mask.sum())
    assert 0 < acc < 2500
    theta_out = torch.full((acc - 1, 2), SENTINEL, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got, cnt = run_round(cengine, thr, 2500, 33, 17, theta_out, counts, None)
    assert cnt == [acc - 1, acc]
    assert np.array_equal(bits(got), bits(rows[mask][: acc - 1]))


# ------------------------------------------------------------------ 5. the class, box prior
def box_prior():
    return Independent(Uniform(torch.from_numpy(LOW), torch.from_numpy(HIGH)), 1)


def make(cweights, prior, threshold=0.3):
    from npe_pfn import NPE_PFN_RestrictedPrior

    rp = NPE_PFN_RestrictedPrior(prior, acceptance_threshold=threshold,
                                 tabpfn_classifier_kwargs=dict(random_state=SEED, weights=cweights, device="cuda:0",
                                                               preprocessing="none"))
    X, y = context(2)
    rp.append_simulations(torch.from_numpy(X), torch.from_numpy(y))
    return rp


def test_class_box_prior_samples_the_row_stream(cweights):
    rp = make(cweights, box_prior())
    eng = rp.classifier.engine
    thr = float(np.median(last_prob(eng, ref.proposals(LOW, HIGH, 1000, SEED, 0))))
    rp.acceptance_threshold = thr
    predict = lambda rows: last_prob(eng, rows)  # noqa: E731

    s1 = rp.sample((300,), max_sampling_batch_size=256, save_acceptance_rate=True)
    want1, acc1, prop1 = ref.sample_stream(predict, LOW, HIGH, 300, SEED, 0, thr, 256)
    assert s1.shape == (300, 2) and s1.device.type == "cpu"  # the prior's device
    assert np.array_equal(bits(s1.numpy()), bits(want1))
    assert rp.acceptance_rate == acc1 / prop1 and prop1 > 300
    assert rp.accept(s1).all() and rp.sample_counter == 2

    # the next call draws from the next counters; shapes as sample_shape
    s2 = rp.sample((3, 100), max_sampling_batch_size=256)
    want2, _, _ = ref.sample_stream(predict, LOW, HIGH, 300, SEED, 2, thr, 256)
    assert s2.shape == (3, 100, 2)
    assert np.array_equal(bits(s2.reshape(300, 2).numpy()), bits(want2))
    assert not np.array_equal(bits(s2.reshape(300, 2).numpy()), bits(s1.numpy()))

    # a new object repeats the first call, whatever the batch schedule
    rp_b = make(cweights, box_prior(), threshold=thr)
    s1024 = rp_b.sample((300,), max_sampling_batch_size=1024)
    assert np.array_equal(bits(s1024.numpy()), bits(s1.numpy()))


# ------------------------------------------------------------------ 6. the class, another prior
def test_class_generic_prior(cweights):
    prior = MultivariateNormal(torch.tensor([0.0, 0.5]), 0.25 * torch.eye(2))
    rp = make(cweights, prior)
    eng = rp.classifier.engine
    torch.manual_seed(8)
    probe = prior.sample((500,))
    rp.acceptance_threshold = float(eng.predict_proba(probe)[:, -1].median())
    s = rp.sample((200,), max_sampling_batch_size=256, save_acceptance_rate=True)
    assert s.shape == (200, 2) and rp.accept(s).all()
    assert 0.0 < rp.acceptance_rate < 1.0
    assert rp.sample_counter == 0  # the Philox stream is the box path's
    mask = (eng.predict_proba(probe)[:, -1] > rp.acceptance_threshold).cpu()
    assert mask.any() and (~mask).any()
    lp = rp.log_prob(probe)
    assert torch.equal(lp[mask], prior.log_prob(probe)[mask]) and torch.isneginf(lp[~mask]).all()


# ------------------------------------------------------------------ 7. the iteration cap
def test_threshold_one_raises_after_max_iter(cweights):
    rp = make(cweights, box_prior(), threshold=1.0)
    with pytest.raises(RuntimeError, match=r"max_iter_rejection=2.*\b0 of the 50 samples.*306 proposed"):
        rp.sample((50,), max_sampling_batch_size=256, max_iter_rejection=2)


# ------------------------------------------------------------------ 8. entry errors
def test_entry_errors(cengine):
    from npe_pfn.engine import Engine, EngineError

    fit(cengine)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(EngineError, match="features"):
        cengine.restricted_box_round(-1.0, 1.0, 0.3, 10, 0, 0, torch.zeros(4, 3, device="cuda"), counts)
    assert counts.cpu().tolist() == [0, 0]
    with pytest.raises(ValueError, match="capacity"):
        cengine.restricted_box_round(-1.0, 1.0, 0.3, 10, 0, 0, torch.zeros(4, 2, device="cuda"), counts, capacity=5)
    rcfg = ModelConfig()
    reg = Engine(rcfg, synthetic_weights(rcfg, seed=0), device=torch.device("cuda", 0), random_state=SEED,
                 preprocessing="none")
    with pytest.raises(EngineError, match="before fit_classes"):
        reg.predict_accept(torch.zeros(3, 2), 0.3)
    X, y = context(2)
    reg.fit(torch.from_numpy(X), torch.from_numpy(y))
    with pytest.raises(EngineError, match="before fit_classes"):
        reg.predict_accept(torch.zeros(3, 2), 0.3)
    with pytest.raises(EngineError, match="before fit_classes"):
        reg.restricted_box_round(-1.0, 1.0, 0.3, 10, 0, 0, torch.zeros(4, 2, device="cuda"), counts)
