"""GPU: npfn_ar_score -- the per-step log densities and PIT values of the teacher-forced pass.

150 context rows, dim_x = 3, dim_theta = 3, preprocessing "none" and "ensemble"; everything the
tests read is computed once per mode (fixture ``runs``).
"""
import numpy as np
import pytest
import torch

from bar_cdf_ref import cdf_from_probs
from npe_pfn.diagnostics import pit_ks_statistic
from npe_pfn.weights import ModelConfig, synthetic_weights
from oracle.tabpfn_oracle import OracleTabPFN

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
MODES = {"none": 0, "ensemble": 3}
N_CTX, DX, DTH, N = 150, 3, 3, 80
M_OBS, PER = 4, 20
SEED = 2
N_CAL = 512
ORACLE_STEP = DTH - 1
# max |cdf_steps[:, ORACLE_STEP] - oracle| measured on this file's fixed seed on an MI355X (profiles/ar_score/parity.json)
# and the bound asserted: twice the measured value, for box-to-box differences in bf16 accumulation order
ORACLE_MEASURED = {"none": 1.570870e-04, "ensemble": 1.321911e-04}
ORACLE_BOUND = {m: 2 * v for m, v in ORACLE_MEASURED.items()}   # 3.141740e-04, 2.643822e-04


def _data():
    rng = np.random.default_rng(21)
    th = rng.normal(size=(N_CTX, DTH)).astype(np.float32)
    x = (np.exp(0.5 * (th @ rng.normal(size=(DTH, DX)))) + 0.1 * rng.normal(size=(N_CTX, DX))).astype(np.float32)
    xq = (x[:N] + 0.05 * rng.normal(size=(N, DX))).astype(np.float32)          # 80 distinct query rows
    tq = rng.normal(size=(N, DTH)).astype(np.float32)
    tq[0] = 40.0                                                             # far tail: the half-normal end bar
    xu = x[N: N + M_OBS].copy()                                              # 4 observations x 20 thetas
    tr = rng.normal(size=(M_OBS * PER, DTH)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, th, xq, tq, xu, tr))


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(CFG, seed=0)


@pytest.fixture(scope="module", params=list(MODES))
def runs(request, weights):
    from npe_pfn.engine import Engine

    mode = request.param
    x, th, xq, tq, xu, tr = _data()
    eng = Engine(CFG, weights, device=torch.device("cuda", 0), random_state=SEED, preprocessing=mode)
    r = {"mode": mode, "eng": eng, "data": (x, th, xq, tq, xu, tr)}
    r["lp"] = eng.ar_log_prob(x, th, xq, tq)
    r["steps"], r["cdf"] = eng.ar_score(x, th, xq, tq)
    r["lp_rep"] = eng.ar_log_prob(x, th, xu.repeat_interleave(PER, 0), tr, x_unique=xu)
    r["steps_rep"], r["cdf_rep"] = eng.ar_score(x, th, xu, tr)
    return r


def _sum_in_order(steps):
    acc = torch.zeros(steps.shape[0], dtype=torch.float32, device=steps.device)
    for k in range(steps.shape[1]):
        acc += steps[:, k]
    return acc


def test_plain_steps_sum_to_ar_log_prob_bit_for_bit(runs):
    assert runs["steps"].shape == (N, DTH) and runs["cdf"].shape == (N, DTH)
    assert runs["steps"].is_cuda and runs["steps"].dtype == torch.float32
    assert torch.isfinite(runs["steps"]).all()
    assert torch.equal(_sum_in_order(runs["steps"]), runs["lp"])


def test_repeated_steps_sum_to_ar_log_prob_repeated_bit_for_bit(runs):
    assert runs["steps_rep"].shape == (M_OBS * PER, DTH)
    assert torch.equal(_sum_in_order(runs["steps_rep"]), runs["lp_rep"])


def test_reproducible_and_chunked_bit_for_bit(runs):
    """The same call twice, one output at a time, and in chunks of 32 query rows (80 rows: 32, 32,
    16): the same bits -- the existing chunk tests allow no difference (the forward is
    batch-invariant)."""
    eng = runs["eng"]
    x, th, xq, tq, xu, tr = runs["data"]
    s2, c2 = eng.ar_score(x, th, xq, tq)
    assert torch.equal(s2, runs["steps"]) and torch.equal(c2, runs["cdf"])
    s3, none = eng.ar_score(x, th, xq, tq, want_cdf=False)
    none2, c3 = eng.ar_score(x, th, xq, tq, want_logp=False)
    assert none is None and none2 is None
    assert torch.equal(s3, runs["steps"]) and torch.equal(c3, runs["cdf"])
    eng.set_chunk_rows(32)
    try:
        s4, c4 = eng.ar_score(x, th, xq, tq)
        s5, c5 = eng.ar_score(x, th, xu, tr)
    finally:
        eng.set_chunk_rows(16384)
    assert torch.equal(s4, runs["steps"]) and torch.equal(c4, runs["cdf"])
    assert torch.equal(s5, runs["steps_rep"]) and torch.equal(c5, runs["cdf_rep"])


def test_fit_reuse_gives_the_same_bits(runs):
    eng = runs["eng"]
    x, th, xq, tq, _, _ = runs["data"]
    eng.set_fit_token(12345)
    try:
        first = eng.ar_score(x, th, xq, tq)
        again = eng.ar_score(x, th, xq, tq)      # reuses every step's fit
    finally:
        eng.set_fit_token(0)
    for got in (first, again):
        assert torch.equal(got[0], runs["steps"]) and torch.equal(got[1], runs["cdf"])


def test_cdf_steps_match_the_unfused_route(runs):
    """fit -> predict_logits -> bar_cdf on get_borders, per step: |d| <= 2e-5 (the unfused route
    rounds log p to fp32 and exponentiates again: with |log p| <= 88 about 5e-6 relative per bar,
    in the numerator and in the total)."""
    eng = runs["eng"]
    x, th, xq, tq, _, _ = runs["data"]
    joint = torch.cat([x, th], 1)
    test = torch.cat([xq, tq], 1)
    for k in range(DTH):
        eng.fit(joint[:, : DX + k], joint[:, DX + k])
        ref = eng.bar_cdf(eng.predict_logits(test[:, : DX + k]), eng.borders(), tq[:, k])
        d = (runs["cdf"][:, k] - ref).abs().max().item()
        print(f"{runs['mode']} step {k}: max |fused - unfused| = {d:.3e}")
        assert d <= 2e-5, (k, d)
    assert runs["cdf"][0, 0].item() > 0.999   # theta = 40: the right tail


def test_cdf_steps_near_the_oracle(runs, weights):
    """Anchor against OracleTabPFN(emulate_bf16=True) mixtures through the fp64 restatement
    (tests/bar_cdf_ref.py), at the last step (k = 2: the widest table, both teacher-forced theta
    columns among its features).  The oracle's fit is what this test costs, so the earlier steps
    are not refitted here: test_cdf_steps_match_the_unfused_route pins every step to the engine's
    own fit -> predict route, which the oracle tests of the forward anchor.  Measured on this
    file's fixed seed on an MI355X over the 80 rows: max |d| = 1.570870e-04 ("none") and
    1.321911e-04 ("ensemble") (ORACLE_MEASURED above, profiles/ar_score/parity.json).  The bound is
    twice that, 3.141740e-04 and 2.643822e-04: the margin covers box-to-box differences in bf16
    accumulation order."""
    mode = runs["mode"]
    x, th, xq, tq, _, _ = (a.numpy() for a in runs["data"])
    orc = OracleTabPFN(weights, CFG.n_estimators, CFG.softmax_temperature, seed=SEED, emulate_bf16=True,
                       preprocessing=MODES[mode])
    joint = np.concatenate([x, th], 1)
    test = np.concatenate([xq, tq], 1)
    got = runs["cdf"].cpu().numpy().astype(np.float64)
    k = ORACLE_STEP
    orc.fit(joint[:, : DX + k], joint[:, DX + k])
    ref = cdf_from_probs(orc.predict_probs(test[:, : DX + k]), orc.borders(), tq[:, k])
    worst = float(np.abs(got[:, k] - ref).max())
    print(f"{mode}: max |cdf_steps - oracle| = {worst:.6e} (bound {ORACLE_BOUND[mode]})")
    assert worst <= ORACLE_BOUND[mode], (worst, ORACLE_BOUND[mode])


def test_self_calibration(runs):
    """512 draws of ar_sample for one observation, scored by ar_score on the same engine and
    context: the PIT values of the engine's own samples are uniform -- KS distance of every
    dimension <= 1.95 / sqrt(512), the critical value at alpha = 0.001 (fixed seeds: deterministic)."""
    eng = runs["eng"]
    x, th, _, _, xu, _ = runs["data"]
    obs = xu[:1]
    draws, _ = eng.ar_sample(x, th, obs.repeat(N_CAL, 1), counter=0, x_unique=obs)
    _, pit = eng.ar_score(x, th, obs, draws, want_logp=False)
    ks = pit_ks_statistic(pit.cpu())
    print(f"{runs['mode']}: KS per dimension = {ks.tolist()} (critical {1.95 / np.sqrt(N_CAL):.4f})")
    assert ks.shape == (DTH,)
    assert float(ks.max()) <= 1.95 / np.sqrt(N_CAL), ks


def test_errors(runs):
    from npe_pfn.engine import _ptr

    eng = runs["eng"]
    x, th, xq, tq, xu, tr = runs["data"]
    with pytest.raises(ValueError):
        eng.ar_score(x, th, xq, tq, want_logp=False, want_cdf=False)
    with pytest.raises(ValueError):
        eng.ar_score(x, th, xu[:3], tr)                      # 3 does not divide 80
    with pytest.raises(ValueError):
        eng.ar_score(x, th, xq, tq[:, :2])
    dev = [a.cuda().contiguous() for a in (x, th, xu, tr)]
    out = torch.empty((M_OBS * PER, DTH), device="cuda")
    lib, h, s = eng.lib, eng.h, eng.stream
    args = (h, _ptr(dev[0]), _ptr(dev[1]), N_CTX, DX, DTH, _ptr(dev[2]))
    assert lib.npfn_ar_score(*args, 3, _ptr(dev[3]), M_OBS * PER, _ptr(out), None, 1e-15, s) == -1   # 3 does not divide 80
    assert lib.npfn_ar_score(*args, 0, _ptr(dev[3]), M_OBS * PER, _ptr(out), None, 1e-15, s) == -1   # n_unique < 1
    assert lib.npfn_ar_score(*args, M_OBS, _ptr(dev[3]), M_OBS * PER, None, None, 1e-15, s) == -1    # both outputs NULL
    assert lib.npfn_ar_score(*args, M_OBS, None, M_OBS * PER, _ptr(out), None, 1e-15, s) == -1        # no theta
    assert lib.npfn_ar_score(h, _ptr(dev[0]), _ptr(dev[1]), N_CTX, 0, DTH, _ptr(dev[2]), M_OBS, _ptr(dev[3]),
                             M_OBS * PER, _ptr(out), None, 1e-15, s) == -1                            # dim_x < 1
    eng.set_estimator_range(0, CFG.n_estimators // 2)
    try:
        assert lib.npfn_ar_score(*args, M_OBS, _ptr(dev[3]), M_OBS * PER, _ptr(out), None, 1e-15, s) == -3   # NPFN_ESTATE
    finally:
        eng.set_estimator_range(0, CFG.n_estimators)
    # the engine is still usable, and gives the same bits
    s2, _ = eng.ar_score(x, th, xu, tr, want_cdf=False)
    assert torch.equal(s2, runs["steps_rep"])
