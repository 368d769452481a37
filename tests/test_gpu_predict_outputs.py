"""GPU: TabPFNRegressor.predict's summary outputs (npfn_predict_stats).

The smallest shape of test_predict_matches_oracle (64 context rows, 3 features, 40 query rows) on
the default model, under preprocessing "none", "ensemble" (translated target borders) and
average_before_softmax; and a small-head model (250 bars: the generic mix path).  Tolerances:
bar_stats_ref.check_*.  npfn_predict_stats summarises windows of rows inside the engine;
predict_logits + bar_stats is the same arithmetic on the whole [N, n_bars] logits.
"""
import numpy as np
import pytest
import torch

from bar_stats_ref import check_mean, check_mode, check_quantiles, ref_cdf
from npe_pfn.weights import ModelConfig, synthetic_weights
from oracle.tabpfn_oracle import OracleTabPFN

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
# tabpfn's default levels.  q = 0 and 1 are left to test_gpu_bar_stats.py: a position error is the
# CDF error over the density, and a fitted predictive distribution's density vanishes at its ends
# (the oracle's own answer there hinges on whether its fp32 softmax sums to 1), so a tolerance
# on the position says nothing there.
QS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
VARIANTS = {"none": dict(preprocessing="none"), "ensemble": dict(preprocessing="ensemble"),
            "avg_before_softmax": dict(preprocessing="ensemble", average_before_softmax=True)}


def _data(n=64, F=3, N=40, seed=67):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    y = (X @ rng.normal(size=F) + 0.3 * rng.normal(size=n)).astype(np.float32)
    Xq = rng.normal(size=(N, F)).astype(np.float32)
    return X, y, Xq


@pytest.fixture(scope="module")
def weights():
    return synthetic_weights(CFG, seed=0)


@pytest.fixture(scope="module")
def fitted(weights):
    """{variant: (regressor, Xq, predict_stats as numpy, predict_logits, borders)}, computed once."""
    from npe_pfn.tabpfn import TabPFNRegressor

    X, y, Xq = _data()
    out = {}
    for name, kw in VARIANTS.items():
        reg = TabPFNRegressor(weights=weights, random_state=3, device="cuda:0", **kw)
        reg.fit(torch.from_numpy(X), torch.from_numpy(y))
        eng = reg.engine
        xq = torch.from_numpy(Xq).cuda()
        st = {k: v.cpu().numpy() for k, v in eng.predict_stats(xq, QS).items()}
        out[name] = (reg, xq, st, eng.predict_logits(xq), eng.borders())
    return out


def _check_against_logits(eng, st, logits, borders, what):
    lg, b = logits.cpu().numpy(), borders.cpu().numpy()
    check_quantiles(st["quantiles"], lg, b, QS, what=what)
    check_mean(st["mean"], lg, b, what=what)
    check_mode(st["mode"], lg, b, what=what)
    # and against the unfused device path: each within the tolerance of the reference, so within
    # the same bounds of each other (the mode by density, as near-ties may resolve either way)
    un = {k: v.cpu().numpy() for k, v in eng.bar_stats(logits, borders, QS).items()}
    span = float(b[-1]) - float(b[0])
    assert np.abs(st["quantiles"].astype(np.float64) - un["quantiles"]).max() <= 1e-4 * span, what
    assert (np.abs(st["mean"].astype(np.float64) - un["mean"])
            <= 2e-5 * span + 4 * np.spacing(np.abs(un["mean"])).astype(np.float64)).all(), what
    check_mode(un["mode"], lg, b, what=what + " unfused")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_stats_equal_stats_of_the_logits(fitted, variant):
    reg, xq, st, logits, borders = fitted[variant]
    _check_against_logits(reg.engine, st, logits, borders, variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_chunked_rows_give_the_same_bits(fitted, variant):
    reg, xq, st, _, _ = fitted[variant]
    eng = reg.engine
    eng.set_chunk_rows(16)   # 40 rows: chunks of 16, 16, 8
    try:
        ch = {k: v.cpu().numpy() for k, v in eng.predict_stats(xq, QS).items()}
    finally:
        eng.set_chunk_rows(16384)
    for k in ("mean", "mode", "quantiles"):
        assert np.array_equal(ch[k], st[k]), (variant, k)


def test_row_windows_give_the_same_bits(fitted):
    """npfn_predict_stats summarises 8192 rows at a time: with the 40 query rows behind 8192 others
    they fall into the second window of one forward chunk.  The forward is batch-invariant, so
    their results are those of the 40-row call bit for bit."""
    reg, xq, st, _, _ = fitted["none"]
    big = torch.cat([xq.repeat(205, 1)[:8192], xq])
    out = {k: v.cpu().numpy() for k, v in reg.engine.predict_stats(big, QS).items()}
    assert out["quantiles"].shape == (len(QS), big.shape[0])
    for k in ("mean", "mode"):
        assert np.array_equal(out[k][8192:], st[k]) and np.array_equal(out[k][:40], st[k]), k
    assert np.array_equal(out["quantiles"][:, 8192:], st["quantiles"])
    assert np.array_equal(out["quantiles"][:, :40], st["quantiles"])


def test_quantiles_against_the_cpu_oracle(fitted, weights):
    """A CDF gap is bounded by the total variation, 0.02 for this pair (test_predict_matches_oracle);
    1e-4 on top for the quantile's own tolerance."""
    reg, xq, st, _, _ = fitted["none"]
    X, y, Xq = _data()
    orc = OracleTabPFN(weights, CFG.n_estimators, CFG.softmax_temperature, seed=3, emulate_bf16=True)
    orc.fit(X, y)
    lg_ref = np.log(np.maximum(orc.predict_probs(Xq), 1e-38)).astype(np.float32)
    for i, q in enumerate(QS):
        gap = np.abs(ref_cdf(lg_ref, orc.borders(), st["quantiles"][i]) - q)
        print(f"q={q}: max |cdf_oracle(x) - q| = {gap.max():.4f}")
        assert gap.max() <= 0.02 + 1e-4, (q, gap.max())


def test_predict_surface(fitted):
    reg, xq, st, logits, borders = fitted["none"]
    Xq = xq.cpu().numpy()
    N = Xq.shape[0]
    for ot in ("mean", "median", "mode"):
        v = reg.predict(Xq, output_type=ot)
        assert isinstance(v, np.ndarray) and v.shape == (N,) and v.dtype == np.float32
        t = reg.predict_tensor(Xq, output_type=ot)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), v)
    assert np.array_equal(reg.predict(Xq, output_type="mean"), st["mean"])
    assert np.array_equal(reg.predict(Xq, output_type="mode"), st["mode"])
    median = reg.predict(Xq, output_type="median")
    assert np.array_equal(median, st["quantiles"][QS.index(0.5)])
    qs = reg.predict(Xq, output_type="quantiles", quantiles=[0.25, 0.75])
    assert isinstance(qs, list) and len(qs) == 2 and all(a.shape == (N,) and a.dtype == np.float32 for a in qs)
    assert (qs[0] <= median).all() and (median <= qs[1]).all()
    deciles = reg.predict(Xq, output_type="quantiles")
    assert len(deciles) == 9 and all(np.array_equal(a, st["quantiles"][i]) for i, a in enumerate(deciles))
    main = reg.predict(Xq, output_type="main")
    assert set(main) == {"mean", "median", "mode", "quantiles"} and len(main["quantiles"]) == 9
    assert np.array_equal(main["median"], median) and np.array_equal(main["mean"], st["mean"])
    assert np.array_equal(main["mode"], st["mode"])
    tmain = reg.predict_tensor(Xq, output_type="main")
    assert tmain["mean"].is_cuda and tmain["median"].is_cuda and all(t.is_cuda for t in tmain["quantiles"])


def test_full_output_is_unchanged(fitted):
    reg, xq, st, logits, borders = fitted["none"]
    for out in (reg.predict(xq), reg.predict(xq, output_type="full", quantiles=[])):
        assert set(out) == {"logits", "criterion"}
        assert out["logits"].is_cuda and torch.equal(out["logits"], logits)
        assert torch.equal(out["criterion"].borders, borders)


def test_criterion_summaries_agree_with_predict(fitted):
    """BarCriterion.mean / median / mode / icdf on the predicted logits against predict_tensor: the
    fused-vs-unfused tolerances."""
    reg, xq, st, logits, borders = fitted["none"]
    crit = reg.predict(xq)["criterion"]
    span = float(borders[-1] - borders[0])
    got = {"mean": crit.mean(logits), "median": crit.median(logits), "mode": crit.mode(logits),
           "icdf": crit.icdf(logits, [0.1, 0.9]), "icdf1": crit.icdf(logits, 0.3)}
    assert all(v.is_cuda for v in got.values())   # on the logits' device
    assert got["icdf"].shape == (2, logits.shape[0]) and got["icdf1"].shape == (logits.shape[0],)
    mean = reg.predict_tensor(xq, "mean")
    assert ((got["mean"] - mean).abs().double() <= 2e-5 * span + 4 * torch.from_numpy(
        np.spacing(np.abs(mean.cpu().numpy()))).cuda().double()).all()
    assert (got["median"] - reg.predict_tensor(xq, "median")).abs().max().item() <= 1e-4 * span
    q = reg.predict_tensor(xq, "quantiles", quantiles=[0.1, 0.3, 0.9])
    assert (got["icdf"][0] - q[0]).abs().max().item() <= 1e-4 * span
    assert (got["icdf1"] - q[1]).abs().max().item() <= 1e-4 * span
    assert (got["icdf"][1] - q[2]).abs().max().item() <= 1e-4 * span
    check_mode(got["mode"].cpu().numpy(), logits.cpu().numpy(), borders.cpu().numpy(), what="criterion")
    cpu = crit.mean(logits.cpu())
    assert not cpu.is_cuda and torch.equal(cpu, got["mean"].cpu())


def test_small_head_generic_mix_path():
    """250 bars are no multiple of 4: the generic mix path under npfn_predict_stats."""
    from npe_pfn.engine import Engine

    cfg = ModelConfig(n_layers=2, n_bars=250, max_groups=16)
    eng = Engine(cfg, synthetic_weights(cfg, seed=0), device=torch.device("cuda", 0), random_state=3)
    X, y, Xq = _data()
    eng.fit(torch.from_numpy(X), torch.from_numpy(y))
    xq = torch.from_numpy(Xq).cuda()
    st = {k: v.cpu().numpy() for k, v in eng.predict_stats(xq, QS).items()}
    _check_against_logits(eng, st, eng.predict_logits(xq), eng.borders(), "250 bars")
