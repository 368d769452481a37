"""GPU: npfn_bar_stats (criterion.mean / .median / .mode / .icdf) against tests/bar_stats_ref.py.

Inputs are the construction of test_bar_sample_and_nll_match_oracle (logits 2 N(0, 1), borders
3 sort(N(0, 1))): 64 rows at 5000 bars plus five special rows, and 64 rows at 2 bars (both
tails), 64 (fewer bars than threads), 250 (no multiple of 4) and 1024.  The tolerances and their
derivations are in bar_stats_ref.check_*.  No row here is all -inf or NaN.
"""
import ctypes

import numpy as np
import pytest
import torch

from bar_stats_ref import check_mean, check_mode, check_quantiles
from npe_pfn.weights import ModelConfig, synthetic_weights
from oracle.philox import uniforms

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
QS = (0.0, 1e-6, 0.1, 0.5, 0.9, 1 - 1e-6, 1.0)
SIZES = (5000, 2, 64, 250, 1024)
R = 64
# the special rows appended at 5000 bars
ROW_FIRST, ROW_LAST, ROW_UPPER, ROW_ONEHOT, ROW_EQUAL = R, R + 1, R + 2, R + 3, R + 4
ONEHOT_BAR, UPPER_FROM = 1234, 4000


@pytest.fixture(scope="module")
def engine():
    from npe_pfn.engine import Engine

    return Engine(CFG, synthetic_weights(CFG, seed=0), device=torch.device("cuda", 0), random_state=3,
                  preprocessing="none")


def _inputs(nb):
    rng = np.random.default_rng(1)
    logits = (rng.normal(size=(R, nb)) * 2).astype(np.float32)
    borders = np.sort(rng.normal(size=nb + 1)).astype(np.float32) * 3
    if nb == 5000:
        sp = np.full((5, nb), -np.inf, np.float32)
        sp[0, 0] = 0.3
        sp[1, -1] = -1.0
        sp[2, UPPER_FROM:] = (rng.normal(size=nb - UPPER_FROM) * 2).astype(np.float32)
        sp[3, ONEHOT_BAR] = 2.0
        sp[4, :] = 0.5
        logits = np.concatenate([logits, sp])
    return logits, borders


@pytest.fixture(scope="module")
def cases(engine):
    """{n_bars: (logits, borders, device results as numpy)}: computed once, read by every test."""
    out = {}
    for nb in SIZES:
        logits, borders = _inputs(nb)
        st = engine.bar_stats(torch.from_numpy(logits).cuda(), torch.from_numpy(borders).cuda(), QS)
        assert set(st) == {"mean", "mode", "quantiles"} and all(v.is_cuda for v in st.values())
        out[nb] = (logits, borders, {k: v.cpu().numpy() for k, v in st.items()})
    return out


@pytest.mark.parametrize("nb", SIZES)
def test_quantiles_match_oracle_icdf(cases, nb):
    logits, borders, st = cases[nb]
    check_quantiles(st["quantiles"], logits, borders, QS, what=f"nb={nb}")


def test_quantiles_never_land_in_a_zero_mass_bar(cases):
    logits, borders, st = cases[5000]
    x = st["quantiles"]
    assert (x[:, ROW_FIRST] >= borders[0]).all() and (x[:, ROW_FIRST] <= borders[1]).all()
    assert (x[:, ROW_LAST] >= borders[-2]).all() and (x[:, ROW_LAST] <= borders[-1]).all()
    assert (x[:, ROW_UPPER] >= borders[UPPER_FROM]).all()
    assert (x[:, ROW_ONEHOT] >= borders[ONEHOT_BAR]).all() and (x[:, ROW_ONEHOT] <= borders[ONEHOT_BAR + 1]).all()
    # q = 0 / 1: the left / right border of the first / last bar with mass
    assert x[0, ROW_UPPER] == borders[UPPER_FROM] and x[0, ROW_ONEHOT] == borders[ONEHOT_BAR]
    assert x[-1, ROW_ONEHOT] == borders[ONEHOT_BAR + 1] and x[-1, ROW_FIRST] == borders[1]


@pytest.mark.parametrize("nb", SIZES)
def test_mean_matches_reference(cases, nb):
    logits, borders, st = cases[nb]
    check_mean(st["mean"], logits, borders, what=f"nb={nb}")


@pytest.mark.parametrize("nb", SIZES)
def test_mode_is_the_densest_bar(cases, nb):
    logits, borders, st = cases[nb]
    j = check_mode(st["mode"], logits, borders, what=f"nb={nb}")
    if nb == 5000:
        w = np.diff(borders.astype(np.float64))
        assert j[ROW_EQUAL] == int(np.where(w > 0, w, np.inf).argmin())   # equal mass: the narrowest bar
        assert j[ROW_FIRST] == 0 and j[ROW_LAST] == nb - 1 and j[ROW_ONEHOT] == ONEHOT_BAR


def test_quantile_at_a_draws_uniform_is_the_draw(engine, cases):
    """icdf(u_i) of row i is bar_sample's draw of row i at that uniform: the same arithmetic, only
    FMA contraction may differ between the two kernels (1e-6 of the span)."""
    logits, borders, _ = cases[5000]
    counter = 9
    lt, bt = torch.from_numpy(logits[:8]).cuda(), torch.from_numpy(borders).cuda()
    u = uniforms(engine.random_state, counter, 8)
    draws = engine.bar_sample(lt, bt, counter=counter).cpu().numpy()
    x = engine.bar_stats(lt, bt, [float(v) for v in u], mean=False, mode=False)["quantiles"].cpu().numpy()
    mine = np.diagonal(x)   # level i on row i
    span = float(borders[-1]) - float(borders[0])
    print("max |icdf(u) - draw| =", np.abs(mine - draws).max(), "bound", 1e-6 * span)
    assert np.abs(mine.astype(np.float64) - draws.astype(np.float64)).max() <= 1e-6 * span


def test_each_statistic_alone_gives_the_same_values(engine, cases):
    logits, borders, st = cases[250]
    lt, bt = torch.from_numpy(logits).cuda(), torch.from_numpy(borders).cuda()
    only_mean = engine.bar_stats(lt, bt, (), mean=True, mode=False)
    only_mode = engine.bar_stats(lt, bt, (), mean=False, mode=True)
    only_q = engine.bar_stats(lt, bt, QS, mean=False, mode=False)
    assert set(only_mean) == {"mean"} and set(only_mode) == {"mode"} and set(only_q) == {"quantiles"}
    assert np.array_equal(only_mean["mean"].cpu().numpy(), st["mean"])
    assert np.array_equal(only_mode["mode"].cpu().numpy(), st["mode"])
    assert np.array_equal(only_q["quantiles"].cpu().numpy(), st["quantiles"])
    assert engine.bar_stats(lt, bt, (), mean=False, mode=False) == {}


def test_no_rows_and_bad_arguments(engine, cases):
    logits, borders, _ = cases[64]
    lt, bt = torch.from_numpy(logits).cuda(), torch.from_numpy(borders).cuda()
    st = engine.bar_stats(lt[:0], bt, QS)
    assert st["mean"].shape == (0,) and st["mode"].shape == (0,) and st["quantiles"].shape == (len(QS), 0)
    lib, vp = engine.lib, ctypes.c_void_p
    q = torch.tensor(QS, dtype=torch.float32, device="cuda")
    out = torch.empty(len(QS) * R, dtype=torch.float32, device="cuda")
    args = (vp(lt.data_ptr()), vp(bt.data_ptr()))
    assert lib.npfn_bar_stats(*args, 0, 64, vp(q.data_ptr()), len(QS), None, None, vp(out.data_ptr()), engine.stream) == 0
    for n_bars, n_q in ((1, 1), (64, -1), (64, 65)):
        assert lib.npfn_bar_stats(*args, R, n_bars, vp(q.data_ptr()), n_q, None, None, vp(out.data_ptr()),
                                  engine.stream) != 0
    assert lib.npfn_bar_stats(*args, R, 64, None, 1, None, None, vp(out.data_ptr()), engine.stream) != 0
    assert lib.npfn_bar_stats(*args, R, 64, vp(q.data_ptr()), 1, None, None, None, engine.stream) != 0
    with pytest.raises(ValueError):
        engine.bar_stats(lt, bt, [1.5])
    torch.cuda.synchronize()
