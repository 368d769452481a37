"""GPU: npfn_bar_cdf (criterion.cdf) against the fp64 restatement tests/bar_cdf_ref.py.

Logits 3 N(0, 1), borders 3 sort(N(0, 1)); 2, 3, 257 (no multiple of 4, more bars than threads) and
5000 bars; 1 and 5 rows, of the 5 one with -inf in a third of its bars and one all -inf.  Every row
is scored at 13 targets: below b[0], at b[0], inside the left tail bar, at b[1], at a bar midpoint,
exactly on an inner border, at b[n_bars-1], inside the right tail bar, at b[n_bars], beyond it,
-inf, +inf and NaN.

Tolerance |d| <= 2e-6: fp32 exp plus a two-sided block sum of at most 5000 terms, and the result
itself is fp32.
"""
import ctypes

import numpy as np
import pytest
import torch

from bar_cdf_ref import bar_cdf_ref
from npe_pfn.weights import ModelConfig, synthetic_weights
from oracle.philox import uniforms

pytestmark = pytest.mark.gpu

CFG = ModelConfig()
SIZES = (2, 3, 257, 5000)
ROWS = (1, 5)
TOL = 2e-6
N_Y = 13
Y_RIGHT = (6, 7, 8, 9)     # at b[nb-1], inside the right tail bar, at b[nb], beyond it
Y_NEG_INF, Y_POS_INF, Y_NAN = 10, 11, 12
ROW_HOLES, ROW_EMPTY = 1, 4


@pytest.fixture(scope="module")
def engine():
    from npe_pfn.engine import Engine

    return Engine(CFG, synthetic_weights(CFG, seed=0), device=torch.device("cuda", 0), random_state=3,
                  preprocessing="none")


def _inputs(nb, rows):
    rng = np.random.default_rng(7 + nb)
    logits = (3.0 * rng.normal(size=(rows, nb))).astype(np.float32)
    borders = (np.sort(rng.normal(size=nb + 1)) * 3).astype(np.float32)
    if rows > 1:
        logits[ROW_HOLES, rng.permutation(nb)[: max(nb // 3, 1)]] = -np.inf
        logits[ROW_EMPTY] = -np.inf
    b = borders.astype(np.float64)
    m = nb // 2
    ys = np.array([b[0] - 0.37 * (b[1] - b[0]) - 0.1, b[0], b[0] + 0.4 * (b[1] - b[0]), b[1], 0.5 * (b[m] + b[m + 1]),
                   b[max(m, 1)], b[nb - 1], b[nb - 1] + 0.3 * (b[nb] - b[nb - 1]), b[nb],
                   b[nb] + 0.45 * (b[nb] - b[nb - 1]) + 0.1, -np.inf, np.inf, np.nan]).astype(np.float32)
    assert ys.shape == (N_Y,)
    return np.repeat(logits, N_Y, 0), borders, np.tile(ys, rows)   # row r at target t: index r * N_Y + t


@pytest.fixture(scope="module")
def cases(engine):
    """{(n_bars, rows): (device result [rows, N_Y], fp64 restatement)}: computed once."""
    out = {}
    for nb in SIZES:
        for rows in ROWS:
            logits, borders, ys = _inputs(nb, rows)
            got = engine.bar_cdf(torch.from_numpy(logits).cuda(), torch.from_numpy(borders).cuda(),
                                 torch.from_numpy(ys).cuda())
            assert got.is_cuda and got.dtype == torch.float32 and got.shape == (rows * N_Y,)
            out[nb, rows] = (got.cpu().numpy().reshape(rows, N_Y), bar_cdf_ref(logits, borders, ys).reshape(rows, N_Y))
    return out


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nb", SIZES)
def test_matches_the_restatement(cases, nb, rows):
    got, ref = cases[nb, rows]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    d = np.abs(got.astype(np.float64) - ref)[ok]
    print(f"nb={nb} rows={rows}: max |gpu - fp64| = {d.max():.3e}")
    assert d.max() <= TOL, d.max()
    assert (got[ok] >= 0).all() and (got[ok] <= 1).all()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nb", SIZES)
def test_upper_tail_keeps_its_complement(cases, nb, rows):
    """1 - F at the right-tail targets: the mass is summed from both sides and F formed from the
    smaller one, so the complement is not what rounding leaves of 1 - (a long sum from the left)."""
    got, ref = cases[nb, rows]
    for r in range(rows):
        if rows > 1 and r == ROW_EMPTY:
            continue
        for t in Y_RIGHT:
            d = abs((1.0 - np.float64(got[r, t])) - (1.0 - ref[r, t]))
            assert d <= TOL, (nb, r, t, d)


@pytest.mark.parametrize("nb", SIZES)
def test_nan_and_infinite_targets(cases, nb):
    got, _ = cases[nb, 5]
    assert np.isnan(got[ROW_EMPTY]).all()                       # no finite logit: NaN at every target
    live = [r for r in range(5) if r != ROW_EMPTY]
    assert np.isnan(got[live, Y_NAN]).all()
    assert (got[live, Y_NEG_INF] == 0.0).all() and (got[live, Y_POS_INF] == 1.0).all()
    assert not np.isnan(got[live][:, :Y_NAN]).any()


def test_errors_and_empty_call(engine):
    from npe_pfn.engine import EngineError, load_library

    lib = load_library()
    buf = torch.zeros(8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.npfn_bar_cdf(p, p, p, 1, 1, p, engine.stream) == -1         # n_bars < 2
    assert lib.npfn_bar_cdf(p, p, p, -1, 2, p, engine.stream) == -1        # n_rows < 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.npfn_bar_cdf(args[0], args[1], args[2], 1, 2, args[3], engine.stream) == -1
    assert lib.npfn_bar_cdf(None, None, None, 0, 2, None, engine.stream) == 0   # nothing to do
    out = engine.bar_cdf(torch.zeros((0, 4)), torch.arange(5.0), torch.zeros(0))
    assert out.shape == (0,)
    with pytest.raises(EngineError):
        engine.bar_cdf(torch.zeros((2, 1)), torch.arange(2.0), torch.zeros(2))
    with pytest.raises(ValueError):
        engine.bar_cdf(torch.zeros((2, 4)), torch.arange(4.0), torch.zeros(2))


@pytest.mark.parametrize("nb", (257, 5000))
def test_round_trip_through_bar_sample(engine, nb):
    """cdf(sample(u)) == u on the inner bars (the two tail bars get -inf logits, so every draw
    lands in an inner bar): within n_bars * 2^-24, the worst-case error of an fp32 prefix sum.

    The borders are evenly spaced on [-3, 3].  The draw itself is an fp32 number, and rounding it
    moves its CDF by (p_j / w_j) ulp(y) / 2, which no kernel can undo: at most (n_bars / 6) 2^-23
    = n_bars 2^-25.6 here, a third of the bound even for a bar that holds all the mass.  With the
    random borders of the tests above one narrow bar makes that term alone exceed the bound (257
    bars: p_j = 0.39 in a bar 1.3e-3 wide at y = 1.57 gives 1.8e-5, from an fp64 sampler as
    well), and the test would measure the number format instead of the prefix sums."""
    n, counter = 300, 5
    rng = np.random.default_rng(nb)
    logits = (3.0 * rng.normal(size=(n, nb))).astype(np.float32)
    logits[:, 0] = -np.inf
    logits[:, -1] = -np.inf
    borders = np.linspace(-3.0, 3.0, nb + 1).astype(np.float32)
    lg, bd = torch.from_numpy(logits).cuda(), torch.from_numpy(borders).cuda()
    draws = engine.bar_sample(lg, bd, counter)
    assert bool(((draws >= bd[1]) & (draws <= bd[nb - 1])).all())
    back = engine.bar_cdf(lg, bd, draws).cpu().numpy().astype(np.float64)
    u = uniforms(engine.random_state, counter, n).astype(np.float64)
    d = np.abs(back - u).max()
    print(f"nb={nb}: max |cdf(sample(u)) - u| = {d:.3e} (bound {nb * 2.0 ** -24:.3e})")
    assert d <= nb * 2.0 ** -24, d


def test_criterion_cdf_returns_on_the_device_of_y(engine):
    from npe_pfn.tabpfn import BarCriterion, TabPFNRegressor

    reg = TabPFNRegressor(random_state=3, preprocessing="none")
    reg._engine = engine
    logits, borders, ys = _inputs(257, 1)
    crit = BarCriterion(reg, torch.from_numpy(borders).cuda())
    on_cpu = crit.cdf(torch.from_numpy(logits).cuda(), torch.from_numpy(ys))
    on_gpu = crit.cdf(torch.from_numpy(logits), torch.from_numpy(ys).cuda())
    assert not on_cpu.is_cuda and on_gpu.is_cuda
    assert torch.equal(torch.isnan(on_cpu), torch.isnan(on_gpu.cpu()))
    ok = ~torch.isnan(on_cpu)
    assert torch.equal(on_cpu[ok], on_gpu.cpu()[ok])
