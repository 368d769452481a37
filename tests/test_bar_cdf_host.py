"""The bar CDF's closed form (include/npfn.h npfn_bar_cdf) on the CPU in fp64: the numpy
restatement tests/bar_cdf_ref.py against the NLL's density (oracle.tabpfn_oracle.bar_nll), and the
package's torch function npe_pfn.bar_cdf against the restatement.  Also pit_ks_statistic against
scipy (a test-only dependency)."""
import numpy as np
import pytest
import torch

from bar_cdf_ref import bar_cdf_ref, bucket64, softmax64
from oracle.tabpfn_oracle import bar_bucket, bar_nll

N_BARS = [2, 3, 64]


def _case(nb, seed=0):
    """One row of logits and uneven fp32 borders (every value fp32-representable)."""
    rng = np.random.default_rng(100 + nb + seed)
    logits = (2.0 * rng.normal(size=(1, nb))).astype(np.float32)
    widths = (0.05 + rng.random(nb)).astype(np.float32)
    borders = (np.float32(-1.5) + np.concatenate([[0.0], np.cumsum(widths)])).astype(np.float32)
    return logits, borders


def _cdf(logits, borders, y):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return bar_cdf_ref(np.repeat(logits, y.shape[0], 0), borders, y)


@pytest.mark.parametrize("nb", N_BARS)
def test_bar_masses_and_limits(nb):
    """Between its two borders an inner bar holds exactly p_j.  A tail bar is a half-normal whose
    median lies on the outer border: p_j / 2 lies between its borders (F(b[0]) = p_0 / 2), the
    other half beyond, and all of p_j between the inner border and infinity."""
    logits, borders = _case(nb)
    p = softmax64(logits)[0]
    F = _cdf(logits, borders, borders)
    for j in range(nb):
        want = p[j] if 0 < j < nb - 1 else p[j] / 2
        assert abs((F[j + 1] - F[j]) - want) <= 1e-12, (j, F[j + 1] - F[j], want)
    assert abs(F[0] - p[0] / 2) <= 1e-15
    lo, hi = _cdf(logits, borders, [-np.inf, np.inf])
    assert lo == 0.0 and hi == 1.0
    assert abs((F[1] - lo) - p[0]) <= 1e-12 and abs((hi - F[nb - 1]) - p[nb - 1]) <= 1e-12
    far = _cdf(logits, borders, [borders[0] - 1e6, borders[-1] + 1e6])
    assert far[0] == 0.0 and far[1] == 1.0


@pytest.mark.parametrize("nb", N_BARS)
def test_monotone_on_a_sorted_grid(nb):
    logits, borders = _case(nb)
    span = float(borders[-1] - borders[0])
    grid = np.sort(np.concatenate([np.linspace(borders[0] - 2 * span, borders[-1] + 2 * span, 4001),
                                   borders.astype(np.float64)]))
    F = _cdf(logits, borders, grid)
    assert np.all(np.diff(F) >= -1e-15)
    assert F.min() >= 0.0 and F.max() <= 1.0


@pytest.mark.parametrize("nb", N_BARS)
def test_derivative_is_the_nll_density(nb):
    """Central difference of the CDF == exp(-bar_nll) at the midpoint of every bar, at points inside
    both tail bars and at 4 widths beyond each end: relative 1e-5 with a step of 1e-4 of the bar
    width (the density is constant inside an inner bar and smooth in a tail)."""
    logits, borders = _case(nb)
    b = borders.astype(np.float64)
    w = np.diff(b)
    pts = [(0.5 * (b[j] + b[j + 1]), w[j]) for j in range(nb)]
    pts += [(b[0] + 0.25 * w[0], w[0]), (b[0] + 0.8 * w[0], w[0]),
            (b[nb - 1] + 0.2 * w[-1], w[-1]), (b[nb - 1] + 0.75 * w[-1], w[-1]),
            (b[0] - 4 * w[0], w[0]), (b[-1] + 4 * w[-1], w[-1])]
    for y, width in pts:
        y = float(np.float32(y))   # bar_nll reads y as fp32
        h = 1e-4 * width
        lo, hi = _cdf(logits, borders, [y - h, y + h])
        dens = float(np.exp(-np.float64(bar_nll(logits, borders, np.array([y], dtype=np.float32))[0])))
        assert abs((hi - lo) / (2 * h) - dens) <= 1e-5 * dens, (nb, y, (hi - lo) / (2 * h), dens)


def _edge_ys(borders):
    b = borders.astype(np.float64)
    nb = b.shape[0] - 1
    return np.concatenate([b, 0.5 * (b[:-1] + b[1:]), [b[0] - 0.3, b[0] - 7.0, b[-1] + 0.3, b[-1] + 7.0,
                                                         b[0] + 0.3 * (b[1] - b[0]), b[nb - 1] + 0.6 * (b[-1] - b[nb - 1]),
                                                         -np.inf, np.inf, np.nan]])


@pytest.mark.parametrize("nb", N_BARS)
def test_package_bar_cdf_equals_the_restatement(nb):
    import npe_pfn

    logits, borders = _case(nb, seed=1)
    ys = _edge_ys(borders)
    lg = np.repeat(logits, ys.shape[0], 0)
    lg[3, max(nb // 3, 1):] = -np.inf    # a row with bars of no mass
    lg = np.concatenate([lg, np.full((1, nb), -np.inf, dtype=np.float32)])   # and one without a finite logit
    ys = np.concatenate([ys, [0.0]])
    ref = bar_cdf_ref(lg, borders, ys)
    got = npe_pfn.bar_cdf(torch.from_numpy(lg), torch.from_numpy(borders), torch.from_numpy(ys))
    assert got.dtype == torch.float64 and got.shape == (ys.shape[0],)
    got = got.numpy()
    assert np.isnan(ref[-1]) and np.isnan(ref[-2]) and ref[-3] == 1.0 and ref[-4] == 0.0
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-12
    # numpy borders (the oracle criterion's) and a float32 y are taken as they are
    got32 = npe_pfn.bar_cdf(lg[:5], borders, ys[:5].astype(np.float32)).numpy()
    assert np.abs(got32 - bar_cdf_ref(lg[:5], borders, ys[:5].astype(np.float32))).max() <= 1e-12
    with pytest.raises(ValueError):
        npe_pfn.bar_cdf(lg, borders[:-1], ys)


def test_bucket_rule_is_the_nlls():
    _, borders = _case(64)
    ys = _edge_ys(borders)[:-1].astype(np.float32)
    np.testing.assert_array_equal(bucket64(borders.astype(np.float64), ys.astype(np.float64)), bar_bucket(borders, ys))


def test_pit_ks_statistic_equals_scipy():
    from scipy import stats
    from npe_pfn.diagnostics import pit_ks_statistic

    rng = np.random.default_rng(5)
    u = np.stack([rng.random(200), rng.beta(2.0, 1.0, 200), np.clip(rng.normal(0.5, 0.2, 200), 0, 1)], 1)
    got = pit_ks_statistic(torch.from_numpy(u))
    assert got.shape == (3,)
    for k in range(3):
        assert abs(float(got[k]) - stats.kstest(u[:, k], "uniform").statistic) <= 1e-12
    np.testing.assert_allclose(pit_ks_statistic(torch.from_numpy(u.reshape(20, 10, 3))).numpy(), got.numpy(), atol=0)
    with pytest.raises(ValueError):
        pit_ks_statistic(torch.zeros(5))
