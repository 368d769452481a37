"""CPU side of the regressor's summary outputs (mean / median / mode / quantiles).

* tests/bar_stats_ref.py, the reference the GPU tests compare against, checked against closed
  forms and against the oracle's ``bar_sample``;
* the C-ABI declares and binds npfn_bar_stats / npfn_predict_stats;
* TabPFNRegressor.predict's argument checks run before any engine exists.
"""
import os
import re

import numpy as np
import pytest
import torch

from bar_stats_ref import ref_cdf, ref_icdf, ref_icdf64, ref_mean, ref_mode_density
from conftest import ROOT
from oracle.tabpfn_oracle import HALFNORMAL_MEDIAN, bar_sample


def _inputs(R=16, nb=200, seed=0):
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(R, nb)) * 2).astype(np.float32)
    borders = np.sort(rng.normal(size=nb + 1)).astype(np.float32) * 3
    return logits, borders


def test_mean_of_a_tail_bar_is_the_half_normal_mean():
    _, borders = _inputs()
    nb = borders.size - 1
    b = borders.astype(np.float64)
    first = np.full((1, nb), -np.inf, np.float32)
    first[0, 0] = 0.0
    last = np.full((1, nb), -np.inf, np.float32)
    last[0, -1] = 0.0
    hn0 = float(torch.distributions.HalfNormal(torch.tensor((b[1] - b[0]) / HALFNORMAL_MEDIAN, dtype=torch.float64)).mean)
    hn1 = float(torch.distributions.HalfNormal(torch.tensor((b[-1] - b[-2]) / HALFNORMAL_MEDIAN, dtype=torch.float64)).mean)
    assert abs(ref_mean(first, borders)[0] - (b[1] - hn0)) <= 1e-12
    assert abs(ref_mean(last, borders)[0] - (b[-2] + hn1)) <= 1e-12


def test_mean_of_equal_interior_bars_is_the_midpoint():
    nb = 50
    borders = np.linspace(-2.0, 3.0, nb + 1).astype(np.float32)
    logits = np.full((1, nb), 0.7, np.float32)
    logits[0, 0] = logits[0, -1] = -np.inf   # no tail mass
    mid = 0.5 * (float(borders[1]) + float(borders[-2]))
    assert abs(ref_mean(logits, borders)[0] - mid) <= 1e-6   # the fp32 linspace is equal-width to 1 ulp only


def test_cdf_inverts_icdf():
    logits, borders = _inputs()
    logits[:3, :120] = -np.inf    # zero-mass bars in front
    logits[3, 60:] = -np.inf      # and behind
    for q in (0.0, 1e-6, 0.1, 0.5, 0.9, 1 - 1e-6, 1.0):
        x = ref_icdf64(logits, borders, q)
        np.testing.assert_allclose(ref_cdf(logits, borders, x), q, rtol=0, atol=1e-12)
    q = np.random.default_rng(3).uniform(size=logits.shape[0])
    np.testing.assert_allclose(ref_cdf(logits, borders, ref_icdf64(logits, borders, q)), q, rtol=0, atol=1e-12)


def test_icdf_is_the_oracle_bar_sample():
    """ref_icdf is oracle.bar_sample wherever that is finite; the spelled-out ref_icdf64 agrees
    with it (fp32 softmax and fp32 result there, fp64 here: 1e-5 of the span), and fills the
    zero-mass bar the oracle's searchsorted picks at q = 0."""
    logits, borders = _inputs()
    span = float(borders[-1] - borders[0])
    for q in (0.1, 0.5, 0.9, np.random.default_rng(4).uniform(size=logits.shape[0])):
        x = ref_icdf(logits, borders, q)
        assert np.array_equal(x, bar_sample(logits, borders, np.broadcast_to(np.float64(q), (logits.shape[0],))))
        assert np.abs(x - ref_icdf64(logits, borders, q)).max() <= 1e-5 * span
    logits[:, :120] = -np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        assert not np.isfinite(bar_sample(logits, borders, np.zeros(logits.shape[0]))).any()
    np.testing.assert_array_equal(ref_icdf(logits, borders, 0.0), np.full(logits.shape[0], borders[120]))
    # q = 1: the right border of the last bar with mass, up to the oracle's fp32 softmax total
    assert np.abs(ref_icdf(logits, borders, 1.0) - borders[-1]).max() <= 1e-4 * span
    np.testing.assert_allclose(ref_icdf64(logits, borders, 1.0), borders[-1], rtol=0, atol=1e-9)


def test_mode_density_skips_zero_width_bars():
    logits, borders = _inputs(R=2, nb=8)
    borders[3] = borders[4]
    d = ref_mode_density(logits, borders)
    assert np.isneginf(d[:, 3]).all() and np.isfinite(np.delete(d, 3, axis=1)).all()


def test_abi_declares_and_binds_the_stats_entry_points():
    from npe_pfn.engine import LIB_PATH, SIGNATURES, load_library

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npfn.h")).read(), flags=re.S)
    for name in ("npfn_bar_stats", "npfn_predict_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", src), f"include/npfn.h does not declare {name}"
        assert name in SIGNATURES, f"{name} has no ctypes signature in npe_pfn/engine.py"
        assert len(SIGNATURES[name][1]) == 10
    if not os.path.exists(LIB_PATH):
        pytest.fail("libnpfn.so is not built; run `make -C npe-pfn_amd` (__graft_entry__.build())")
    lib = load_library()
    assert hasattr(lib, "npfn_bar_stats") and hasattr(lib, "npfn_predict_stats")


@pytest.mark.parametrize("kwargs", [
    dict(output_type="nope"),
    dict(output_type="quantiles", quantiles=[1.5]),
    dict(output_type="quantiles", quantiles=[-0.1]),
    dict(output_type="quantiles", quantiles=list(np.linspace(0, 1, 65))),
    dict(output_type="full", quantiles=[1.5]),
])
def test_predict_argument_checks_need_no_engine(kwargs):
    from npe_pfn.tabpfn import TabPFNRegressor

    reg = TabPFNRegressor(device="cpu")   # any touch of reg.engine would raise for the device
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError, match="output_type|quantiles"):
        reg.predict(X, **kwargs)
    with pytest.raises(ValueError, match="output_type|quantiles"):
        reg.predict_tensor(X, **kwargs)
    assert reg._engine is None


def test_stats_request_lists():
    from npe_pfn.tabpfn import TabPFNRegressor

    reg = TabPFNRegressor(device="cpu")
    deciles = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
    assert reg._stats_request("quantiles", None) == (deciles, False, False)
    assert reg._stats_request("main", None) == (deciles + [0.5], True, True)
    assert reg._stats_request("main", [0.25]) == ([0.25, 0.5], True, True)
    assert reg._stats_request("median", [0.3]) == ([0.5], False, False)
    assert reg._stats_request("mean", None) == ([], True, False)
    assert reg._stats_request("mode", None) == ([], False, True)
    assert reg._stats_request("full", []) == ([], False, False)
