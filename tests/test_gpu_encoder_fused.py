"""The encoder fused into the layer-0 row launch (NPFN_ENC_FUSED, default on) against k_encode.

With the switch on, k_encode_seed writes four scalars per token and the layer-0 launch of
k_row_layer expands them in registers; with NPFN_ENC_FUSED=0 k_encode writes every token's 192
values and the launch reads them back.  Both evaluate a token with the same fma chain, so the
two engines must agree bit for bit: per-estimator logits (npfn_forward_logits), the decoder's
input tokens, the predict mixture and an autoregressive sample's draws.

A row has C = (F + 1) // 2 + 1 tokens and a 256-slot tile holds 256 // C whole rows.  Cases:
33 context rows; 1, 37 and 300 query rows (one tile, a ragged last tile, rows per tile that do
not divide the rows); C = 2, 9, 25, 64 on the fused form and C = 66 on the long-row instances,
which keep k_encode under either setting; preprocessing "none" (one segment) and "ensemble"
(four estimators: two segments, C = 9 and C = 5, half of them with the target transform).
NaN, +inf and -inf cells sit in query rows everywhere and in the context rows under "none" --
the indicator branch of the seed on both the test side and, through the fit, the train side
(the ensemble's quantile, power and SVD fits of a non-finite column are not what this file is
about, so its context stays finite).

Outputs are compared as bit patterns (stricter than torch.equal, and defined if a value is NaN).
"""
import os
from contextlib import contextmanager
from dataclasses import replace

import numpy as np
import pytest
import torch

from npe_pfn.weights import ModelConfig, synthetic_weights

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CFG = ModelConfig(n_layers=3, n_bars=250, n_estimators=2)
N_CTX = 33
ROWS = (1, 37, 300)
F_NONE = {2: 1, 9: 15, 25: 48, 64: 126, 66: 130}   # C -> F (odd F: a half zero-padded token)
F_ENS = 6


@contextmanager
def _env(value):
    old = os.environ.get("NPFN_ENC_FUSED")
    os.environ["NPFN_ENC_FUSED"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["NPFN_ENC_FUSED"]
        else:
            os.environ["NPFN_ENC_FUSED"] = old


@pytest.fixture(scope="module")
def engines():
    """(fused, k_encode) engine pairs by preprocessing mode, the switch set before creation."""
    from npe_pfn.engine import Engine

    cache = {}

    def get(mode):
        if mode not in cache:
            cfg = CFG if mode == "none" else replace(CFG, n_estimators=4)
            w = synthetic_weights(cfg, seed=0)
            pair = []
            for value in ("1", "0"):
                with _env(value):
                    pair.append(Engine(cfg, w, device=DEV, random_state=3, preprocessing=mode))
            cache[mode] = tuple(pair)
        return cache[mode]

    return get


def _table(F, N, holes_in_context):
    """(X [33, F], y [33], Xq [N, F]) with NaN, +inf and -inf cells."""
    rng = np.random.default_rng(100 * F + N)
    z = rng.normal(size=(N_CTX + N, 3))
    X = (z @ rng.normal(size=(3, F)) + 0.3 * rng.normal(size=(N_CTX + N, F))).astype(np.float32)
    y = (z[:N_CTX, 0] + 0.2 * rng.normal(size=N_CTX)).astype(np.float32)
    Xc, Xq = X[:N_CTX].copy(), X[N_CTX:].copy()
    vals = (np.nan, np.inf, -np.inf)
    for i, v in enumerate(vals):
        Xq[(i * 7) % N, (i * 5) % F] = v            # first rows: present at N = 1 as well
        Xq[N - 1 - (i % N), (F - 1 - i) % F] = v    # the last (ragged) tile's rows
        if holes_in_context:
            Xc[3 + 9 * i, (2 * i) % F] = v
            Xc[N_CTX - 1 - i, (F - 1 - 2 * i) % F] = v
    return tuple(torch.from_numpy(a) for a in (Xc, y, Xq))


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _outputs(eng, X, y, Xq):
    eng.fit(X, y)
    return eng.forward_logits(Xq), eng.forward_targets(Xq), eng.predict_logits(Xq)


def _compare(engines, mode, F, N, holes_in_context):
    X, y, Xq = _table(F, N, holes_in_context)
    on, off = engines(mode)
    got = _outputs(on, X, y, Xq)
    ref = _outputs(off, X, y, Xq)
    E = on.cfg.n_estimators
    assert got[0].shape == (E, N, CFG.n_bars) and got[2].shape == (N, CFG.n_bars)
    for what, a, b in zip(("logits", "tokens", "mixture"), got, ref):
        print(f"ENCFUSED {mode} F {F} N {N} {what}: finite {bool(torch.isfinite(a.float()).all())}"
              f" differing {int((_bits(a) != _bits(b)).sum())}")
        assert _same(a, b), (mode, F, N, what)


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("C", list(F_NONE))
def test_one_segment_gives_k_encodes_bits(engines, C, N):
    """Preprocessing "none": one segment of C tokens per row (C = 66: the long-row instance)."""
    F = F_NONE[C]
    assert (F + 1) // 2 + 1 == C
    _compare(engines, "none", F, N, holes_in_context=True)


@pytest.mark.parametrize("N", ROWS)
def test_two_segments_give_k_encodes_bits(engines, N):
    """Preprocessing "ensemble": the SVD pipelines (C = 9) and the fingerprint ones (C = 5) in one
    launch, with and without the target transform."""
    from oracle.preprocess_oracle import MODE_ENSEMBLE, estimator_configs, n_features_of

    tokens = [(n_features_of(t, F_ENS, N_CTX) + 1) // 2 + 1 for t, _ in estimator_configs(MODE_ENSEMBLE, 4)]
    assert tokens == [9, 9, 5, 5]
    assert [tt for _, tt in estimator_configs(MODE_ENSEMBLE, 4)] == [False, True, False, True]
    _compare(engines, "ensemble", F_ENS, N, holes_in_context=False)


def test_ar_sample_gives_equal_draws(engines):
    """One autoregressive sample of 50 rows over 3 dims: the per-step fits (train side) and
    forwards (test side) of both engines draw the same values."""
    rng = np.random.default_rng(5)
    n, dx, dth, N = N_CTX, 2, 3, 50
    th = rng.normal(size=(n, dth)).astype(np.float32)
    x = (th @ rng.normal(size=(dth, dx)) + 0.3 * rng.normal(size=(n, dx))).astype(np.float32)
    xq = np.repeat(x[:1], N, 0)
    draws = []
    for eng in engines("ensemble"):
        theta, _ = eng.ar_sample(torch.from_numpy(x), torch.from_numpy(th), torch.from_numpy(xq), counter=0)
        assert theta.shape == (N, dth) and bool(torch.isfinite(theta).all())
        draws.append(theta)
    assert torch.equal(draws[0], draws[1])
