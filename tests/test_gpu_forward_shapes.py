"""The forward at every row-tile and key-tile boundary against the oracle's goldens.

The engine's decoder logits and decoder-input tokens, per estimator, against
tests/golden/forward_shapes.npz (tests/golden/make_golden_forward_shapes.py: the bf16-emulating
CPU oracle on ModelConfig(n_layers=3, n_bars=250, n_estimators=2), preprocessing "none",
random_state 3; no oracle runs here).  A row has C = (F + 1) // 2 + 1 tokens; k_row_layer puts
256 // C whole rows into a 256-slot tile.

Set A, token-count edges: n = 40 context rows (24 from C = 128 on), N = 2 * (256 // C) + 1 query
rows (at least 3) -- per estimator two full tiles and a one-row tail tile:

    C           F              pins down
    2           1, 2           128 rows per tile, N = 257; odd F: a half zero-padded token
    16 | 17     30 | 31        1 | 2 key blocks; full tile | one dead slot
    32 | 33     62 | 63        2 | 3 key blocks
    48 | 49     94 | 95        3 | 4 key blocks
    64 | 65     126 | 127      key-block template | feat_attn_rows_long
    85 | 86     167 | 169      3 rows in 255 slots | 2 rows
    128 | 129   254 | 255      2 full rows | 1 row and 127 dead slots
    255 256|257 507 510 | 511  last fused sizes | first per-sublayer (wide) size

Set B, key-tile and query-block edges of the item attention at C = 3: n in 2, 31|32|33,
63|64|65, 127|128|129 with N = 129 (one query past a 128-query block); n = 64 with N = 1, 127,
128.

Set C, mixed launch: preprocessing "ensemble", F = 254, n = 30, N = 3, three estimators (two
would both be the SVD pipeline): 258, 258 and 129 tokens per row -- the per-sublayer path and the
fused long path in one forward.

Per-sublayer kernels at their own boundary (NPFN_UNFUSED=1): F = 282 | 283, C = 142 | 143:
k_feat_attn at its LDS cap | the first k_feat_attn_wide size.

Bars.  d_ref / t_ref of a case are the largest per-row, per-estimator TV / relative L2 distance
between the bf16-emulating and the fp32 oracle: what bf16 rounding at the engine's rounding
points does at that shape (d_ref 0.0032-0.0054, t_ref 0.0064-0.0096).  The engine differs from
the emulating oracle below that: accumulation order, exp2 / rcp approximations, the fast GELU.
Every row's probabilities softmax(logits_e / T) must be within min(4 d_ref, 0.02) TV of the
golden, every row's tokens within 4 t_ref; tests/test_forward_shapes_power.py shows that a single
dropped key is at least twice that bar away.  Each estimator is checked alone
(set_estimator_range(e, 1): the tile layout above) and in the full-range forward, and under
"none" the mixture of npfn_predict against the mean of the goldens.

The golden keeps every row at full resolution up to 33 query rows.  The larger cases (C = 2,
Set B) keep the rows on either side of each tile and block edge plus the first and last row
(tokens and all 250 bars), and for EVERY row the probabilities summed over bins of 10 bars, held
to the same bar (the TV of the bins is a lower bound of the TV of the bars).

Bitwise invariants at C = 17, 65, 85, 129, 256: predicting the first N - 1 rows gives those rows'
logits bit for bit, and an engine with the static tile schedule (NPFN_ROWK_STATIC=1) gives the
dynamic schedule's logits bit for bit.
"""
import os

import numpy as np
import pytest
import torch

import forward_shapes_ref as fs
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INVARIANT_CASES = ["A_F31", "A_F127", "A_F167", "A_F255", "A_F510"]   # C = 17, 65, 85, 129, 256


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, fs.GOLDEN_FILE)) as z:
        return {c.name: fs.Golden(z, c) for c in fs.CASES}


def _new_engine(case):
    from npe_pfn.engine import Engine

    return Engine(fs.config_of(case), fs.weights_of(case), device=DEV, random_state=fs.RANDOM_STATE,
                  preprocessing=case.mode)


@pytest.fixture(scope="module")
def engines():
    """Default-path engines by (n_estimators, preprocessing), shared by the cases."""
    cache = {}

    def get(case):
        key = (case.E, case.mode)
        if key not in cache:
            assert "NPFN_UNFUSED" not in os.environ and "NPFN_ROWK_STATIC" not in os.environ
            cache[key] = _new_engine(case)
        return cache[key]

    return get


def _tensors(case):
    return tuple(torch.from_numpy(a) for a in fs.table(case))


def _outputs(eng, case, e0, count):
    """(probs [count, N, nb] float64, tokens [count, N, d] float32) of estimators [e0, e0 + count)."""
    X, y, Xq = _tensors(case)
    eng.set_estimator_range(e0, count)
    eng.fit(X, y)
    lg = eng.forward_logits(Xq).float().cpu().numpy()
    tok = eng.forward_targets(Xq).float().cpu().numpy()
    assert lg.shape == (count, case.N, fs.CFG.n_bars) and tok.shape == (count, case.N, fs.CFG.d_model)
    assert np.isfinite(lg).all() and np.isfinite(tok).all()
    return fs.probs_of(lg, eng.cfg.softmax_temperature), tok


def _check(g, what, p, tok=None, e0=0):
    """Every row of p (and tok) of estimators e0.. against the golden; prints, then asserts."""
    case, E = g.case, p.shape[0]
    bar, tbar = min(4 * g.d_ref, 0.02), 4 * g.t_ref
    ref_p = g.probs[e0:e0 + E] if tok is not None else g.probs.mean(0, keepdims=True)
    d = fs.tv(p[:, g.rows], ref_p)
    msg = f"FWDSHAPE {case.name} {what}: d_ref {g.d_ref:.5f} t_ref {g.t_ref:.5f} TV max {d.max():.5f}"
    dc = t = None
    if g.coarse is not None:
        ref_c = g.coarse[e0:e0 + E] if tok is not None else g.coarse.mean(0, keepdims=True)
        dc = fs.tv(fs.coarse(p), ref_c)
        msg += f" coarse TV (all {case.N} rows) max {dc.max():.5f}"
    if tok is not None:
        t = fs.rel_l2(tok[:, g.rows], g.tokens[e0:e0 + E])
        msg += f" tokens rel L2 max {t.max():.5f}"
    print(msg)
    assert d.max() <= bar, (case.name, what, "TV", d.max(), bar, np.argwhere(d > bar)[:8].tolist())
    if dc is not None:
        assert dc.max() <= bar, (case.name, what, "coarse TV", dc.max(), bar, np.argwhere(dc > bar)[:8].tolist())
    if t is not None:
        assert t.max() <= tbar, (case.name, what, "tokens", t.max(), tbar, np.argwhere(t > tbar)[:8].tolist())


def _check_case(eng, g):
    case = g.case
    try:
        for e in range(case.E):
            p, tok = _outputs(eng, case, e, 1)
            _check(g, f"estimator {e} alone", p, tok, e0=e)
    finally:
        eng.full_range()
    p, tok = _outputs(eng, case, 0, case.E)
    _check(g, "full range", p, tok)
    return p


@pytest.mark.parametrize("name", [c.name for c in fs.CASES if c.mode == "none" and not c.unfused])
def test_token_and_context_edges_match_golden(engines, golden, name):
    """Sets A and B: per-estimator probabilities and tokens, and the npfn_predict mixture."""
    g = golden[name]
    assert g.tokens_per_row == (g.case.C,) * g.case.E
    eng = engines(g.case)
    _check_case(eng, g)
    _, _, Xq = _tensors(g.case)
    mix = torch.softmax(eng.predict_logits(Xq), -1).double().cpu().numpy()
    _check(g, "predict mixture", mix[None])


def test_mixed_launch_matches_golden(engines, golden):
    """Set C: the wide per-sublayer groups and the fused long group in one forward."""
    from oracle.preprocess_oracle import svd_components

    g = golden["C_F254"]
    case = g.case
    print("tokens per row of the estimators:", g.tokens_per_row)
    assert g.tokens_per_row == fs.SET_C_TOKENS
    eng = engines(case)
    _check_case(eng, g)
    # the engine's own pipelines: raw | quantile | k SVD | power columns and E fingerprints, i.e.
    # 2 F + k + 1 = 513 features (257 groups + target) and F + 1 = 255 (128 groups + target)
    k = svd_components(case.n, case.F)
    width = 3 * case.F + k + case.E
    X, y, _ = _tensors(case)
    eng.fit(X, y)
    assert eng.debug_views(case.n, width).shape == (case.n, width)


@pytest.mark.parametrize("name", ["U_F282", "U_F283"])
def test_per_sublayer_feature_attention_boundary_matches_golden(golden, monkeypatch, name):
    """NPFN_UNFUSED=1 at C = 142 (k_feat_attn at its LDS cap) and 143 (k_feat_attn_wide)."""
    g = golden[name]
    assert g.tokens_per_row == (g.case.C,) * g.case.E and g.case.C == {"U_F282": 142, "U_F283": 143}[name]
    monkeypatch.setenv("NPFN_UNFUSED", "1")
    eng = _new_engine(g.case)
    _check_case(eng, g)
    _, _, Xq = _tensors(g.case)
    _check(g, "predict mixture", torch.softmax(eng.predict_logits(Xq), -1).double().cpu().numpy()[None])


@pytest.mark.parametrize("name", [c.name for c in fs.CASES if c.name.startswith("A_")])
def test_per_sublayer_path_matches_golden_at_token_edges(golden, monkeypatch, name):
    """Set A once more on the per-sublayer kernels (NPFN_UNFUSED=1): k_feat_attn's own key
    blocks, its hand-over to k_feat_attn_wide between C = 129 and 255, and the K/V pack, against
    the same goldens with the same bars."""
    g = golden[name]
    monkeypatch.setenv("NPFN_UNFUSED", "1")
    _check_case(_new_engine(g.case), g)


def test_forward_logits_chunks_give_the_same_bits(golden):
    """npfn_forward_logits over chunks of 100 of A_F1's 257 query rows (npfn_set_chunk_rows):
    the unchunked call's logits bit for bit, and under a partial range the full range's."""
    case = fs.BY_NAME["A_F1"]
    eng = _new_engine(case)
    lg, _, tok = _logits(eng, case)
    eng.set_chunk_rows(100)
    lg_c, _, tok_c = _logits(eng, case)
    assert torch.equal(lg_c, lg) and torch.equal(tok_c, tok)
    X, y, Xq = _tensors(case)
    eng.set_estimator_range(1, 1)
    eng.fit(X, y)
    assert torch.equal(eng.forward_logits(Xq), lg[1:])


def _logits(eng, case, rows=None):
    """(per-estimator fp16 logits, mixture logits) of the first `rows` query rows, full range."""
    X, y, Xq = _tensors(case)
    eng.full_range()
    eng.fit(X, y)
    Xq = Xq if rows is None else Xq[:rows]
    return eng.forward_logits(Xq), eng.predict_logits(Xq), eng.forward_targets(Xq)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_prefix_of_the_rows_gives_the_same_bits(engines, name):
    """A row's result does not depend on which rows share its tiles: dropping the last row (the
    one-row tail tile) leaves every other row's logits and tokens bit for bit."""
    case = fs.BY_NAME[name]
    eng = engines(case)
    lg, mix, tok = _logits(eng, case)
    lg1, mix1, tok1 = _logits(eng, case, case.N - 1)
    assert torch.equal(lg1, lg[:, :-1]) and torch.equal(tok1, tok[:, :-1]) and torch.equal(mix1, mix[:-1])


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_static_tile_schedule_gives_the_same_bits(engines, monkeypatch, name):
    """NPFN_ROWK_STATIC=1 (tiles assigned by block index) against the dynamic tile counter."""
    case = fs.BY_NAME[name]
    lg, mix, tok = _logits(engines(case), case)
    monkeypatch.setenv("NPFN_ROWK_STATIC", "1")
    lg_s, mix_s, tok_s = _logits(_new_engine(case), case)
    assert torch.equal(lg_s, lg) and torch.equal(tok_s, tok) and torch.equal(mix_s, mix)
