"""CPU checks behind the forward shape-edge goldens (tests/golden/forward_shapes.npz).

* OracleTabPFN.target_tokens is the decoder input of _estimator_logits: the decoder applied to
  it reproduces the logits bit for bit, under both roundings and with two estimator groups.
* The golden file cannot drift from the oracle: two cheap cases are regenerated and compared.
  Tolerances: the file keeps probabilities as float16 (<= 2.5e-4 TV) and another BLAS or thread
  count may reorder the oracle's fp32 sums (a few bf16 roundings flip: ~1e-4 relative L2), so
  TV <= 5e-4, tokens 1e-3 relative L2, d_ref / t_ref 5 % -- all far below d_ref ~ 4e-3 and
  t_ref ~ 7e-3, the smallest change to the oracle's arithmetic that the file could hide.
* The file's layout: every case present, the stored rows and the token counts as declared.
"""
import os

import numpy as np
import pytest

import forward_shapes_ref as fs
from conftest import GOLDEN
from oracle.tabpfn_oracle import OracleTabPFN


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, fs.GOLDEN_FILE)) as z:
        return {c.name: fs.Golden(z, c) for c in fs.CASES}


@pytest.mark.parametrize("emulate", [True, False])
@pytest.mark.parametrize("mode", ["none", "ensemble"])
def test_decoder_on_target_tokens_reproduces_estimator_logits(emulate, mode):
    case = fs.Case("t", 5, 12, 4, "", mode=mode, E=3)   # ensemble: two token counts, two estimator groups
    orc = fs.fit_oracle(case, emulate)
    _, _, Xq = fs.table(case)
    tok = orc.target_tokens(Xq)
    assert tok.shape == (3, 4, fs.CFG.d_model) and tok.dtype == np.float32
    if emulate:
        fs.bf16_bits(tok)   # asserts bf16 values
    lg = orc._estimator_logits(Xq)
    groups = OracleTabPFN._groups(orc.state)
    assert len(groups) == (2 if mode == "ensemble" else 1)
    for a, b in groups:   # group by group: the GEMM shapes of _estimator_logits
        assert np.array_equal(orc.decode_tokens(tok[a:b]), lg[a:b])
    _, lg2 = orc.predict_probs(Xq, return_estimator_logits=True)
    assert np.array_equal(lg, lg2)


def test_golden_file_holds_every_case(golden):
    for c in fs.CASES:
        g = golden[c.name]
        rows = fs.edge_rows(c)
        assert np.array_equal(g.rows, rows), c.name
        assert g.probs.shape == (c.E, len(rows), fs.CFG.n_bars) and g.tokens.shape == (c.E, len(rows), fs.CFG.d_model)
        assert (g.coarse is None) == (len(rows) == c.N), c.name
        if g.coarse is not None:
            assert g.coarse.shape == (c.E, c.N, fs.CFG.n_bars // fs.COARSE)
            assert fs.tv(g.coarse[:, rows], fs.coarse(g.probs)).max() <= 1e-3
        assert g.tokens_per_row == (fs.SET_C_TOKENS if c.name == "C_F254" else (c.C,) * c.E), c.name
        assert 0 < g.d_ref < 0.01 and 0 < g.t_ref < 0.02, (c.name, g.d_ref, g.t_ref)
        assert np.abs(g.probs.sum(-1) - 1).max() <= 1e-3


@pytest.mark.parametrize("name", ["A_F31", "B_n33_N129"])
def test_golden_file_matches_the_oracle(golden, name):
    case, g = fs.BY_NAME[name], golden[name]
    new = fs.golden_arrays(case)
    assert np.array_equal(new["rows"], g.rows) and tuple(new["tokens_per_row"]) == g.tokens_per_row
    assert fs.tv(new["probs"].astype(np.float64), g.probs).max() <= 5e-4
    assert fs.rel_l2(fs.bf16_from_bits(new["tokens"]), g.tokens).max() <= 1e-3
    if g.coarse is not None:
        assert fs.tv(new["coarse"].astype(np.float64), g.coarse).max() <= 5e-4
    assert abs(float(new["d_ref"]) - g.d_ref) <= 0.05 * g.d_ref, (float(new["d_ref"]), g.d_ref)
    assert abs(float(new["t_ref"]) - g.t_ref) <= 0.05 * g.t_ref, (float(new["t_ref"]), g.t_ref)
