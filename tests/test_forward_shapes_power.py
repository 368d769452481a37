"""The forward shape-edge bar has teeth: one dropped feature-attention key is seen (CPU only).

tests/test_gpu_forward_shapes.py holds the engine's per-estimator probabilities to
min(4 * d_ref, 0.02) TV of the golden on every row.  Here three deliberately wrong oracles run
the C = 17 case (A_F31: 40 context rows, 31 query rows).  Each wraps the softmax of the oracle's
feature attention so that key C - 2, the last feature token, gets no weight

* for every query of every row,
* for the target token's query only,
* for the first row of each of the oracle's row chunks only (one row in eight at 2 threads),

in the fit and in the predict, every layer.  Each must be at least twice the bar away from the
golden on at least one row -- so nobody can later widen the bar until it no longer sees a one-key
masking error without this test failing first.  Measured: 0.087 / 0.075 / 0.047 on the worst row
against a bar of 0.018.  The unpatched oracle must reproduce the golden (up to its float16
storage).
"""
import os

import numpy as np
import pytest

import forward_shapes_ref as fs
import oracle.tabpfn_oracle as orc_mod
from conftest import GOLDEN

CASE = fs.BY_NAME["A_F31"]
DROP = CASE.C - 2


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, fs.GOLDEN_FILE)) as z:
        return fs.Golden(z, CASE)


def _drop_all(sc):
    sc[..., DROP] = -np.inf


def _drop_target_query(sc):
    sc[:, :, CASE.C - 1, DROP] = -np.inf


def _drop_first_row_of_chunk(sc):
    sc[0, ..., DROP] = -np.inf


def _tv_to_golden(monkeypatch, golden, mutate):
    """Largest and per-row TV to the golden of the emulating oracle whose feature-attention scores
    ([rows, heads, C queries, C keys], the only 4-D softmax of the oracle) pass through mutate."""
    plain = orc_mod.softmax

    def wrapped(x, axis=-1):
        x = np.asarray(x, dtype=np.float32)
        if mutate is not None and x.ndim == 4:
            assert x.shape[-2:] == (CASE.C, CASE.C), x.shape
            x = x.copy()
            mutate(x)
        return plain(x, axis)

    monkeypatch.setenv("NPFN_ORACLE_THREADS", "2")   # 8 row chunks per call, whatever the host
    monkeypatch.setattr(orc_mod, "softmax", wrapped)
    p, _ = fs.oracle_outputs(fs.fit_oracle(CASE, True), CASE)
    return fs.tv(p[:, golden.rows], golden.probs)   # [E, N]


def test_unpatched_oracle_is_the_golden(monkeypatch, golden):
    assert _tv_to_golden(monkeypatch, golden, None).max() <= 5e-4


@pytest.mark.parametrize("mutate", [_drop_all, _drop_target_query, _drop_first_row_of_chunk],
                         ids=["every_query", "target_query", "first_row_of_chunk"])
def test_one_dropped_key_is_twice_the_bar_away(monkeypatch, golden, mutate):
    bar = min(4 * golden.d_ref, 0.02)
    d = _tv_to_golden(monkeypatch, golden, mutate)
    print(f"{mutate.__name__}: TV to the golden max {d.max():.4f} median {np.median(d):.4f}; bar {bar:.4f}")
    assert d.max() >= 2 * bar, (d.max(), bar)
