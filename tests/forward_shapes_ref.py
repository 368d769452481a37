"""Cases, data model and distances shared by the forward shape-edge tests.

Used by tests/golden/make_golden_forward_shapes.py (writes tests/golden/forward_shapes.npz from
the CPU oracle alone), tests/test_forward_shapes_host.py and tests/test_forward_shapes_power.py
(CPU) and tests/test_gpu_forward_shapes.py (the engine against the file).

Model: ModelConfig(n_layers=3, n_bars=250, n_estimators=2), synthetic_weights(cfg, seed=0),
random_state 3 -- small enough for the CPU oracle to run every case in seconds, and three layers
are enough for every sublayer kernel to see the output of every other.  Data: the model of
test_wide_tables_long_rows_match_oracle (three latent factors, X = z A + 0.3 noise,
y = z0 + 0.2 noise) drawn from numpy.random.default_rng(F).

A row has C = (F + 1) // 2 + 1 tokens under preprocessing "none" (two features per token plus
the target); the row kernel puts 256 // C whole rows into a 256-slot tile.
"""
from dataclasses import dataclass, replace

import numpy as np

from npe_pfn.weights import ModelConfig, synthetic_weights
from oracle.tabpfn_oracle import OracleTabPFN, softmax

CFG = ModelConfig(n_layers=3, n_bars=250, n_estimators=2)
RANDOM_STATE = 3
GOLDEN_FILE = "forward_shapes.npz"
FULL_ROWS_MAX = 33   # cases with more query rows keep full-resolution goldens for edge_rows() only
COARSE = 10          # bars per bin of the all-rows coarse probabilities of those cases
MODES = {"none": 0, "ensemble": 3}


@dataclass(frozen=True)
class Case:
    name: str
    F: int
    n: int            # context rows
    N: int            # query rows
    what: str         # the boundary the case pins down
    mode: str = "none"
    E: int = 2        # n_estimators
    unfused: bool = False   # run on the per-sublayer path (NPFN_UNFUSED=1)

    @property
    def C(self) -> int:
        return (self.F + 1) // 2 + 1


def tokens_of(F: int) -> int:
    return (F + 1) // 2 + 1


def _set_a():
    what = {
        1: "C=2, odd F: 128 rows per tile, N = 257",
        2: "C=2: 128 rows per tile, N = 257",
        30: "C=16: one key block, 16 rows fill the tile",
        31: "C=17: two key blocks, 15 rows and one dead slot",
        62: "C=32: two key blocks",
        63: "C=33: three key blocks",
        94: "C=48: three key blocks",
        95: "C=49: four key blocks",
        126: "C=64: last size of the key-block template",
        127: "C=65: first feat_attn_rows_long size",
        167: "C=85: 3 rows in 255 slots",
        169: "C=86: 2 rows per tile",
        254: "C=128: 2 rows fill the tile",
        255: "C=129: 1 row and 127 dead slots",
        507: "C=255: fused, one dead slot, odd F",
        510: "C=256: last fused size, the row fills the tile",
        511: "C=257: first per-sublayer (wide) size",
    }
    out = []
    for F, w in what.items():
        C = tokens_of(F)
        out.append(Case(f"A_F{F}", F, 24 if C >= 128 else 40, max(3, 2 * (256 // C) + 1), w))
    return out


def _set_b():
    out = [Case(f"B_n{n}_N129", 3, n, 129, f"{n} context rows (32-key tiles, 64-key steps), 129 queries")
           for n in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
    out += [Case(f"B_n64_N{N}", 3, 64, N, f"64 context rows, {N} queries (128-query blocks)") for N in (1, 127, 128)]
    return out


CASES = _set_a() + _set_b() + [
    # the ensemble's first three estimators: quantile + original + SVD (twice, the second with the
    # target transform) and power + fingerprint -- two estimators alone would both be the former
    Case("C_F254", 254, 30, 3, "ensemble: 258 tokens (wide path) and 129 tokens (fused long path) in one forward",
         mode="ensemble", E=3),
    Case("U_F282", 282, 24, 3, "per-sublayer path, C=142: k_feat_attn at its LDS cap", unfused=True),
    Case("U_F283", 283, 24, 3, "per-sublayer path, C=143: first k_feat_attn_wide size", unfused=True),
]
BY_NAME = {c.name: c for c in CASES}
SET_C_TOKENS = (258, 258, 129)   # per estimator of C_F254, asserted by the maker and the tests


def config_of(case: Case) -> ModelConfig:
    return CFG if case.E == CFG.n_estimators else replace(CFG, n_estimators=case.E)


def weights_of(case: Case):
    return synthetic_weights(config_of(case), seed=0)


def table(case: Case):
    """(X [n, F], y [n], Xq [N, F]) float32 of a case."""
    rng = np.random.default_rng(case.F)
    n, N, F = case.n, case.N, case.F
    z = rng.normal(size=(n + N, 3))
    X = (z @ rng.normal(size=(3, F)) + 0.3 * rng.normal(size=(n + N, F))).astype(np.float32)
    y = (z[:n, 0] + 0.2 * rng.normal(size=n)).astype(np.float32)
    return X[:n], y, X[n:]


def edge_rows(case: Case) -> np.ndarray:
    """Query rows with full-resolution goldens: all of them up to FULL_ROWS_MAX rows; past that
    the first and last row, the rows on either side of every row-kernel tile edge and of the
    128-query block edge."""
    N = case.N
    if N <= FULL_ROWS_MAX:
        return np.arange(N)
    T = 256 // case.C
    rows = {0, N - 1, 127, 128}
    for k in range(T, N, T):
        rows |= {k - 1, k}
    return np.array(sorted(r for r in rows if 0 <= r < N))


def probs_of(logits: np.ndarray, T: float) -> np.ndarray:
    """Per-estimator probabilities softmax(logits_e / T), float64."""
    return softmax(np.asarray(logits, dtype=np.float32) * np.float32(1.0 / T), -1).astype(np.float64)


def coarse(p: np.ndarray) -> np.ndarray:
    """Probabilities summed over bins of COARSE bars: TV of the bins <= TV of the bars."""
    return p.reshape(p.shape[:-1] + (p.shape[-1] // COARSE, COARSE)).sum(-1)


def tv(p, q) -> np.ndarray:
    return 0.5 * np.abs(np.asarray(p, np.float64) - np.asarray(q, np.float64)).sum(-1)


def rel_l2(a, ref) -> np.ndarray:
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((a - ref) ** 2).sum(-1)) / np.sqrt((ref ** 2).sum(-1))


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """bf16-representable float32 -> its upper 16 bits."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def bf16_from_bits(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def fit_oracle(case: Case, emulate: bool, weights=None) -> OracleTabPFN:
    cfg = config_of(case)
    orc = OracleTabPFN(weights if weights is not None else weights_of(case), cfg.n_estimators,
                       cfg.softmax_temperature, seed=RANDOM_STATE, emulate_bf16=emulate, preprocessing=MODES[case.mode])
    X, y, _ = table(case)
    orc.fit(X, y)
    return orc


def oracle_outputs(orc: OracleTabPFN, case: Case):
    """(probs [E, N, nb] float64, tokens [E, N, d] float32) of a fitted oracle."""
    _, _, Xq = table(case)
    tok = orc.target_tokens(Xq)
    return probs_of(orc.decode_tokens(tok), orc.T), tok


def golden_arrays(case: Case, weights=None) -> dict:
    """What the golden file holds for a case (see make_golden_forward_shapes.py)."""
    emu = fit_oracle(case, True, weights)
    p, tok = oracle_outputs(emu, case)
    p32, tok32 = oracle_outputs(fit_oracle(case, False, weights), case)
    rows = edge_rows(case)
    out = {
        "shape": np.array([case.F, case.n, case.N, case.E, RANDOM_STATE], dtype=np.int64),
        "tokens_per_row": np.array([es.n_groups + 1 for es in emu.state.estimators], dtype=np.int64),
        "rows": rows.astype(np.int32),
        "probs": p[:, rows].astype(np.float16),
        "tokens": bf16_bits(tok[:, rows]),
        "d_ref": np.float64(tv(p, p32).max()),
        "t_ref": np.float64(rel_l2(tok, tok32).max()),
    }
    if len(rows) < case.N:
        out["coarse"] = coarse(p).astype(np.float16)
    return out


class Golden:
    """One case of the golden file."""

    def __init__(self, z, case: Case):
        g = {k: z[f"{case.name}/{k}"] for k in ("shape", "tokens_per_row", "rows", "probs", "tokens", "d_ref", "t_ref")}
        assert tuple(g["shape"]) == (case.F, case.n, case.N, case.E, RANDOM_STATE), (case.name, g["shape"])
        self.case = case
        self.tokens_per_row = tuple(int(c) for c in g["tokens_per_row"])
        self.rows = g["rows"].astype(np.int64)
        self.probs = g["probs"].astype(np.float64)          # [E, len(rows), nb]
        self.tokens = bf16_from_bits(g["tokens"])           # [E, len(rows), d]
        self.d_ref, self.t_ref = float(g["d_ref"]), float(g["t_ref"])
        key = f"{case.name}/coarse"
        self.coarse = z[key].astype(np.float64) if key in z.files else None   # [E, N, nb / COARSE]
