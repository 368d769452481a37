"""Case table and helpers of the preprocessing edge suite (TEST INFRASTRUCTURE).

tests/test_preprocess_edges_host.py proves on the CPU that the cases below are fair (they reach
the branch they name, the oracle is sklearn's on them, the likelihoods are curved, the SVDs are
determined); tests/test_gpu_preprocess_edges.py runs them through the engine.  Every expected
value comes from oracle/preprocess_oracle.py; nothing here reads the engine.

The tables are literal: no case is generated, skipped or filtered at run time, and the host test
counts them.  One engine fit per case, on ``ModelConfig(n_layers=1, n_bars=250)`` with eight
estimators (every pipeline of every mode occurs: ``estimator_configs``).
"""
from __future__ import annotations

import numpy as np

from oracle import preprocess_oracle as po

SEED = 11          # the engine's random_state: fingerprint salts and the quantile subsample follow it
E = 8              # ModelConfig().n_estimators
MODES = {"quantile": po.MODE_QUANTILE, "quantile+power": po.MODE_QUANTILE_POWER, "ensemble": po.MODE_ENSEMBLE}

# device constants the cases are built around (npfn_kernels.hip / npfn_kernels.h)
PF_REGS_MAX = 2048         # PF_THREADS * PF_VPT: (sign, log1p|x|) in registers
QT_SORT_MAX = 16384        # k_power_fit keeps the column in LDS up to here
FP_MIN = 4                 # kFpMin: candidates precomputed for an early row
FP_ONE_WAVE_MAX = 4096     # k_fp_train_resolve runs 64 threads up to here, 1024 beyond


def small_cfg():
    from npe_pfn.weights import ModelConfig

    return ModelConfig(n_layers=1, n_bars=250)


# ============================================================================ 1. quantile cases
# (id, mode, n, columns): "base" = continuous | five-valued ties | constant; "planted" adds four
# columns whose finite counts are 0, 1, 128 and 129 (the rest NaN / +inf / -inf).
QUANTILE_CASES = (
    ("q-n2", "quantile", 2, "base"),
    ("q-n3", "quantile", 3, "base"),
    ("q-n9", "quantile", 9, "base"),
    ("q-n10", "quantile", 10, "base"),
    ("q-n11", "quantile", 11, "base"),
    ("q-n15", "quantile", 15, "base"),
    ("q-n255", "quantile", 255, "base"),
    ("q-n256", "quantile", 256, "base"),
    ("q-n257", "quantile", 257, "planted"),
    ("q-n320", "quantile", 320, "base"),
    ("q-n325", "quantile", 325, "base"),
    ("q-n1285", "quantile", 1285, "base"),
    ("q-n10000", "quantile", 10_000, "base"),
    ("q-n10001", "quantile", 10_001, "base"),
    # one ensemble fit per size class (tiny, sort edge, several quantiles per thread, subsample):
    # the SVD reads the same raw | quantile columns
    ("qe-n10", "ensemble", 10, "base"),
    ("qe-n256", "ensemble", 256, "base"),
    ("qe-n1285", "ensemble", 1285, "base"),
    ("qe-n10001", "ensemble", 10_001, "base"),
)
PLANTED_FINITE = (0, 1, 128, 129)
CLASSIFIER_CASE = ("qc-n330", "ensemble", 330, "base")   # fit_classes, K = 3: div = 10
CLASSIFIER_K = 3


def quantile_table(n: int, columns: str):
    """(X [n, F], y [n]) of a quantile case."""
    rng = np.random.default_rng(1000 + n)
    cont = np.exp(1.5 * rng.normal(size=n))
    ties = rng.integers(0, 5, size=n).astype(np.float64)
    cols = [cont, ties, np.full(n, 3.0)]
    if columns == "planted":
        bad = np.array([np.nan, np.inf, -np.inf])
        for c, keep in enumerate(PLANTED_FINITE):
            col = rng.normal(size=n) * 2.0 + 1.0
            drop = rng.permutation(n)[: n - keep]
            col[drop] = bad[(np.arange(drop.size) + c) % 3]
            cols.append(col)
    X = np.stack(cols, 1).astype(np.float32)
    y = (0.5 * np.log(cont) + 0.3 * rng.normal(size=n)).astype(np.float32)
    return X, y


QUERY_ROWS = 20


def query_values(q: np.ndarray) -> np.ndarray:
    """The query values of one column with quantile table q (float32 [QUERY_ROWS]): both ends,
    nextafter on both sides of either, a repeated quantile (the middle one where none repeats) and
    its neighbours, midpoints of the first, middle and last cell, a far value on either side,
    +-inf, NaN, -0.0 and 0.0."""
    f = np.float32
    if q.size == 0:
        q = np.array([-1.0, 1.0])
    lo, hi = f(q[0]), f(q[-1])
    inner = q[1:-1] if q.size > 2 else q
    vals, cnt = np.unique(inner, return_counts=True)
    rep = f(vals[np.argmax(cnt)]) if cnt.max() > 1 else f(q[q.size // 2])
    m = q.size // 2
    mids = [0.5 * (q[0] + q[min(1, q.size - 1)]), 0.5 * (q[max(m - 1, 0)] + q[m]), 0.5 * (q[-2 if q.size > 1 else -1] + q[-1])]
    out = [lo, hi, np.nextafter(lo, f(-np.inf)), np.nextafter(lo, f(np.inf)), np.nextafter(hi, f(-np.inf)),
           np.nextafter(hi, f(np.inf)), rep, np.nextafter(rep, f(-np.inf)), np.nextafter(rep, f(np.inf)),
           f(mids[0]), f(mids[1]), f(mids[2]), f(lo - 10.0 - abs(lo)), f(hi + 10.0 + abs(hi)),
           f(np.inf), f(-np.inf), f(np.nan), f(-0.0), f(0.0), f(0.5 * (float(lo) + float(hi)))]
    assert len(out) == QUERY_ROWS
    return np.asarray(out, dtype=np.float32)


def quantile_queries(qtabs) -> np.ndarray:
    return np.stack([query_values(q) for q in qtabs], 1)


# ============================================================================ 2. power cases
POWER_SIZE_CASES = (("p-n2048", 2048), ("p-n2049", 2049), ("p-n16384", 16_384), ("p-n16385", 16_385))
POWER_SIZE_COLUMNS = ("lognormal", "normal")
# the columns of the n = 300 corner fit, in order; kind: "clamp+" / "clamp-" (lambda = +-6), "identity"
# (lambda = 1: constant or no finite value), "fit" (an interior optimum)
POWER_CORNER_N = 300
POWER_CORNER_COLUMNS = (
    ("clamp_hi", "clamp+"),
    ("clamp_lo", "clamp-"),
    ("constant", "identity"),
    ("all_nan", "identity"),
    ("holes", "fit"),
    ("two_values", "fit"),
    ("outlier", "fit"),
)
# the same columns as the target (finite ones only): one ensemble fit each
POWER_TARGET_CASES = (
    ("t-clamp_hi", "clamp_hi", "clamp+"),
    ("t-clamp_lo", "clamp_lo", "clamp-"),
    ("t-constant", "constant", "identity"),
    ("t-two_values", "two_values", "fit"),
    ("t-outlier", "outlier", "fit"),
)
CLAMP_BRACKET = 1e-8      # the search's final bracket: 2 * 0.618^40 = 9e-9
LLF_CURVATURE_MIN = 1e-7  # yj_neg_llf(lam +- 1e-4) - yj_neg_llf(lam) of every "fit" column
# Margin of criterion (b): LLF_FACTOR times the spread of the oracle's own likelihood over its final
# bracket (pure float64 evaluation noise: the parabola contributes < 1e-13 there).  The factor: a
# golden-section search on a noisy function ends within two noise amplitudes of the minimum, on
# each side of the comparison (2 + 2); the device's one-pass variance S2 - S1^2 / n of the shifted
# values loses mean^2 / var more than the oracle's two-pass form, which is below 8 for every
# column here (shifted by the minimum, the values are one-signed: mean^2 / var <= a few) -- 4 * 8.
LLF_FACTOR = 32.0


def power_size_table(n: int):
    rng = np.random.default_rng(2000 + n)
    X = np.stack([np.exp(rng.normal(size=n)), 3.0 * rng.normal(size=n) + 0.5], 1).astype(np.float32)
    y = np.exp(0.8 * rng.normal(size=n) + 0.2).astype(np.float32)
    return X, y


def power_corner_columns() -> dict:
    n = POWER_CORNER_N
    rng = np.random.default_rng(77)
    u = rng.uniform(size=n)
    hi = 30.0 * u ** (1.0 / 12.0)
    holes = np.exp(0.7 * rng.normal(size=n))
    holes[::9] = np.nan
    holes[4::31] = np.inf
    holes[7::37] = -np.inf
    two = np.where(rng.uniform(size=n) < 0.35, 1.5, -0.25)
    out = rng.normal(size=n)
    out[17] = 1e6
    cols = {"clamp_hi": hi, "clamp_lo": -hi, "constant": np.full(n, 2.5), "all_nan": np.full(n, np.nan),
            "holes": holes, "two_values": two, "outlier": out}
    return {k: v.astype(np.float32) for k, v in cols.items()}


def power_corner_table():
    c = power_corner_columns()
    X = np.stack([c[name] for name, _ in POWER_CORNER_COLUMNS], 1)
    y = np.random.default_rng(78).normal(size=POWER_CORNER_N).astype(np.float32)
    return X, y


def target_table(column: str):
    """An ensemble fit whose target is one of the corner columns; one plain feature (no SVD)."""
    y = power_corner_columns()[column]
    X = np.random.default_rng(79).normal(size=(POWER_CORNER_N, 1)).astype(np.float32)
    return X, y


def power_queries(F: int) -> np.ndarray:
    """Query rows of a power case: both signs and magnitudes beyond the train range, +-0, values
    that vanish against 1, NaN and +-inf (pass through), the same in every column."""
    rng = np.random.default_rng(80)
    v = np.concatenate([3.0 * rng.normal(size=12), [0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 37.5, -37.5,
                                                     np.nan, np.inf, -np.inf]])
    return np.repeat(v[:, None], F, 1).astype(np.float32)


def finite64(col) -> np.ndarray:
    x = np.asarray(col, dtype=np.float32).astype(np.float64)
    return x[np.isfinite(x)]


def llf_bracket_spread(col):
    """(lambda of the oracle, spread of its likelihood over lambda +- k * 1e-9, k = 0..8)."""
    x = finite64(col)
    lam = po.yj_fit(x)
    f = [po.yj_neg_llf(x, lam + k * 1e-9) for k in range(-8, 9)]
    return lam, float(max(f) - min(f))


def llf_margin(col):
    """Criterion (b)'s margin: (oracle lambda, bracket spread, LLF_FACTOR x the spread) -- the spread
    taken as at least one float64 spacing of the likelihood, below which it cannot be told from 0."""
    x = finite64(col)
    lam, spread = llf_bracket_spread(col)
    return lam, spread, LLF_FACTOR * max(spread, float(np.spacing(abs(po.yj_neg_llf(x, lam)))))


def llf_excess(col, lam: float) -> float:
    x = finite64(col)
    return float(po.yj_neg_llf(x, lam) - po.yj_neg_llf(x, po.yj_fit(x)))


def llf_curvature(col):
    x = finite64(col)
    lam = po.yj_fit(x)
    f0 = po.yj_neg_llf(x, lam)
    return float(po.yj_neg_llf(x, lam - 1e-4) - f0), float(po.yj_neg_llf(x, lam + 1e-4) - f0)


def recover_lambda(col, dcol, lam0: float) -> float:
    """lambda* = the lambda whose ``power_transform_vec(col, .)`` fits the transformed column dcol
    best (relative least squares over the finite entries, Gauss-Newton from lam0 in float64).
    dcol carries the float32 rounding of n values, so lambda* is good to about
    2^-24 / (sqrt(n distinct) * log1p|x|): ~1e-9 at n = 300."""
    x32 = np.asarray(col, dtype=np.float32)
    fin = np.isfinite(x32)
    x = x32[fin].astype(np.float64)
    d = np.asarray(dcol, dtype=np.float32)[fin].astype(np.float64)
    w = np.where(d != 0.0, 1.0 / np.maximum(np.abs(d), 1e-300), 0.0)
    lam, h = float(lam0), 1e-6
    for _ in range(8):
        g = (po.yeo_johnson(x, lam + h) - po.yeo_johnson(x, lam - h)) / (2 * h) * w
        r = (po.yeo_johnson(x, lam) - d) * w
        den = float(g @ g)
        if den == 0.0 or not np.isfinite(den):
            break
        lam -= float(r @ g) / den
    return lam


def ulps32(a, b) -> np.ndarray:
    """|a - b| in units of the float32 spacing at the larger magnitude (0 where both are equal,
    non-finite entries included)."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))


# ============================================================================ 3. fingerprint cases
# (id, F, n, duplicates): "straddle" = row 3 again at rows 60..67 (across the first 64-row batch);
# "run80" = row 5 again at rows 100..179; "stride80" = one row at rows 0, 5, ..., 395;
# "tail20" = row 0 again as the last 20 rows
FINGERPRINT_CASES = (
    ("fp-F1", 1, 130, "straddle"),
    ("fp-F6", 6, 130, "straddle"),
    ("fp-F7", 7, 130, "straddle"),
    ("fp-F8", 8, 130, "straddle"),
    ("fp-F14", 14, 130, "straddle"),
    ("fp-F15", 15, 130, "straddle"),
    ("fp-F16", 16, 130, "straddle"),
    ("fp-run80", 4, 400, "run80"),
    ("fp-stride80", 4, 400, "stride80"),
    ("fp-n4096", 4, 4096, "tail20"),
    ("fp-n4097", 4, 4097, "tail20"),
)
FP_QUERY_ROWS = 12


def duplicate_rows(n: int, dup: str):
    """(source row, rows that repeat it)."""
    if dup == "straddle":
        return 3, np.arange(60, 68)
    if dup == "run80":
        return 5, np.arange(100, 180)
    if dup == "stride80":
        return 0, np.arange(5, 400, 5)
    if dup == "tail20":
        return 0, np.arange(n - 20, n)
    raise KeyError(dup)


def fingerprint_table(F: int, n: int, dup: str):
    """(X, y, Xq): Xq row 0 copies the duplicated train row, row 1 another train row."""
    rng = np.random.default_rng(3000 + 17 * F + n)
    X = rng.normal(size=(n, F)).astype(np.float32)
    src, rows = duplicate_rows(n, dup)
    X[rows] = X[src]
    y = (X[:, 0] + 0.2 * rng.normal(size=n)).astype(np.float32)
    Xq = rng.normal(size=(FP_QUERY_ROWS, F)).astype(np.float32)
    Xq[0] = X[src]
    Xq[1] = X[n - 1 if dup != "tail20" else 1]
    return X, y, Xq


def sha256_blocks(F: int) -> int:
    """64-byte blocks of the padded message of an F-feature row (8F bytes + 0x80 + 8 length bytes)."""
    return (8 * F + 1 + 8 + 63) // 64


# ============================================================================ 4. SVD cases
SVD_CASES = (("svd-const-col", 60, 4),)
SVD_GAP_MIN = 1e-6


def svd_table(n: int, F: int):
    rng = np.random.default_rng(4000 + n)
    z = rng.normal(size=(n, 2))
    X = (z @ rng.normal(size=(2, F)) + 0.4 * rng.normal(size=(n, F)))
    X[:, 2] = -1.25                                    # the constant raw column
    y = (z[:, 0] + 0.1 * rng.normal(size=n)).astype(np.float32)
    Xq = rng.normal(size=(9, F))
    Xq[:, 2] = np.array([-1.25, -1.25, 0.0, 3.0, -1.25, -1.25, -1.25, 1.0, -1.25])
    Xq[5, 1] = np.nan                                  # one NaN feature: NaN SVD columns
    Xq[6] = X[4]                                       # a train row
    return X.astype(np.float32), y, Xq.astype(np.float32)


def gram_gaps(Z: np.ndarray, k: int) -> np.ndarray:
    """Relative gaps between consecutive eigenvalues 1..k+1 of the oracle's scaled Gram matrix."""
    Z = np.asarray(Z, dtype=np.float64)
    mu = Z.mean(0)
    scale = np.sqrt(((Z - mu) ** 2).mean(0))
    scale = np.where(scale < 10 * np.finfo(np.float64).eps, 1.0, scale)
    Y = Z / scale
    w = np.sort(np.linalg.eigvalsh(Y.T @ Y))[::-1]
    return (w[:k] - w[1:k + 1]) / w[0]


# ============================================================================ 5. end to end
# (id, mode, table): degenerate tables through predict_logits against OracleTabPFN(emulate_bf16=True).
# The all-NaN column runs under "quantile+power": the oracle defines no imputation before the SVD.
E2E_CASES = (
    ("e2e-constant-col", "ensemble", "constant"),
    ("e2e-all-nan-col", "quantile+power", "all_nan"),
    ("e2e-n2", "ensemble", "n2"),
    ("e2e-F1", "ensemble", "F1"),
)
E2E_TV_MAX = 0.02


def e2e_table(kind: str):
    rng = np.random.default_rng(5000 + len(kind))
    n, F, N = (2, 2, 6) if kind == "n2" else (48, 1 if kind == "F1" else 3, 10)
    X = rng.normal(size=(n, F)).astype(np.float32)
    Xq = rng.normal(size=(N, F)).astype(np.float32)
    if kind == "constant":
        X[:, 1] = 0.75
        Xq[:, 1] = 0.75
        Xq[3, 1] = 2.0
    if kind == "all_nan":
        X[:, 1] = np.nan
        Xq[:, 1] = np.nan
        Xq[3, 1] = 1.0
    y = (X[:, 0] + 0.3 * rng.normal(size=n)).astype(np.float32)
    return X, y, Xq


# ============================================================================ the oracle's views
class OracleViews:
    """The views table [rows, 3F + k + E] of a fit, block by block, from the oracle's functions."""

    def __init__(self, X: np.ndarray, mode: str, seed: int = SEED, classifier: bool = False):
        self.X = np.asarray(X, dtype=np.float32)
        self.n, self.F = self.X.shape
        self.mode = mode
        div = po.QUANTILE_DIV_COARSE if classifier and mode == "ensemble" else po.QUANTILE_DIV
        self.sub = po.quantile_subsample(self.n, seed)
        self.qtab = [po.quantile_fit(self.X[:, j], self.n, div, self.sub) for j in range(self.F)]
        self.k = po.svd_components(self.n, self.F) if mode == "ensemble" else 0
        self.svd = None
        if self.k:
            self.Z = np.concatenate([self.X, self.quant(self.X)], 1).astype(np.float64)
            self.svd = po.svd_fit(self.Z, self.k)
        self.salts = [po.fingerprint_salt(seed, e) for e in range(E)]
        F, k = self.F, self.k
        self.q_off, self.s_off, self.p_off, self.fp_off, self.Vw = F, 2 * F, 2 * F + k, 3 * F + k, 3 * F + k + E

    def quant(self, R: np.ndarray) -> np.ndarray:
        R = np.asarray(R, dtype=np.float32)
        return np.stack([po.quantile_transform_vec(R[:, j], self.qtab[j]) for j in range(self.F)], 1)

    def svd_cols(self, R: np.ndarray) -> np.ndarray:
        R = np.asarray(R, dtype=np.float32)
        with np.errstate(all="ignore"):
            return po.svd_transform(np.concatenate([R, self.quant(R)], 1).astype(np.float64), *self.svd)

    def fingerprints(self, R: np.ndarray, train: bool) -> np.ndarray:
        return np.stack([po.fingerprint(R, s, train) for s in self.salts], 1)
