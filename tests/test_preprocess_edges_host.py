"""CPU: the cases of tests/test_gpu_preprocess_edges.py are fair (tests/preprocess_edges_ref.py).

* The case tables are literal and counted; every case reaches the branch it is named for (quantile
  counts, sort padding, the subsample switch, SHA-256 block counts, duplicate depth).
* The oracle is sklearn 1.7.2's on the new inputs: QuantileTransformer on the tiny, tied, constant,
  one-finite-value and subsampled columns and on every query value; PowerTransformer on the corner
  columns (its Brent search is unbounded: on the clamp columns it runs past +-6, where the
  oracle's and the device's fixed search on [-6, 6] stop at the end of the grid).
* Power fit: clamp lambdas, likelihood slopes and curvatures, the bracket spread that sets the
  margin of criterion (b) -- printed per column -- and a float64 model of the device's own formula
  (shifted sums of expm1(a L) / a in 512 strided partial sums) that passes criteria (a) and (b):
  the bars can be met.
* Every SVD that is compared has a relative eigenvalue gap >= 1e-6.
"""
import hashlib

import numpy as np
import pytest

import preprocess_edges_ref as pr
from oracle import preprocess_oracle as po


# ------------------------------------------------------------------ the tables are literal
def test_case_tables_are_counted():
    assert len(pr.QUANTILE_CASES) == 18 and len(pr.POWER_SIZE_CASES) == 4 and len(pr.POWER_CORNER_COLUMNS) == 7
    assert len(pr.POWER_TARGET_CASES) == 5 and len(pr.FINGERPRINT_CASES) == 11 and len(pr.SVD_CASES) == 1
    assert len(pr.E2E_CASES) == 4
    assert [c[2] for c in pr.QUANTILE_CASES if c[1] == "quantile"] == [2, 3, 9, 10, 11, 15, 255, 256, 257, 320, 325,
                                                                        1285, 10_000, 10_001]
    assert [c[1] for c in pr.POWER_SIZE_CASES] == [pr.PF_REGS_MAX, pr.PF_REGS_MAX + 1, pr.QT_SORT_MAX,
                                                   pr.QT_SORT_MAX + 1]
    assert [c[1] for c in pr.FINGERPRINT_CASES[:7]] == [1, 6, 7, 8, 14, 15, 16]
    ids = [c[0] for t in (pr.QUANTILE_CASES, pr.POWER_SIZE_CASES, pr.POWER_TARGET_CASES, pr.FINGERPRINT_CASES,
                          pr.SVD_CASES, pr.E2E_CASES) for c in t] + [pr.CLASSIFIER_CASE[0]]
    assert len(set(ids)) == len(ids)
    # eight estimators: every pipeline of every mode occurs
    assert {t for t, _ in po.estimator_configs(po.MODE_ENSEMBLE, pr.E)} == {po.T_QSVD, po.T_PFP}
    assert set(po.estimator_configs(po.MODE_ENSEMBLE, pr.E)) == {(po.T_QSVD, False), (po.T_QSVD, True),
                                                                 (po.T_PFP, False), (po.T_PFP, True)}
    assert {t for t, _ in po.estimator_configs(po.MODE_QUANTILE_POWER, pr.E)} == {po.T_QUANT, po.T_POWER}
    assert {t for t, _ in po.estimator_configs(po.MODE_ENSEMBLE, pr.E, True)} == {po.T_QSVD, po.T_RFP}
    assert pr.small_cfg().n_estimators == pr.E


# ------------------------------------------------------------------ quantile cases
def test_quantile_cases_reach_their_branches():
    nq = {n: po.n_quantiles_for(n) for _, m, n, _ in pr.QUANTILE_CASES if m == "quantile"}
    assert [nq[n] for n in (2, 3, 9, 10, 11)] == [2, 2, 2, 2, 2] and nq[15] == 3      # quantile_count clamps
    assert (nq[320], nq[325]) == (64, 65)            # one | two quantiles in a lane's scan segment
    assert nq[1285] == 257                           # more than one quantile per thread
    assert po.quantile_subsample(10_000, pr.SEED) is None and po.quantile_subsample(10_001, pr.SEED).size == 10_000
    assert po.n_quantiles_for(pr.CLASSIFIER_CASE[2], po.QUANTILE_DIV_COARSE) == 33
    for _, _, n, cols in pr.QUANTILE_CASES:
        X, y = pr.quantile_table(n, cols)
        assert X.shape == (n, 7 if cols == "planted" else 3) and np.isfinite(y).all()
        assert np.isfinite(X[:, :3]).all() and np.ptp(X[:, 2]) == 0
        assert np.unique(X[:, 1]).size <= 5
        if n >= 255:
            assert np.unique(X[:, 1]).size == 5 and np.unique(X[:, 0]).size >= n - 2   # float32 may collide
    X, _ = pr.quantile_table(257, "planted")        # the sort pads 255 | 256 | 257 and 128 | 129 values
    assert tuple(np.isfinite(X[:, 3:]).sum(0)) == pr.PLANTED_FINITE == (0, 1, 128, 129)
    assert np.isnan(X[:, 3:]).any() and np.isposinf(X[:, 3:]).any() and np.isneginf(X[:, 3:]).any()
    ov = pr.OracleViews(X, "quantile")
    assert ov.qtab[3].size == 0 and np.ptp(ov.qtab[4]) == 0 and ov.qtab[4].size == 51
    # the ties column repeats quantiles, and the query values hit one
    Xq = pr.quantile_queries(ov.qtab)
    assert Xq.shape == (pr.QUERY_ROWS, 7)
    q = ov.qtab[1]
    assert (np.diff(q) == 0).any() and Xq[6, 1] in q and (q == Xq[6, 1]).sum() > 1
    assert Xq[0, 1] == 0.0 and np.signbit(Xq[17, 1]) and Xq[17, 1] == q[0]    # -0.0 on the x == q[0] override
    for j in (0, 1, 2, 4, 5, 6):
        q = ov.qtab[j]
        assert Xq[0, j] == q[0] and Xq[1, j] == q[-1] and Xq[2, j] < q[0] < Xq[3, j] and Xq[4, j] < q[-1] < Xq[5, j]


def _sk_quantile(col, n, div, seed, xq):
    from sklearn.preprocessing import QuantileTransformer
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        qt = QuantileTransformer(output_distribution="uniform", n_quantiles=max(n // div, 2), random_state=seed)
        qt.fit(np.where(np.isfinite(col), col, np.nan).astype(np.float64)[:, None])
        ok = ~np.isinf(xq)                           # sklearn's input check refuses inf; NaN passes through
        out = np.full(xq.shape, np.nan)
        out[ok] = qt.transform(xq[ok, None].astype(np.float64))[:, 0]
    return qt, out, ok


@pytest.mark.parametrize("cid,mode,n,cols", [c for c in pr.QUANTILE_CASES if c[1] == "quantile"] + [pr.CLASSIFIER_CASE],
                         ids=lambda v: v if isinstance(v, str) and "-" in v else None)
def test_quantile_oracle_is_sklearn_on_the_cases(cid, mode, n, cols):
    """Quantile tables (rtol 1e-7, as test_quantile_fit_with_subsample_matches_sklearn) and the
    transform of the train column and of every finite or NaN query value (atol 1e-6)."""
    X, _ = pr.quantile_table(n, cols)
    classifier = cid == pr.CLASSIFIER_CASE[0]
    div = po.QUANTILE_DIV_COARSE if classifier else po.QUANTILE_DIV
    ov = pr.OracleViews(X, mode, classifier=classifier)
    Xq = pr.quantile_queries(ov.qtab)
    for j in range(X.shape[1]):
        if not np.isfinite(X[:, j]).any():
            assert ov.qtab[j].size == 0              # sklearn: an all-NaN table; the engine passes the column through
            np.testing.assert_array_equal(ov.quant(Xq)[:, j], Xq[:, j])
            continue
        x = np.concatenate([X[:, j], Xq[:, j]])
        qt, ref, ok = _sk_quantile(X[:, j], n, div, pr.SEED, x)
        q = ov.qtab[j]
        assert q.size == qt.n_quantiles_
        np.testing.assert_allclose(q, qt.quantiles_[:, 0], rtol=1e-7, atol=1e-11)
        got = po.quantile_transform_vec(x, q)
        np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=1e-6, equal_nan=True)
        np.testing.assert_array_equal(got[~ok], x[~ok])           # +-inf pass through
        np.testing.assert_array_equal(po.quantile_transform(x[n:], q), got[n:])


# ------------------------------------------------------------------ power cases
def _power_columns():
    """Every column whose lambda is compared: (name, column, kind)."""
    for cid, n in pr.POWER_SIZE_CASES:
        X, y = pr.power_size_table(n)
        for j, name in enumerate(pr.POWER_SIZE_COLUMNS):
            yield f"{cid}/{name}", X[:, j], "fit"
        yield f"{cid}/target", y, "fit"
    cols = pr.power_corner_columns()
    for name, kind in pr.POWER_CORNER_COLUMNS:
        yield f"corner/{name}", cols[name], kind


def test_power_corner_lambdas_and_target_cases():
    cols = pr.power_corner_columns()
    assert list(cols) == [n for n, _ in pr.POWER_CORNER_COLUMNS]
    for sign, name in ((1.0, "clamp_hi"), (-1.0, "clamp_lo")):
        x = pr.finite64(cols[name])
        lam = po.yj_fit(x)
        assert abs(lam - sign * 6.0) <= pr.CLAMP_BRACKET, lam
        slope = po.yj_neg_llf(x, sign * (6.0 - 1e-4)) - po.yj_neg_llf(x, sign * 6.0)
        print(f"{name}: lambda {lam:+.10f}, likelihood slope {slope:.2e} per 1e-4 at the clamp")
        assert slope >= 5e-5                         # the grid's best node is the last one, by a wide margin
    assert po.yj_fit(cols["constant"]) == 1.0 and po.yj_fit(cols["all_nan"]) == 1.0
    h = cols["holes"]
    assert np.isnan(h).any() and np.isposinf(h).any() and np.isneginf(h).any() and np.isfinite(h).sum() > 200
    assert np.unique(cols["two_values"]).size == 2 and cols["outlier"].max() == np.float32(1e6)
    for cid, col, kind in pr.POWER_TARGET_CASES:
        assert np.isfinite(cols[col]).all() and dict(pr.POWER_CORNER_COLUMNS)[col] == kind
        X, y = pr.target_table(col)
        assert X.shape == (pr.POWER_CORNER_N, 1) and po.svd_components(*X.shape) == 0


def _device_model_lambda(x):
    """float64 model of k_power_fit's search: the transform as expm1(a L) / a with L = log1p|x|,
    sums of the values shifted by the minimum's transform in 512 strided partials."""
    L, pos = np.log1p(np.abs(x)), x >= 0
    S, n, imin = float((np.sign(x) * L).sum()), x.size, int(np.argmin(x))

    def nll(lam):
        t = np.empty_like(L)
        t[pos] = L[pos] if abs(lam) < po._EPS1 else np.expm1(lam * L[pos]) / lam
        t[~pos] = -L[~pos] if not abs(lam - 2.0) > po._EPS1 else -np.expm1((2.0 - lam) * L[~pos]) / (2.0 - lam)
        d = np.zeros(-(-n // 512) * 512)
        d[:n] = t - t[imin]
        d = d.reshape(-1, 512)
        s1, s2 = d.sum(0).sum(), (d * d).sum(0).sum()
        var = max(s2 - s1 * s1 / n, 0.0) / n
        return np.inf if not var >= np.finfo(np.float64).tiny else -(-n / 2.0 * np.log(var) + (lam - 1.0) * S)

    grid = po.YJ_GRID_LO + po.YJ_GRID_STEP * np.arange(po.YJ_GRID_N)
    i = int(np.argmin([nll(g) for g in grid]))
    a, b = grid[max(i - 1, 0)], grid[min(i + 1, po.YJ_GRID_N - 1)]
    r = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - r * (b - a), a + r * (b - a)
    fc, fd = nll(c), nll(d)
    for _ in range(po.YJ_GOLDEN_STEPS):
        if fc <= fd:
            b, d, fd = d, c, fc
            c = b - r * (b - a)
            fc = nll(c)
        else:
            a, c, fc = c, d, fd
            d = a + r * (b - a)
            fd = nll(d)
    return 0.5 * (a + b)


@pytest.mark.parametrize("name,col,kind", list(_power_columns()), ids=[c[0] for c in _power_columns()])
def test_power_columns_are_curved_and_the_bars_can_be_met(name, col, kind):
    if kind == "identity":
        assert po.yj_fit(col) == 1.0
        return
    x = pr.finite64(col)
    lam, spread, margin = pr.llf_margin(col)
    if kind == "fit":
        lo, hi = pr.llf_curvature(col)
        print(f"{name}: lambda {lam:+.9f}, curvature {lo:.2e} / {hi:.2e} per 1e-4, bracket spread {spread:.2e} "
              f"x {pr.LLF_FACTOR:g} = margin {margin:.2e}")
        assert min(lo, hi) >= pr.LLF_CURVATURE_MIN and spread > 0.0
    # the model of the device's formula meets (a) and (b) through the same recovery the GPU test uses
    lam_dev = _device_model_lambda(x)
    dcol = po.power_transform_vec(col, lam_dev)
    lam_star = pr.recover_lambda(col, dcol, lam)
    print(f"{name}: device model lambda {lam_dev:+.10f}, recovered {lam_star - lam_dev:+.1e} away")
    assert pr.ulps32(dcol, po.power_transform_vec(col, lam_star)).max() <= 1.0
    if kind == "fit":
        assert abs(lam_star - lam_dev) <= 1e-7
        assert pr.llf_excess(col, lam_star) <= margin and pr.llf_excess(col, lam_dev) <= margin
        # and the bar sees a lambda that is off by 1e-4: at least 1e-7, against margins below 1e-9
        assert margin < 0.01 * pr.LLF_CURVATURE_MIN
    else:
        sign = 1.0 if kind == "clamp+" else -1.0
        assert abs(lam_star - sign * 6.0) <= pr.CLAMP_BRACKET and abs(lam_star - lam_dev) <= 2.5e-9


def test_power_oracle_is_sklearn_on_the_corner_columns():
    """PowerTransformer (Brent, unbounded): interior optima as test_power_fit_matches_sklearn; on the
    clamp columns sklearn's lambda lies beyond the grid's end, the side the fixed search stops at;
    the transform itself at sklearn's lambda."""
    import warnings

    from sklearn.preprocessing import PowerTransformer

    cols = pr.power_corner_columns()
    for name, kind in pr.POWER_CORNER_COLUMNS:
        if kind == "identity":
            continue
        col = cols[name][np.isfinite(cols[name])]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pt = PowerTransformer(method="yeo-johnson", standardize=False).fit(col[:, None].astype(np.float64))
            want = pt.transform(col[:, None].astype(np.float64))[:, 0]
        ref, lam, x = float(pt.lambdas_[0]), po.yj_fit(col), col.astype(np.float64)
        print(f"{name}: oracle lambda {lam:+.6f}, sklearn {ref:+.6f}")
        if kind == "fit":
            assert po.yj_neg_llf(x, lam) <= po.yj_neg_llf(x, ref) + 1e-6 * abs(po.yj_neg_llf(x, ref))
            assert abs(lam - ref) <= 2e-3, (lam, ref)
        else:
            assert ref * np.sign(lam) > 6.0
        np.testing.assert_allclose(po.yeo_johnson(x, ref), want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ fingerprint cases
def test_fingerprint_cases_reach_every_padding_shape_and_depth():
    assert [pr.sha256_blocks(F) for F in (1, 6, 7, 8, 14, 15, 16)] == [1, 1, 2, 2, 2, 3, 3]
    # F = 7 and F = 15: the data ends on a block's 56th byte, so 0x80 and the length move apart;
    # F = 8 and F = 16: the data fills a block and the 0x80 word opens the next one
    assert (8 * 7) % 64 == 56 and (8 * 15) % 64 == 56 and (8 * 8) % 64 == 0 and (8 * 16) % 64 == 0
    for cid, F, n, dup in pr.FINGERPRINT_CASES:
        X, y, Xq = pr.fingerprint_table(F, n, dup)
        src, rows = pr.duplicate_rows(n, dup)
        assert X.shape == (n, F) and (X[rows] == X[src]).all() and np.array_equal(Xq[0], X[src])
        salt = po.fingerprint_salt(pr.SEED, 0)
        fp = po.fingerprint(X, salt, train=True)
        hv = np.round(fp.astype(np.float64) * po.FP_BUCKETS).astype(int)
        assert np.unique(hv).size == n
        want = int(hashlib.sha256((X[1].astype(np.float64) + salt).tobytes()).hexdigest(), 16) % po.FP_BUCKETS
        assert hv[1] == want or dup == "tail20"      # row 1 is no duplicate of an earlier row
        # adds the last duplicate needs: every earlier copy took one
        last, taken, add = int(rows[-1]), set(hv[:rows[-1]].tolist()), 0
        while po.row_hash(X[last].astype(np.float64) + float(salt) + float(add)) in taken:
            add += 1
        assert hv[last] == po.row_hash(X[last].astype(np.float64) + float(salt) + float(add))
        if dup == "straddle":
            assert rows[0] < 64 <= rows[-1] and add >= rows.size
        if dup in ("run80", "stride80"):
            assert add >= 64 + pr.FP_MIN             # past the first round of 64 fresh hashes
        if dup == "stride80":
            assert (np.diff(rows) == 5).all() and rows.size + 1 == 80
        if dup == "tail20":
            assert add >= 20 and (n - pr.FP_ONE_WAVE_MAX) in (0, 1)
        # the query copy of a train row keeps the un-rehashed hash
        assert po.fingerprint(Xq[:1], salt, train=False)[0] == fp[src]


# ------------------------------------------------------------------ SVD cases
def test_compared_svds_are_determined():
    for cid, n, F in pr.SVD_CASES:
        X, y, Xq = pr.svd_table(n, F)
        assert np.ptp(X[:, 2]) == 0 and np.isnan(Xq).sum() == 1
        ov = pr.OracleViews(X, "ensemble")
        assert ov.k == 2 and np.ptp(ov.quant(X)[:, 2]) == 0        # the quantile column is constant too
        assert ov.svd[0][2] == 1.0 and ov.svd[0][F + 2] == 1.0       # scale 0 -> 1
        gaps = pr.gram_gaps(ov.Z, ov.k)
        print(f"{cid}: relative eigenvalue gaps {gaps}")
        assert gaps.min() >= pr.SVD_GAP_MIN
        s = ov.svd_cols(Xq)
        assert np.isnan(s[5]).all() and np.isfinite(np.delete(s, 5, 0)).all()
    for cid, mode, n, cols in pr.QUANTILE_CASES + (pr.CLASSIFIER_CASE,):
        if mode != "ensemble":
            continue
        X, _ = pr.quantile_table(n, cols)
        ov = pr.OracleViews(X, mode, classifier=cid == pr.CLASSIFIER_CASE[0])
        gaps = pr.gram_gaps(ov.Z, ov.k)
        print(f"{cid}: k = {ov.k}, relative eigenvalue gaps {gaps}")
        assert ov.k == 1 and gaps.min() >= pr.SVD_GAP_MIN


# ------------------------------------------------------------------ end-to-end tables
@pytest.mark.parametrize("cid,mode,kind", pr.E2E_CASES, ids=[c[0] for c in pr.E2E_CASES])
def test_oracle_predicts_on_the_degenerate_tables(cid, mode, kind):
    from npe_pfn.weights import synthetic_weights
    from oracle.tabpfn_oracle import OracleTabPFN

    cfg = pr.small_cfg()
    X, y, Xq = pr.e2e_table(kind)
    orc = OracleTabPFN(synthetic_weights(cfg, seed=0), cfg.n_estimators, cfg.softmax_temperature, seed=pr.SEED,
                       emulate_bf16=True, preprocessing=pr.MODES[mode])
    st = orc.fit(X, y)
    p = orc.predict_probs(Xq)
    assert p.shape == (Xq.shape[0], cfg.n_bars) and np.isfinite(p).all()
    np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-4)
    if kind in ("constant", "all_nan"):             # the degenerate column is unused: its group scale shrinks
        assert any((es.gscale > 1.0).any() for es in st.estimators)
    if kind == "F1":
        assert st.svd is None and [es.n_feat for es in st.estimators] == [3] * 4 + [2] * 4
