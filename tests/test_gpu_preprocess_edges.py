"""The preprocessing kernels at every size, path and column edge, against the sklearn-pinned oracle.

k_quantile_fit, k_qt_subsample, k_power_fit, k_views, k_views_svd, k_views_fp, k_fp_train_hash,
k_fp_train_resolve and k_col_stats: the preprocessed table read back through ``Engine.debug_views``
(train rows straight after the fit, query rows straight after the predict) against
oracle/preprocess_oracle.py.  The cases are the literal tables of tests/preprocess_edges_ref.py;
tests/test_preprocess_edges_host.py proves on the CPU that they are fair.  Every fit runs on
``ModelConfig(n_layers=1, n_bars=250)``: preprocessing plus one cheap forward.

Branch -> case:

* k_power_fit storage forms: registers | LDS | global memory -- ``p-n2048`` | ``p-n2049``,
  ``p-n16384`` | ``p-n16385`` (feature columns under "quantile+power", the target block
  ``blockIdx.x == F`` under "ensemble").
* Lambda search corners: best node 12 / 0 -- ``clamp_hi`` / ``clamp_lo``; lambda = 1 -- ``constant``,
  ``all_nan``; NaN / inf entries skipped -- ``holes``; ``two_values``, ``outlier``; the same columns
  as the target (``ylam``, ``ystats[3:6]``) -- ``t-clamp_hi`` ... ``t-outlier``.
* SHA-256 padding: one block ``fp-F1``, ``fp-F6``; two from ``fp-F7`` (0x80 and the length apart);
  0x80 opens the second block ``fp-F8``; the same again at ``fp-F14``, ``fp-F15``, ``fp-F16``.
* k_fp_train_resolve: duplicates across the first batch boundary -- the ``straddle`` rows 60..67 of
  every ``fp-F*`` case; a second round of fresh hashes in slow_row -- ``fp-run80``, ``fp-stride80``;
  the one-wave | 16-wave slow path -- ``fp-n4096`` | ``fp-n4097`` (and ``qe-n10001``: a second block
  of distinct hashes).
* k_quantile_fit: quantile_count clamps -- ``q-n2`` ... ``q-n11``, ``q-n15``; no / one finite value and
  the sort's padding at 128 | 129 and 255 | 256 | 257 values -- ``q-n255``, ``q-n256``, ``q-n257``
  (planted columns); nq = 64 | 65 -- ``q-n320`` | ``q-n325``; nq > 256 -- ``q-n1285``; the subsample
  switch -- ``q-n10000`` | ``q-n10001``; div = 10 -- ``qc-n330`` (fit_classes).
* k_views on query rows: ``query_values`` of every quantile case (both ends, nextafter around them,
  a repeated quantile, midpoints, far values, +-inf, NaN, -0.0); k_views_fp on query rows: every
  fingerprint and ensemble case.
* F = 1 under the ensemble (no SVD columns) -- ``fp-F1``, ``e2e-F1``.
* SVD with a constant column (scale 0 -> 1), a NaN query feature -- ``svd-const-col``; the ensemble
  fits ``qe-n10`` ... ``qe-n10001`` compare their one SVD column too.
* used flags and group scales of k_build_params (not readable): ``e2e-*`` at TV <= 0.02.  The
  log-probabilities of ``predict_logits`` hold -inf on bars without mass (250 bars out to +-40
  standard deviations), so "finite" is asserted as: no NaN, no +inf, every row has mass, and -inf
  only where the oracle's probability is 0 or the rounding of its float32 cdf (<= 2^-23).

Found by ``q-n256`` / ``qe-n256``: k_quantile_fit's percentile index fraction g = (cnt - 1) * p -
floor(.) was contracted into one FMA, which gave g = 2.8e-15 where numpy's rounded product gives 0;
at a tie boundary of the five-valued column (52 zeros of 256 rows, p = 0.2) the quantile came out
2.8e-15 instead of 0, the run of repeated quantiles was one shorter, and nextafter(q[0]) mapped to
0.18 instead of sklearn's 0.20.  The kernel now rounds as numpy does.

Tolerances: raw columns exact; quantile columns atol 1e-6, rtol 0; SVD columns rtol 1e-4, atol
1e-4; fingerprints bit-exact.  Power columns: lambda* is recovered from the device's train and
query column by fitting the oracle's own transform to it (``recover_lambda``), then (a) the column
equals ``power_transform_vec(x, lambda*)`` to 1 float32 ulp and (b) lambda* is as likely as the
oracle's lambda to within LLF_FACTOR = 32 times the spread of the oracle's own likelihood over its
final bracket (the factor's reasoning: preprocess_edges_ref.LLF_FACTOR); at a clamp (b) is
|lambda* -+ 6| <= 1e-8.  Bracket spreads measured on the CPU (host test output), margin = 32 x:

    p-n2048   lognormal 9.1e-13  normal 9.1e-13  target 1.4e-12
    p-n2049   lognormal 4.5e-13  normal 9.1e-13  target 9.1e-13
    p-n16384  lognormal 7.3e-12  normal 7.3e-12  target 3.6e-12
    p-n16385  lognormal 7.3e-12  normal 1.5e-11  target 7.3e-12
    corner    holes 1.1e-13  two_values 1.1e-13  outlier 1.7e-13

against likelihood rises of 1.4e-7 ... 1.8e-4 for a lambda that is off by 1e-4.
"""
import numpy as np
import pytest
import torch

import preprocess_edges_ref as pr
from oracle import preprocess_oracle as po

pytestmark = pytest.mark.gpu

CFG = pr.small_cfg()
DEV = torch.device("cuda", 0)
_ids = lambda cases: [c[0] for c in cases]  # noqa: E731


@pytest.fixture(scope="module")
def weights():
    from npe_pfn.weights import synthetic_weights

    return synthetic_weights(CFG, seed=0)


def _fit_and_query(weights, mode, X, y, Xq, Vw, n_classes=0):
    """(train views, query views, engine): one fit, one predict."""
    from npe_pfn.engine import Engine

    eng = Engine(CFG, weights, device=DEV, random_state=pr.SEED, preprocessing=mode)
    if n_classes:
        eng.fit_classes(torch.from_numpy(X), torch.from_numpy(y), n_classes)
    else:
        eng.fit(torch.from_numpy(X), torch.from_numpy(y))
    tv = eng.debug_views(X.shape[0], Vw)
    assert tv.shape == (X.shape[0], Vw)
    out = eng.predict_proba(torch.from_numpy(Xq)) if n_classes else eng.predict_logits(torch.from_numpy(Xq))
    qv = eng.debug_views(Xq.shape[0], Vw)
    assert qv.shape == (Xq.shape[0], Vw)
    return tv, qv, eng, out


def _check_raw_and_quantile(ov, views, R):
    F = ov.F
    np.testing.assert_array_equal(views[:, :F], R)
    ref = ov.quant(R)
    got = views[:, ov.q_off:ov.q_off + F]
    bad = ~np.isfinite(R)
    np.testing.assert_array_equal(got[bad], R[bad])                       # non-finite entries pass through
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6, equal_nan=True)


def _check_svd(ov, views, R):
    ref = ov.svd_cols(R)
    got = views[:, ov.s_off:ov.s_off + ov.k]
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-4, atol=1e-4)


def _check_fingerprints(ov, views, R, train):
    """Every estimator's column; past 5000 rows the first and the last estimator's (hashlib's time)."""
    est = list(range(pr.E)) if R.shape[0] <= 5000 else [0, pr.E - 1]
    ref = np.stack([po.fingerprint(R, ov.salts[e], train) for e in est], 1)
    np.testing.assert_array_equal(views[:, [ov.fp_off + e for e in est]], ref)


# ============================================================================ 1. quantile
@pytest.mark.parametrize("cid,mode,n,cols", pr.QUANTILE_CASES, ids=_ids(pr.QUANTILE_CASES))
def test_quantile_fit_and_transform(weights, cid, mode, n, cols):
    X, y = pr.quantile_table(n, cols)
    ov = pr.OracleViews(X, mode)
    Xq = pr.quantile_queries(ov.qtab)
    tv, qv, _, _ = _fit_and_query(weights, mode, X, y, Xq, ov.Vw)
    _check_raw_and_quantile(ov, tv, X)
    _check_raw_and_quantile(ov, qv, Xq)
    if mode == "ensemble":
        assert ov.k == 1
        _check_svd(ov, tv, X)
        _check_svd(ov, qv, Xq)
        _check_fingerprints(ov, tv, X, True)
        _check_fingerprints(ov, qv, Xq, False)


def test_classifier_coarse_quantile_table(weights):
    cid, mode, n, cols = pr.CLASSIFIER_CASE
    X, _ = pr.quantile_table(n, cols)
    y = np.random.default_rng(6).integers(0, pr.CLASSIFIER_K, size=n).astype(np.float32)
    ov = pr.OracleViews(X, mode, classifier=True)
    assert ov.qtab[0].size == n // po.QUANTILE_DIV_COARSE
    Xq = pr.quantile_queries(ov.qtab)
    tv, qv, _, proba = _fit_and_query(weights, mode, X, y, Xq, ov.Vw, n_classes=pr.CLASSIFIER_K)
    _check_raw_and_quantile(ov, tv, X)
    _check_raw_and_quantile(ov, qv, Xq)
    _check_svd(ov, tv, X)
    _check_fingerprints(ov, tv, X, True)
    _check_fingerprints(ov, qv, Xq, False)
    assert torch.isfinite(proba).all()


# ============================================================================ 2. power
def _check_power_column(name, kind, x, xq, d, dq):
    """Criteria (a) and (b) of the module docstring for one column (train x -> d, query xq -> dq)."""
    bad, badq = ~np.isfinite(x), ~np.isfinite(xq)
    np.testing.assert_array_equal(d[bad], x[bad])
    np.testing.assert_array_equal(dq[badq], xq[badq])
    if kind == "identity":
        lam_star = 1.0
    else:
        lam, spread, margin = pr.llf_margin(x)
        lam_star = pr.recover_lambda(np.concatenate([x, xq]), np.concatenate([d, dq]), lam)
        excess = pr.llf_excess(x, lam_star)
        print(f"{name}: oracle lambda {lam:+.10f}, device lambda* {lam_star:+.10f} ({lam_star - lam:+.1e}), "
              f"likelihood excess {excess:+.2e} (margin {margin:.2e})")
    u, uq = pr.ulps32(d, po.power_transform_vec(x, lam_star)), pr.ulps32(dq, po.power_transform_vec(xq, lam_star))
    assert u.max() <= 1.0 and uq.max() <= 1.0, (name, u.max(), uq.max())
    if kind == "fit":
        assert excess <= margin, (name, excess, margin)
    elif kind != "identity":
        assert abs(lam_star - (6.0 if kind == "clamp+" else -6.0)) <= pr.CLAMP_BRACKET, (name, lam_star)


@pytest.mark.parametrize("cid,n", pr.POWER_SIZE_CASES, ids=_ids(pr.POWER_SIZE_CASES))
def test_power_fit_storage_forms(weights, cid, n):
    X, y = pr.power_size_table(n)
    Xq = pr.power_queries(X.shape[1])
    ov = pr.OracleViews(X, "quantile+power")
    tv, qv, _, _ = _fit_and_query(weights, "quantile+power", X, y, Xq, ov.Vw)
    _check_raw_and_quantile(ov, tv, X)
    _check_raw_and_quantile(ov, qv, Xq)
    for j, name in enumerate(pr.POWER_SIZE_COLUMNS):
        _check_power_column(f"{cid}/{name}", "fit", X[:, j], Xq[:, j], tv[:, ov.p_off + j], qv[:, ov.p_off + j])


def test_power_fit_corner_columns(weights):
    X, y = pr.power_corner_table()
    Xq = pr.power_queries(X.shape[1])
    ov = pr.OracleViews(X, "quantile+power")
    tv, qv, _, _ = _fit_and_query(weights, "quantile+power", X, y, Xq, ov.Vw)
    _check_raw_and_quantile(ov, tv, X)
    for j, (name, kind) in enumerate(pr.POWER_CORNER_COLUMNS):
        _check_power_column(f"corner/{name}", kind, X[:, j], Xq[:, j], tv[:, ov.p_off + j], qv[:, ov.p_off + j])


def _check_target(name, kind, y, eng):
    """``ylam`` by criterion (b); ``ystats`` against the statistics of y and of the float32
    ``power_transform_vec(y, ylam)``: mean and std to 1 ulp, the mean of the standardized values to
    the float32 rounding of one standardized value."""
    from oracle.tabpfn_oracle import OracleTabPFN

    t = eng.debug_target_translation()
    assert t["translated"] and list(t["ett"]) == [int(tt) for _, tt in po.estimator_configs(po.MODE_ENSEMBLE, pr.E)]
    ylam, ys = t["ylam"], t["ystats"]
    if kind == "identity":
        assert ylam == 1.0
    elif kind == "fit":
        lam, spread, margin = pr.llf_margin(y)
        excess = pr.llf_excess(y, ylam)
        print(f"{name}: oracle lambda {lam:+.10f}, ylam {ylam:+.10f} ({ylam - lam:+.1e}), likelihood excess "
              f"{excess:+.2e} (margin {margin:.2e})")
        assert excess <= margin, (name, excess, margin)
    else:
        assert abs(ylam - (6.0 if kind == "clamp+" else -6.0)) <= pr.CLAMP_BRACKET, (name, ylam)
    m, s, _, _ = OracleTabPFN._ystats(y)
    tm, ts, tz, z = OracleTabPFN._ystats(po.power_transform_vec(y, ylam))
    assert pr.ulps32([ys[0], ys[1], ys[3], ys[4]], [m, s, tm, ts]).max() <= 1.0, (name, ys, (m, s, tm, ts))
    bound = 0.0 if np.ptp(y) == 0 else 2.0 ** -23 * (float(np.abs(z).max()) + abs(tm) / ts)
    assert abs(float(ys[5]) - tz) <= bound, (name, ys[5], tz, bound)


@pytest.mark.parametrize("cid,n", pr.POWER_SIZE_CASES, ids=_ids(pr.POWER_SIZE_CASES))
def test_target_power_fit_storage_forms(weights, cid, n):
    """The target block of k_power_fit under the ensemble, and the feature blocks next to it."""
    X, y = pr.power_size_table(n)
    Xq = pr.power_queries(X.shape[1])
    ov = pr.OracleViews(X, "ensemble")
    tv, qv, eng, _ = _fit_and_query(weights, "ensemble", X, y, Xq, ov.Vw)
    _check_target(f"{cid}/target", "fit", y, eng)
    for j, name in enumerate(pr.POWER_SIZE_COLUMNS):
        _check_power_column(f"{cid}/{name} (ensemble)", "fit", X[:, j], Xq[:, j], tv[:, ov.p_off + j],
                            qv[:, ov.p_off + j])


@pytest.mark.parametrize("cid,column,kind", pr.POWER_TARGET_CASES, ids=_ids(pr.POWER_TARGET_CASES))
def test_target_power_fit_corner_columns(weights, cid, column, kind):
    X, y = pr.target_table(column)
    ov = pr.OracleViews(X, "ensemble")
    _, _, eng, _ = _fit_and_query(weights, "ensemble", X, y, X[:4], ov.Vw)
    _check_target(cid, kind, y, eng)


# ============================================================================ 3. fingerprints
@pytest.mark.parametrize("cid,F,n,dup", pr.FINGERPRINT_CASES, ids=_ids(pr.FINGERPRINT_CASES))
def test_fingerprints_bit_exact(weights, cid, F, n, dup):
    X, y, Xq = pr.fingerprint_table(F, n, dup)
    ov = pr.OracleViews(X, "ensemble")
    tv, qv, _, _ = _fit_and_query(weights, "ensemble", X, y, Xq, ov.Vw)
    _check_fingerprints(ov, tv, X, True)
    _check_fingerprints(ov, qv, Xq, False)
    src, _ = pr.duplicate_rows(n, dup)
    np.testing.assert_array_equal(qv[0, ov.fp_off:], tv[src, ov.fp_off:])     # the un-rehashed hash
    _check_raw_and_quantile(ov, tv, X)
    _check_raw_and_quantile(ov, qv, Xq)
    if F == 1:  # no SVD columns: raw | quantile | power | fingerprints, as the oracle's features
        from oracle.tabpfn_oracle import EstimatorState, FitState, OracleTabPFN

        assert ov.k == 0 and tv.shape[1] == 3 * F + 0 + pr.E == 11
        orc = OracleTabPFN(weights, pr.E, CFG.softmax_temperature, seed=pr.SEED, preprocessing=po.MODE_ENSEMBLE)
        st = FitState(F, 1, 0.0, 1.0, 0.0, [], [], qtab=ov.qtab)
        for e in (0, 3):
            es = EstimatorState(po.T_QSVD, e >= 2, 3, 2, None, None, None, None, po.fingerprint_salt(pr.SEED, e))
            for views, R, train in ((tv, X, True), (qv, Xq, False)):
                feats = orc._features(R, st, es, train)
                assert feats.shape == (R.shape[0], 3)
                np.testing.assert_array_equal(views[:, 0], feats[:, 0])
                np.testing.assert_allclose(views[:, 1], feats[:, 1], rtol=0, atol=1e-6)
                np.testing.assert_array_equal(views[:, ov.fp_off + e], feats[:, 2])


# ============================================================================ 4. SVD
@pytest.mark.parametrize("cid,n,F", pr.SVD_CASES, ids=_ids(pr.SVD_CASES))
def test_svd_with_a_constant_column(weights, cid, n, F):
    X, y, Xq = pr.svd_table(n, F)
    ov = pr.OracleViews(X, "ensemble")
    tv, qv, _, _ = _fit_and_query(weights, "ensemble", X, y, Xq, ov.Vw)
    _check_raw_and_quantile(ov, tv, X)
    _check_raw_and_quantile(ov, qv, Xq)
    assert np.ptp(tv[:, ov.q_off + 2]) == 0
    _check_svd(ov, tv, X)
    _check_svd(ov, qv, Xq)
    assert np.isnan(qv[5, ov.s_off:ov.s_off + ov.k]).all()
    _check_fingerprints(ov, tv, X, True)
    _check_fingerprints(ov, qv, Xq, False)


# ============================================================================ 5. end to end
@pytest.mark.parametrize("cid,mode,kind", pr.E2E_CASES, ids=_ids(pr.E2E_CASES))
def test_degenerate_tables_match_the_oracle_end_to_end(weights, cid, mode, kind):
    from oracle.tabpfn_oracle import OracleTabPFN

    X, y, Xq = pr.e2e_table(kind)
    n, F = X.shape
    Vw = 3 * F + (po.svd_components(n, F) if mode == "ensemble" else 0) + pr.E
    _, _, _, logits = _fit_and_query(weights, mode, X, y, Xq, Vw)
    p = torch.softmax(logits, -1).double().cpu().numpy()
    orc = OracleTabPFN(weights, CFG.n_estimators, CFG.softmax_temperature, seed=pr.SEED, emulate_bf16=True,
                       preprocessing=pr.MODES[mode])
    orc.fit(X, y)
    p_ref = orc.predict_probs(Xq).astype(np.float64)
    # predict_logits is the log of the mixed bar probabilities: -inf is the log of a bar without
    # mass.  The oracle has 0 there, or the rounding of its float32 cdf (a translated estimator's
    # bars are differences of a float32 cumsum in [0, 1]: at most one spacing of 1, 2^-23).
    # Nothing else may be non-finite.
    lg = logits.cpu().numpy()
    assert not np.isnan(lg).any() and not np.isposinf(lg).any()
    assert np.isfinite(lg).any(1).all() and np.isfinite(p).all()
    assert (p_ref[np.isneginf(lg)] <= 2.0 ** -23).all(), p_ref[np.isneginf(lg)].max()
    tv = 0.5 * np.abs(p - p_ref).sum(1)
    print(f"{cid}: TV to the oracle max {tv.max():.4f} mean {tv.mean():.4f}")
    assert tv.max() <= pr.E2E_TV_MAX, (tv.max(), tv.mean())
