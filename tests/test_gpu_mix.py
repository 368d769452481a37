"""GPU: the ensemble mix kernels (k_mix_log / _prob / _sample / _nll / _score, the k_group_* twins)
through npfn_mix_rows, on crafted fp16 logits, against the float64 reference tests/mix_ref.py.

Bar counts (each the smallest that reaches its branch of csrc/npfn_kernels.hip):
  generic path  2, 6 (both / most bars are tail bars, 250 threads idle), 250, 257, 1022 (per = 1 /
                2 with empty threads / 4 with a short last thread), 8196, 12 000 (past the register
                path's cap; 98 KB / 144 KB of LDS with translation);
  register path 4, 64, 1024 (<5>, nv = 1: 1 / 16 / 256 live threads), 1028 (nv = 2, thread 128 half
                filled), 5000, 5120 (nv = 5: the default, the full instance), 5124, 8192 (<8>: first
                and last size; 65 600 B of LDS with translation).
Estimators: the ett patterns of mix_ref.ETT_PATTERNS (a translated estimator first, last, twice in
a row, at both parities of e, and the engine's own 8).  Tables: the oracle's for the targets z,
exp(1.5 z), -exp(1.5 z) (none / the upper third / the lower third of the bars cancelled).  16
logit rows per case (mix_ref.case_logits).  Every combination under geo 0 and 1.

BAR, arithmetic mean (mix_ref.mix_bar): per bar |p - p_ref| <= rel p_ref + (n_translated / E) 2
(ceil(nb / 256) + 16) 2^-24.  rel = 2e-5 covers __expf's argument rounding over a logit range of
about 20; a row whose scaled logits span more (the +-65504 row: 1.5e5) gets rel = 2^-23 range
instead, the rounding of x * invT itself in float32 (half an ulp at |x| invT for each of the two
values a difference is formed from).  A bar with mass is never held tighter than 2^-120: below
float32's smallest normal number, 2^-126, the format has no relative precision and __expf flushes.

BAR, geo: log p - log p_ref, its row median over the compared bars removed, within rel + (1 / E)
sum over translated e of delta / q_e,ref (delta the absolute term above).  Bars where a translated
delta / q_e,ref > 0.5 are excused; in the N(0, s^2) rows they may be at most half of the bars with
mass (s = 0.5, and 0.25 from 5124 bars on; the crafted rows hold their mass in a handful of bars
by construction and are not counted).  Bars below 2^-120 in the reference are outside float32's
range after the final softmax and are not compared.  A bar that is zero by structure
(mix_ref.structural_zero: a -inf logit of an untranslated estimator, an empty row, two borders
forced to the same CDF value or read from the same massless source bucket) is exactly zero on the
device.  A reference zero that is the difference of two equal prefix sums read at different source
buckets -- a run of -inf logits inside a translated row, or the bar below the first border forced
to 1, which takes 1 - fl(prefix) -- is not: the device's float32 scan forms the two prefixes by
different additions (thread-serial, wave scan, wave bases), they agree to rounding only, and what
is left of the difference, at most delta, is mass to the mean of logs (tabpfn's float32 cumsum does
the same).  Measured on the device, such bars showed up from 64 bars on.  The decoder emits no
-inf, so in the engine only the bar below the first forced 1 is of this kind.  The row with no
mass is all zeros without exception.

TAILS: every figure is checked twice.  Against the float64 tail arithmetic on the DEVICE's own
mixture (the k_mix_prob row), with the flat tolerances: the draw's CDF within nb 2^-24 of u (plus
what rounding the draw to float32 moves its CDF by, p_j ulp(theta) / (2 w_j), which no kernel can
undo), the log density within 2e-3, the CDF within 2e-6 (tests/test_gpu_bar_cdf.py).  And against
the reference mixture with the mix's own bar propagated: summed up to the draw's / target's bar
for the CDF, mix_bar_j / p_ref,j for the log density (d log p = dp / p) -- a log density or CDF
cannot be known better than the mixture it is read from.
"""
import functools
import math

import numpy as np
import pytest
import torch

import mix_ref as mr
from oracle.philox import uniforms

pytestmark = pytest.mark.gpu

NB_GENERIC = (2, 6, 250, 257, 1022, 8196, 12000)
NB_FAST = (4, 64, 1024, 1028, 5000, 5120, 5124, 8192)
INV_T = mr.inv_temperature(0.9)
DEV = "cuda"
LOG_EPS = math.log(1e-15)
SEED = 11


def _mix(op, logits, **kw):
    from npe_pfn.engine import mix_rows

    return mix_rows(op, logits, inv_temperature=float(INV_T), **kw)


@functools.lru_cache(maxsize=None)
def _tables(nb):
    return mr.tables_for(nb)


def _device_table(nb, target):
    from npe_pfn.engine import pack_translation

    (idx, share, tc), _, _ = _tables(nb)[0][target]
    return pack_translation(idx, share, tc, DEV)


def _rel_rows(lg16):
    return mr.rel_rows(lg16, INV_T)


def _check_arith(p, ref, lg16, n_tr, E, what):
    worst, where, zeros_ok = mr.arith_fraction(p, ref, lg16, INV_T, n_tr, E)
    assert zeros_ok, f"{what}: mass in a bar, or a row, that the reference leaves empty"
    assert worst <= 1.0, f"{what}: |p - p_ref| is {worst:.3f} of its bar at {where}"
    return worst


def _check_geo(p, ref, q, structural, ett, lg16, what):
    worst, excused, zeros_ok, kept = mr.geo_fraction(p, ref, q, structural, ett, lg16, INV_T)
    bad = np.argwhere((ref == 0) & structural & (p != 0))
    assert zeros_ok, (f"{what}: mass in {len(bad)} bars that are zero by structure, first (row, bar, p): "
                      f"{[(int(r), int(b), float(p[r, b])) for r, b in bad[:6]]}")
    assert kept, f"{what}: a compared bar lost its mass"
    assert excused <= 0.5, f"{what}: {excused:.2f} of the bars with mass are excused in a random row"
    assert worst <= 1.0, f"{what}: log p - log p_ref is {worst:.3f} of its bar"
    return worst, excused


def _check_log(lp, p, what):
    """k_mix_log's row is the log of k_mix_prob's: __logf is v_log_f32 (1 ulp in log2 units) times
    ln 2, so within 4e-7 |log p| + 1e-6; -inf exactly where p = 0."""
    assert (np.isneginf(lp) == (p == 0)).all(), what
    ok = p > 0
    want = np.log(p[ok].astype(np.float64))
    assert (np.abs(lp[ok] - want) <= 4e-7 * np.abs(want) + 1e-6).all(), what


def _combos(nb):
    """(ett or None, target or None) of a bar count: the untranslated call once, then every
    pattern under every table (a pattern without a translated estimator still carries a table)."""
    yield None, None, 2
    for ett in mr.ETT_PATTERNS:
        for target in (mr.TARGETS if any(ett) else ("exp",)):
            yield ett, target, len(ett)


@pytest.mark.parametrize("nb", NB_GENERIC + NB_FAST)
def test_prob_and_log_against_the_reference(nb):
    tables, _ = _tables(nb)
    geo_scale = 0.5 if nb < 5124 else 0.25 if nb < 12000 else 0.05
    worst = {0: 0.0, 1: 0.0}
    share = 0.0
    for ci, (ett, target, E) in enumerate(_combos(nb)):
        table = tables[target][0] if target else None
        tab, tc = _device_table(nb, target) if target else (None, None)
        n_tr = sum(ett) if ett else 0
        for geo in (0, 1):
            lg16 = mr.case_logits(nb, E, table[2] if table else np.zeros(nb), seed=1000 * nb + 10 * ci + geo,
                                  scale=geo_scale if geo else 1.0)
            lg = torch.from_numpy(lg16).to(DEV)
            kw = dict(ett=list(ett), tab=tab, tcancel=tc) if target else {}
            p = _mix("prob", lg, geo=geo, **kw).cpu().numpy()
            lp = _mix("log", lg, geo=geo, **kw).cpu().numpy()
            what = f"nb={nb} ett={ett} target={target} geo={geo}"
            _check_log(lp, p, what)
            q = mr.estimator_probs(lg16, INV_T, ett, table)
            if geo:
                ref = mr.geo_from_probs(q, lg16, INV_T, ett)
                w, s = _check_geo(p, ref, q, mr.structural_zero(lg16, INV_T, ett, table), ett, lg16, what)
                share = max(share, s)
            else:
                ref = q.mean(0)
                w = _check_arith(p, ref, lg16, n_tr, E, what)
            worst[geo] = max(worst[geo], w)
            for r in (mr.ROW_EMPTY_ALL,):
                assert (p[r] == 0).all() and np.isneginf(lp[r]).all(), what
    print(f"nb={nb}: largest fraction of the bar: mean {worst[0]:.3f}, geo {worst[1]:.3f}; "
          f"largest excused share {share:.2f}")


# ------------------------------------------------------------------------------------- tails
TAIL_COMBOS = ((None, None, 0), ([1, 0], "exp", 0), ([0, 1, 0], "-exp", 1))
N_Y = 13


def _targets(b32):
    """test_gpu_bar_cdf.py's 13 targets on the borders b32 (the inner border: one of a collapsed
    pair when the borders hold one, so that a zero-width bar lies at the target)."""
    b = b32.astype(np.float64)
    nb = b.shape[0] - 1
    m = nb // 2
    flat = np.nonzero(np.diff(b32[1:nb]) == 0)[0]
    inner = b[flat[len(flat) // 2] + 1] if flat.size else b[max(m, 1)]
    return np.array([b[0] - 0.37 * (b[1] - b[0]) - 0.1, b[0], b[0] + 0.4 * (b[1] - b[0]), b[1],
                     0.5 * (b[m] + b[m + 1]), inner, b[nb - 1], b[nb - 1] + 0.3 * (b[nb] - b[nb - 1]), b[nb],
                     b[nb] + 0.45 * (b[nb] - b[nb - 1]) + 0.1, -np.inf, np.inf, np.nan]).astype(np.float32)


def _summed_bar(bar, j, both_sides):
    c = np.cumsum(bar, axis=1)
    left = c[np.arange(bar.shape[0]), j]
    if not both_sides:
        return left
    return np.minimum(left, c[:, -1] - left + bar[np.arange(bar.shape[0]), j])


@pytest.mark.parametrize("nb", NB_GENERIC + NB_FAST)
def test_tails_against_the_reference(nb):
    tables, bz = _tables(nb)
    bz_d = torch.from_numpy(bz).to(DEV)
    for ci, (ett, target, geo) in enumerate(TAIL_COMBOS):
        E = len(ett) if ett else 2
        table = tables[target][0] if target else None
        tab, tc = _device_table(nb, target) if target else (None, None)
        kw = dict(ett=list(ett), tab=tab, tcancel=tc, geo=geo) if target else dict(geo=geo)
        lg16 = mr.case_logits(nb, E, table[2] if table else np.zeros(nb), seed=77 * nb + ci, scale=0.5 if geo else 1.0)
        lg = torch.from_numpy(lg16).to(DEV)
        R = mr.N_ROWS
        what = f"nb={nb} ett={ett} target={target} geo={geo}"
        p_dev = _mix("prob", lg, **kw)
        p = p_dev.cpu().numpy()
        p64 = p.astype(np.float64)
        ref = mr.mix_probs(lg16, INV_T, ett, table, geo=bool(geo))
        has_mass = ref.sum(1) > 0
        n_tr = sum(ett) if ett else 0
        mixbar = (_rel_rows(lg16)[:, None] * ref + mr.delta_abs(nb) * n_tr / E) if not geo else None
        # ---------------------------------------------------------------- sample
        ystats = np.asarray(tables[target or "z"][1], dtype=np.float32)
        ys_d = torch.from_numpy(ystats).to(DEV)
        b32 = mr.borders32(bz, ystats)
        off, prow0, ldf, col, counter = 3, 7, 3, 1, 5
        feat = torch.full((off + R, ldf), 123.0, device=DEV)
        acc = torch.full((off + R,), 0.25, device=DEV)
        tail = dict(bz=bz_d, ystats=ys_d, seed=SEED, counter=counter, row_offset=off, philox_row0=prow0, feat=feat,
                    col=col, log_eps=LOG_EPS)
        _mix("sample", lg, out0=acc, **tail, **kw)
        f, a = feat.cpu().numpy(), acc.cpu().numpy()
        # group twin: global row g = off + r reads p row g / per, so its rows are shifted by off
        feat2, acc2 = torch.full_like(feat, 123.0), torch.full_like(acc, 0.25)
        pg = torch.cat([torch.zeros((off, nb), device=DEV), p_dev]).contiguous()
        _mix("group_sample", pg, n_rows=R, per=1, out0=acc2, **{**tail, "feat": feat2})
        assert torch.equal(feat.view(torch.int32), feat2.view(torch.int32)), f"{what}: group_sample differs"
        assert torch.equal(acc.view(torch.int32), acc2.view(torch.int32)), f"{what}: group_sample differs"
        assert (f[:off] == 123.0).all() and (f[:, [0, 2]] == 123.0).all() and (a[:off] == 0.25).all(), what
        th = f[off:, col]
        lpd = a[off:].astype(np.float64) - 0.25
        u = uniforms(SEED, counter, R, row_offset=prow0 + off).astype(np.float64)
        assert np.isnan(th[~has_mass]).all() and np.isnan(lpd[~has_mass]).all(), what
        m = has_mass
        rows = np.arange(R)[m]
        j = mr.sample_bucket(b32.astype(np.float64), th[m].astype(np.float64))
        # a draw that rounds onto its bar's left border is bucketed one bar down: count it in its own
        up = (th[m] == b32[j + 1]) & (ref[rows, j] == 0) & (j + 1 < nb)
        j = np.where(up, j + 1, j)
        assert (ref[rows, j] > 0).all() and (p[rows, j] > 0).all(), f"{what}: a draw in a bar without mass"
        wj = (b32[j + 1].astype(np.float64) - b32[j].astype(np.float64))
        fmt = np.where(wj > 0, np.spacing(np.abs(th[m])).astype(np.float64) / 2 / np.where(wj > 0, wj, 1.0), 0.0)
        own = np.abs(mr.cdf_linear(p64[m], b32, th[m]) - u[m])
        lim = nb * 2.0 ** -24 + (p64[rows, j] / p64[m].sum(1)) * fmt
        assert (own <= lim).all(), f"{what}: |F(theta) - u| on the device's mixture {own.max():.3e} > {lim.min():.3e}"
        if mixbar is not None:
            vs = np.abs(mr.cdf_linear(ref[m], b32, th[m]) - u[m])
            lim2 = lim + _summed_bar(mixbar[m], j, False)
            assert (vs <= lim2).all(), f"{what}: |F_ref(theta) - u| {vs.max():.3e}"
        want = mr.log_density(p64[m], b32, th[m])
        want = np.where(np.isneginf(want), LOG_EPS, want)
        assert (np.abs(lpd[m] - want) <= 2e-3 + 1e-6 * np.abs(want)).all(), f"{what}: log density of the draw"
        if mixbar is not None:
            want = mr.log_density(ref[m], b32, th[m])
            okr = np.isfinite(want)
            assert (np.abs(lpd[m] - want)[okr] <= 2e-3 + (mixbar[rows, j] / ref[rows, j])[okr]).all(), \
                f"{what}: the draw's log density against the reference mixture"
        # ---------------------------------------------------------------- nll and score
        for collapsed in (False, True):
            ys2 = np.array([100.0, 2e-3, 0, 0, 0, 0], dtype=np.float32) if collapsed else ystats
            b2 = mr.borders32(bz, ys2)
            ys2_d = torch.from_numpy(ys2).to(DEV)
            y = np.tile(_targets(b2), R)
            RR = R * N_Y
            lgt = lg.repeat_interleave(N_Y, dim=1).contiguous()
            featy = torch.zeros((RR, 2), device=DEV)
            featy[:, 1] = torch.from_numpy(y).to(DEV)
            lp_o, cdf_o = torch.full((RR, 2), 9.0, device=DEV), torch.full((RR, 2), 9.0, device=DEV)
            t2 = dict(bz=bz_d, ystats=ys2_d, feat=featy, col=1, log_eps=LOG_EPS, ldo=2)
            _mix("score", lgt, out0=lp_o, out1=cdf_o, **t2, **kw)
            nll = torch.full((RR,), 0.5, device=DEV)
            _mix("nll", lgt, out0=nll, **{k: v for k, v in t2.items() if k != "ldo"}, **kw)
            lp_g, cdf_g, nll_g = torch.full_like(lp_o, 9.0), torch.full_like(cdf_o, 9.0), torch.full_like(nll, 0.5)
            _mix("group_score", p_dev, n_rows=RR, per=N_Y, out0=lp_g, out1=cdf_g, **t2)
            _mix("group_nll", p_dev, n_rows=RR, per=N_Y, out0=nll_g, **{k: v for k, v in t2.items() if k != "ldo"})
            for x, g in ((lp_o, lp_g), (cdf_o, cdf_g), (nll, nll_g)):
                assert torch.equal(x.view(torch.int32), g.view(torch.int32)), f"{what}: group twin differs"
            lpv, cdv = lp_o.cpu().numpy(), cdf_o.cpu().numpy()
            assert (lpv[:, 1] == 9.0).all() and (cdv[:, 1] == 9.0).all(), what
            lpv, cdv = lpv[:, 0].astype(np.float64), cdv[:, 0].astype(np.float64)
            nl = nll.cpu().numpy()
            assert np.array_equal(nl, np.float32(0.5) + lp_o[:, 0].cpu().numpy(), equal_nan=True), \
                f"{what}: nll is not 0.5 + score's log density"
            P = np.repeat(p64, N_Y, 0)
            mm = np.repeat(has_mass, N_Y)
            fin = ~np.isnan(y)
            assert np.isnan(lpv[~mm]).all() and np.isnan(cdv[~mm]).all(), what
            assert np.isnan(cdv[~fin]).all(), what
            ok = mm & fin
            want = mr.log_density(P[ok], b2, y[ok])
            want = np.where(np.isneginf(want), LOG_EPS, want)
            finite = np.isfinite(want)
            assert np.array_equal(lpv[ok][~finite], want[~finite]), what
            dlp = np.abs(lpv[ok][finite] - want[finite])
            assert (dlp <= 2e-3 + 1e-6 * np.abs(want[finite])).all(), f"{what} collapsed={collapsed}: log density {dlp.max():.3e}"
            wantc = mr.cdf(P[ok], b2, y[ok])
            dc = np.abs(cdv[ok] - wantc)
            assert (dc <= 2e-6).all(), f"{what} collapsed={collapsed}: CDF {dc.max():.3e}"
            assert ((cdv[ok] >= 0) & (cdv[ok] <= 1)).all(), what
            if mixbar is not None:
                REF, MB = np.repeat(ref, N_Y, 0)[ok], np.repeat(mixbar, N_Y, 0)[ok]
                jj = mr.sample_bucket(b2.astype(np.float64), np.nan_to_num(y[ok].astype(np.float64)))
                ar = np.arange(REF.shape[0])
                wr = mr.log_density(REF, b2, y[ok])
                cmp_ = np.isfinite(wr) & (REF[ar, jj] > 0)
                assert (np.abs(lpv[ok][cmp_] - wr[cmp_]) <= 2e-3 + 1e-6 * np.abs(wr[cmp_]) +
                        MB[ar, jj][cmp_] / REF[ar, jj][cmp_]).all(), f"{what}: log density against the reference mixture"
                assert (np.abs(cdv[ok] - mr.cdf(REF, b2, y[ok])) <= 2e-6 + _summed_bar(MB, jj, True)).all(), what
    print(f"nb={nb}: tails ok")


@pytest.mark.parametrize("nb", (250, 1028, 5000, 8192, 12000))
def test_log_over_a_row_window(nb):
    tables, _ = _tables(nb)
    ett = [0, 1, 0]
    tab, tc = _device_table(nb, "exp")
    lg16 = mr.case_logits(nb, 3, tables["exp"][0][2], seed=nb)
    lg = torch.from_numpy(lg16).to(DEV)
    for geo in (0, 1):
        full = _mix("log", lg, ett=ett, tab=tab, tcancel=tc, geo=geo)
        win = _mix("log", lg, ett=ett, tab=tab, tcancel=tc, geo=geo, row0=5, n_rows=7, ldo=nb + 3)
        assert win.shape == (7, nb + 3)
        assert torch.equal(win[:, :nb].view(torch.int32), full[5:12].view(torch.int32))


# --------------------------------------------------------------------- tie-in with the engine
TIE_NB = (250, 1028, 5000, 8192)
N_CTX, N_FEAT, N_QUERY = 48, 3, 16


@functools.lru_cache(maxsize=None)
def _engine(nb):
    from npe_pfn.engine import Engine
    from npe_pfn.weights import ModelConfig, synthetic_weights

    cfg = ModelConfig(n_layers=1, max_groups=16, n_bars=nb)
    w = synthetic_weights(cfg, seed=4)
    return Engine(cfg, w, device=torch.device("cuda", 0), random_state=3, preprocessing="ensemble"), w


def _tie_data(target):
    rng = np.random.default_rng(21)
    X = rng.normal(size=(N_CTX, N_FEAT)).astype(np.float32)
    g = {"z": lambda v: v, "exp": lambda v: np.exp(1.5 * v), "-exp": lambda v: -np.exp(1.5 * v)}[target]
    lin = X @ np.array([0.8, -0.5, 0.3]) + 0.3 * rng.normal(size=N_CTX)
    lin2 = X @ np.array([-0.2, 0.6, 0.5]) + 0.3 * rng.normal(size=N_CTX)
    th = np.stack([g(lin), g(lin2)], 1).astype(np.float32)
    Xq = rng.normal(size=(N_QUERY, N_FEAT)).astype(np.float32)
    return X, th, Xq


def _near_source_border(bz, ystats, frm32):
    """[nb + 1] bool: the common border lies within 2 float32 ulp of a source border (there the
    source bucket or the share may legitimately flip with the last bit of either)."""
    to = mr.borders32(bz, ystats).astype(np.float64)
    f = np.sort(frm32.astype(np.float64))
    k = np.clip(np.searchsorted(f, to), 1, f.size - 1)
    dist = np.minimum(np.abs(to - f[k - 1]), np.abs(to - f[k]))
    return dist <= 2 * np.spacing(np.abs(to).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("target", mr.TARGETS)
@pytest.mark.parametrize("nb", TIE_NB)
def test_engine_table_and_mix_identities(nb, target):
    from oracle.preprocess_oracle import yj_fit

    eng, w = _engine(nb)
    bz = np.asarray(w["borders"], dtype=np.float32)
    X, th, Xq = _tie_data(target)
    inv_t = float(mr.inv_temperature(eng.cfg.softmax_temperature))
    eng.set_average_before_softmax(False)
    eng.fit(X, th[:, 0])
    t = eng.debug_target_translation()
    assert t["translated"] and list(t["ett"]) == [0, 0, 1, 1, 0, 0, 1, 1]
    # ---- the exported table against the oracle's functions on the exported lambda and statistics
    idx, share, tc, frm32 = mr.target_translation_host(bz, t["ylam"], t["ystats"])
    assert np.array_equal(t["tcancel"], tc), f"tcancel differs in {(t['tcancel'] != tc).sum()} bars"
    if target != "z":
        assert t["tcancel"].any(), "the skewed target cancels no bar on the device"
    near = _near_source_border(bz, t["ystats"], frm32)
    flags_d = np.where(t["share"] < 0, -1, np.where(t["share"] > 1.5, 1, 0))
    flags_h = np.where(share < 0, -1, np.where(share > 1.5, 1, 0))
    assert np.array_equal(flags_d[~near], flags_h[~near])
    same = (t["idx"] == idx) & (flags_d == flags_h) & ((flags_h != 0) | (np.abs(t["share"] - share) <= 1e-5))
    excused = ~same & near
    own = mr.oracle_table(th[:, 0], bz)
    near_own = _near_source_border(bz, own[1], mr.target_translation_host(bz, own[2], own[1])[3])
    print(f"nb={nb} {target}: lambda {t['ylam']:.4f} (oracle {yj_fit(th[:, 0]):.4f}), {int(tc.sum())} bars cancelled, "
          f"{int((~same).sum())} entries differ, {int(excused.sum())} of them excused; borders within 2 ulp of a "
          f"source border: {int(near.sum())} (the oracle's own lambda: {int(near_own.sum())})")
    assert (same | near).all(), f"{int((~same & ~near).sum())} table entries differ away from any source border"
    assert excused.sum() <= 0.005 * (nb + 1)
    # ---- log through npfn_mix_rows == predict, bit for bit, under both mixes
    ett, tab, tcd = eng.mix_translation()
    from npe_pfn.engine import mix_rows
    for geo in (False, True):
        eng.set_average_before_softmax(geo)
        want = eng.predict_logits(Xq)
        lg = eng.forward_logits(Xq)
        got = mix_rows("log", lg, inv_temperature=inv_t, ett=ett, tab=tab, tcancel=tcd, geo=geo)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"geo={geo}"
    eng.set_average_before_softmax(False)


@pytest.mark.parametrize("target", mr.TARGETS)
@pytest.mark.parametrize("nb", TIE_NB)
def test_engine_ar_steps_through_mix_rows(nb, target):
    from npe_pfn.engine import mix_rows

    eng, w = _engine(nb)
    eng.set_average_before_softmax(False)
    bz_d = torch.from_numpy(np.asarray(w["borders"], dtype=np.float32)).to(DEV)
    X, th, Xq = _tie_data(target)
    inv_t = float(mr.inv_temperature(eng.cfg.softmax_temperature))
    counter, rb, eps = 9, 5, 1e-15
    log_eps = float(np.log(np.float32(eps)))
    xq_d = torch.from_numpy(Xq).to(DEV)
    theta, lp = eng.ar_sample(X, th, xq_d, counter=counter, with_log_prob=True, eps=eps, row_base=rb)
    lps, cdfs = eng.ar_score(X, th, xq_d, theta, eps=eps)
    xu = xq_d[:4].contiguous()
    theta_rep, _ = eng.ar_sample(X, th, xu.repeat_interleave(4, 0), counter=counter, row_base=rb, x_unique=xu)
    feat = torch.zeros((N_QUERY, N_FEAT + 2), device=DEV)
    feat[:, :N_FEAT] = xq_d
    acc = torch.zeros(N_QUERY, device=DEV)
    eng.ar_fit_begin(X, th)
    for k in range(2):
        eng.ar_fit_step(k)
        ett, tab, tcd = eng.mix_translation()
        ys_d = torch.from_numpy(eng.debug_target_translation()["ystats"]).to(DEV)
        lg = eng.forward_logits(feat[:, :N_FEAT + k].contiguous())
        common = dict(inv_temperature=inv_t, ett=ett, tab=tab, tcancel=tcd, bz=bz_d, ystats=ys_d)
        if k == 0:   # repeated query rows: the mixture once per distinct row, then the group twin
            p_u = mix_rows("prob", eng.forward_logits(xu), inv_temperature=inv_t, ett=ett, tab=tab, tcancel=tcd)
            f_rep = torch.zeros((N_QUERY, 1), device=DEV)
            mix_rows("group_sample", p_u, n_rows=N_QUERY, per=4, bz=bz_d, ystats=ys_d, seed=eng.random_state,
                     counter=counter, philox_row0=rb, feat=f_rep, col=0, log_eps=log_eps)
            assert torch.equal(f_rep[:, 0].view(torch.int32), theta_rep[:, 0].contiguous().view(torch.int32))
        # score first (it reads the column), on the engine's own draw
        feat[:, N_FEAT + k] = theta[:, k]
        o0, o1 = torch.zeros(N_QUERY, device=DEV), torch.zeros(N_QUERY, device=DEV)
        mix_rows("score", lg, feat=feat, col=N_FEAT + k, out0=o0, out1=o1, ldo=1, log_eps=log_eps, **common)
        assert torch.equal(o0.view(torch.int32), lps[:, k].contiguous().view(torch.int32)), f"step {k}: logp_steps"
        assert torch.equal(o1.view(torch.int32), cdfs[:, k].contiguous().view(torch.int32)), f"step {k}: cdf_steps"
        feat[:, N_FEAT + k] = 0
        mix_rows("sample", lg, feat=feat, col=N_FEAT + k, out0=acc, seed=eng.random_state, counter=counter + k,
                 philox_row0=rb, log_eps=log_eps, **common)
        assert torch.equal(feat[:, N_FEAT + k].contiguous().view(torch.int32),
                           theta[:, k].contiguous().view(torch.int32)), f"step {k}: the draw"
    assert torch.equal(acc.view(torch.int32), lp.view(torch.int32)), "the log density of the two steps"


def test_engine_refuses_what_lds_cannot_hold_and_exports_nothing_before_a_fit():
    from npe_pfn.engine import Engine, EngineError, mix_rows, pack_translation
    from npe_pfn.weights import ModelConfig, synthetic_weights

    with pytest.raises(ValueError, match="n_bars = 20000"):
        Engine(ModelConfig(n_layers=1, max_groups=16, n_bars=20000))
    lg = torch.zeros((1, 2, 20000), dtype=torch.float16, device=DEV)
    tab, tc = pack_translation(np.zeros(20001, np.int32), np.zeros(20001, np.float32), np.zeros(20000, np.uint8), DEV)
    assert mix_rows("prob", lg).shape == (2, 20000)            # 82 KB without translation: fits
    with pytest.raises(EngineError, match="LDS"):              # 242 KB with it: refused on the host
        mix_rows("prob", lg, ett=[1], tab=tab, tcancel=tc)
    cfg = ModelConfig(n_layers=1, max_groups=16, n_bars=64)
    eng = Engine(cfg, synthetic_weights(cfg, seed=4), device=torch.device("cuda", 0))
    with pytest.raises(EngineError, match=r"\(-3\)"):
        eng.debug_target_translation()
    eng.set_preprocessing("none")
    eng.fit(np.random.default_rng(0).normal(size=(20, 2)), np.arange(20.0))
    t = eng.debug_target_translation()
    assert not t["translated"] and t["idx"] is None and not t["ett"].any() and np.isnan(t["ylam"])
    assert eng.mix_translation() == (None, None, None)
