"""CPU: the float64 reference of the ensemble mix (tests/mix_ref.py) is right, and the bars of
tests/test_gpu_mix.py have the power to see a kernel that is subtly wrong.

* mix_ref against OracleTabPFN.predict_probs (float32, serial prefix sums) on a fitted small model,
  inside the very bars the device is held to.
* Seeded defects, each applied to the reference's own output or inputs, measured in units of the
  bar: every one but one lies more than 10 bars away in at least one case.  The exception is "the
  -1 / 2 flag read as a share", which is no defect at all: a border at or below the source range has
  idx 0 and an empty prefix, so 0 + p_0 * (-1) clamps to the flag's 0, and one at or above it has idx
  nb - 1, so prefix + 2 p clamps to the flag's 1 -- the flags only save the LDS read.  The test
  asserts that it stays inside the bar.
* The tables of the matrix reach the edges they are meant to (cancel boundary at every residue
  mod 4, a thread whose whole range is cancelled next to one that is not).
* Argument errors of npfn_mix_rows / npfn_debug_target_translation and the n_bars cap, without a
  GPU.
"""
import ctypes

import numpy as np
import pytest

import mix_ref as mr

NB_FAST = (4, 64, 1024, 1028, 5000, 5120, 5124, 8192)


# ------------------------------------------------------------------ the reference is right
@pytest.fixture(scope="module")
def small_model():
    from npe_pfn.weights import ModelConfig, synthetic_weights

    cfg = ModelConfig(n_layers=1, max_groups=16, n_bars=250)
    rng = np.random.default_rng(5)
    X = rng.normal(size=(48, 3)).astype(np.float32)
    lin = X @ np.array([0.8, -0.5, 0.3], dtype=np.float32) + 0.2 * rng.normal(size=48).astype(np.float32)
    Xq = rng.normal(size=(16, 3)).astype(np.float32)
    return cfg, synthetic_weights(cfg, seed=2), X, lin, Xq


@pytest.mark.parametrize("geo", (False, True))
@pytest.mark.parametrize("mode,target", ((0, "z"), (3, "z"), (3, "exp"), (3, "-exp")))
def test_reference_agrees_with_the_oracle(small_model, mode, target, geo):
    from oracle.tabpfn_oracle import OracleTabPFN

    cfg, w, X, lin, Xq = small_model
    y = {"z": lin, "exp": np.exp(1.5 * lin), "-exp": -np.exp(1.5 * lin)}[target].astype(np.float32)
    orc = OracleTabPFN(w, cfg.n_estimators, cfg.softmax_temperature, seed=1, preprocessing=mode,
                       average_before_softmax=geo)
    st = orc.fit(X, y)
    raw = orc._estimator_logits
    orc._estimator_logits = lambda q: raw(q).astype(np.float16).astype(np.float32)   # the mix reads fp16 logits
    probs, logits = orc.predict_probs(Xq, return_estimator_logits=True)
    lg16 = logits.astype(np.float16)
    assert np.array_equal(lg16.astype(np.float32), logits)
    ett = [int(es.target_tf) for es in st.estimators]
    table = None
    if any(ett):
        idx, share, flag, cancel = st.trans
        share = np.where(flag < 0, np.float32(-1), np.where(flag > 0, np.float32(2), share)).astype(np.float32)
        table = (idx, share, cancel.astype(np.uint8))
        if target != "z":
            assert cancel.any(), "the skewed target cancels no bar"
    invT = np.float32(1.0 / orc.T)   # the oracle's own rounding of 1 / T
    q = mr.estimator_probs(lg16, invT, ett if any(ett) else None, table)
    E = len(ett)
    if geo:
        ref = mr.geo_from_probs(q, lg16, invT, ett if any(ett) else None)
        worst, excused, zeros_ok, kept = mr.geo_fraction(
            probs, ref, q, mr.structural_zero(lg16, invT, ett if any(ett) else None, table),
            ett if any(ett) else None, lg16, invT)
        # the oracle takes the log of float32 probabilities, which flush to 0 (-inf) below 2^-126 where
        # the engine keeps the exact log-softmax: such bars are lost here by the oracle, not compared
        print(f"  excused share {excused:.2f}, every compared bar kept: {kept}")
        assert zeros_ok
    else:
        worst, where, zeros_ok = mr.arith_fraction(probs, q.mean(0), lg16, invT, sum(ett), E)
        assert zeros_ok
    print(f"mode={mode} target={target} geo={geo}: oracle float32 vs float64 reference: {worst:.3f} of the bar")
    assert worst <= 1.0


# ------------------------------------------------------------------ the bars have power
def _defect_cases():
    """(nb, nv, ett, target): register-path sizes at nv = 2 and 5, a translated estimator between
    two plain ones and three in a row, both skewed tables."""
    for nb in (1028, 5000):
        for ett in ([0, 1, 0], [1, 1, 1]):
            for target in ("exp", "-exp"):
                yield nb, (nb + 1023) // 1024, ett, target


def _ratio(p_def, ref, lg16, n_tr, E):
    return mr.arith_fraction(p_def.astype(np.float32), ref, lg16, mr.inv_temperature(0.9), n_tr, E)[0]


def test_seeded_defects_lie_far_outside_the_bar():
    invT = mr.inv_temperature(0.9)
    ratios = {}

    def note(name, r):
        ratios[name] = max(ratios.get(name, 0.0), r)

    for nb, nv, ett, target in _defect_cases():
        (idx, share, tc), _, _ = mr.tables_for(nb)[0][target]
        E, n_tr = len(ett), sum(ett)
        lg16 = mr.case_logits(nb, E, tc, seed=nb + E)[:, :mr.N_RANDOM]
        ref = mr.mix_probs(lg16, invT, ett, (idx, share, tc))
        r = lambda p: _ratio(p, ref, lg16, n_tr, E)   # noqa: E731
        PB = 4 * nv
        # a thread-boundary border's table entry taken from its neighbour
        inner = [b for b in range(PB, nb, PB) if 0 <= share[b] <= 1 and 0 <= share[b + 1] <= 1 and 0 <= share[b - 1] <= 1]
        b = inner[len(inner) // 2]
        for d, name in ((1, "border b = 4 nv t taken from b + 1"), (-1, "border b = 4 nv t taken from b - 1")):
            i2, s2 = idx.copy(), share.copy()
            i2[b], s2[b] = idx[b + d], share[b + d]
            note(name, r(mr.mix_probs(lg16, invT, ett, (i2, s2, tc))))
        # one tcancel byte of a 4-byte word dropped
        c = np.nonzero(tc)[0]
        edge = c[0] if c[0] > 0 else c[-1]
        t2 = tc.copy()
        t2[edge] = 0
        note("one tcancel byte dropped", r(mr.mix_probs(lg16, invT, ett, (idx, share, t2))))
        note("flag read as a share", r(mr.mix_probs(lg16, invT, ett, (idx, share, tc), _flags_as_share=True)))
        q = mr.estimator_probs(lg16, invT, ett, (idx, share, tc))
        note("last estimator dropped", r(q[:-1].sum(0) / E))
        note("1 / E taken from E + 1", r(q.sum(0) / (E + 1)))
        note("1 / E taken from E - 1", r(q.sum(0) / (E - 1)))
        moved = ref.copy()
        k = int(np.argmax(ref[0] > 0)) + nb // 3
        moved[:, k + 1] += moved[:, k]
        moved[:, k] = 0
        note("one bar's mass moved to its neighbour", r(moved))
        note("prefix sums restarted at a wave boundary",
             r(mr.mix_probs(lg16, invT, ett, (idx, share, tc), _cum_restart=64 * PB)))
    for name, v in ratios.items():
        print(f"{name}: {v:.1f} bars")
    benign = ratios.pop("flag read as a share")
    assert benign <= 1.0, "reading a flag as a share is supposed to clamp to the flag's own value"
    for name, v in ratios.items():
        assert v >= 10.0, f"{name}: only {v:.2f} bars away from the reference"


# ------------------------------------------------------------------ the tables reach their edges
def test_tables_reach_the_cancel_edges():
    residues = {"exp": set(), "-exp": set()}
    whole_thread = False
    for nb in NB_FAST:
        tables, _ = mr.tables_for(nb)
        assert not tables["z"][0][2].any()
        PB = 4 * ((nb + 1023) // 1024)
        for t in ("exp", "-exp"):
            idx, share, tc = tables[t][0]
            c = np.nonzero(tc)[0]
            assert c.size and (np.diff(c) == 1).all(), (nb, t)
            assert (share < 0).any() or (share > 1.5).any(), (nb, t)
            boundary = c[0] if t == "exp" else c[-1] + 1   # first cancelled bar / first kept bar
            assert (c[-1] == nb - 1) if t == "exp" else (c[0] == 0)
            residues[t].add(int(boundary) % 4)
            per_thread = tc[: nb - nb % PB].reshape(-1, PB) if nb >= PB else tc[None, :0]
            allc, nonec = per_thread.all(1), ~per_thread.any(1)
            whole_thread |= bool((allc[1:] & ~allc[:-1]).any() or (allc[:-1] & ~allc[1:]).any())
    print("cancel boundary residues mod 4:", residues)
    assert residues["exp"] == {0, 1, 2, 3} and residues["-exp"] == {0, 1, 2, 3}
    assert whole_thread


# ------------------------------------------------------------------ arguments and the cap
def test_n_bars_cap():
    from npe_pfn import limits

    assert limits.mix_lds_bytes(8192) == 65600 + limits.MIX_STATIC_LDS        # register path: p overlays pc
    assert limits.mix_lds_bytes(8196) == 64 + 12 * 8196 + limits.MIX_STATIC_LDS            # generic: p and pc
    assert limits.mix_lds_bytes(5000, translated=False) == 64 + 20000 + limits.MIX_STATIC_LDS
    for nb in (2, 5000, 8192, 12000):
        limits.check_n_bars(nb)
    with pytest.raises(ValueError, match="n_bars = 20000"):
        limits.check_n_bars(20000)
    with pytest.raises(ValueError, match="n_bars"):
        limits.check_n_bars(1)
    with pytest.raises(ValueError, match="n_bars = 8192"):
        limits.check_n_bars(8192, lds_limit=65536)


def test_bad_arguments_are_refused_before_any_launch():
    """Host checks only: the pointers are host buffers and no device is touched (an LDS need above
    the limit is refused whether or not a device answers: without one the limit is 64 KiB)."""
    from npe_pfn.engine import MIX_OPS, load_library

    lib = load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ip = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int32))

    def mix(op="log", logits=p, ld_rows=4, row0=0, n_rows=4, n_est=2, n_bars=8, invT=1.0, ett=None, tab=None,
            tcancel=None, geo=0, bz=p, ystats=p, row_offset=0, per=1, feat=p, ldf=2, col=1, out0=p, out1=p, ldo=8):
        return lib.npfn_mix_rows(MIX_OPS.get(op, op), logits, ld_rows, row0, n_rows, n_est, n_bars, invT, ett, tab,
                                 tcancel, geo, bz, ystats, 0, 0, row_offset, 0, per, feat, ldf, col, out0, out1, ldo,
                                 -30.0, None)

    assert mix(op=8) == -1 and b"mix_rows" in lib.npfn_last_error()
    assert mix(op=-1) == -1
    assert mix(n_rows=-1) == -1
    assert mix(n_rows=1 << 31, ld_rows=1 << 31) == -1
    assert mix(n_bars=1) == -1
    assert mix(logits=None) == -1
    assert mix(n_est=0) == -1 and mix(n_est=65) == -1
    assert mix(invT=0.0) == -1 and mix(invT=float("inf")) == -1 and mix(invT=float("nan")) == -1
    assert mix(ett=ip) == -1 and mix(tab=p, tcancel=p) == -1          # partly given
    assert mix(geo=2) == -1
    assert mix(row0=1) == -1 and mix(row0=-1) == -1                   # the window leaves ld_rows
    assert mix(op="prob", ld_rows=5) == -1                            # a window for an op other than log
    assert mix(ldo=7) == -1                                           # log: ldo < n_bars
    assert mix(out0=None) == -1
    assert mix(op="score", out0=None, out1=None) == -1
    assert mix(op="score", ldo=0) == -1
    assert mix(op="sample", bz=None) == -1 and mix(op="nll", feat=None) == -1 and mix(op="score", ystats=None) == -1
    assert mix(op="sample", col=2) == -1 and mix(op="sample", col=-1) == -1 and mix(op="nll", row_offset=-1) == -1
    assert mix(op="group_sample", per=0) == -1
    assert mix(op="group_nll", out0=None) == -1
    assert mix(n_bars=1 << 20, ldo=1 << 20) == -1 and b"LDS" in lib.npfn_last_error() and b"n_bars" in lib.npfn_last_error()
    assert mix(op="group_score", n_bars=1 << 20) == -1
    assert mix(n_rows=0, ld_rows=0) == 0                              # nothing to do, nothing launched
    assert mix(op="group_sample", n_rows=0) == 0

    i32 = ctypes.c_int32
    assert lib.npfn_debug_target_translation(None, 8, 2, p, p, ip, p, p, ip, ctypes.byref(i32())) == -1
    assert b"null engine" in lib.npfn_last_error()


def test_library_exports_and_signatures():
    from npe_pfn.engine import SIGNATURES, load_library
    from test_abi import declared_prototypes

    lib = load_library()
    protos = declared_prototypes()
    for name, n_args in (("npfn_mix_rows", 27), ("npfn_debug_target_translation", 10)):
        assert hasattr(lib, name), f"{name} is not exported by libnpfn.so"
        assert len(SIGNATURES[name][1]) == n_args == len(protos[name])
