"""ctypes binding of the C-ABI engine (include/npfn.h, libnpfn.so).

The library is built in-tree for gfx950 (``make -C npe-pfn_amd`` or
``__graft_entry__.build()``).  There is no CPU fallback: constructing an
:class:`Engine` without the library or without a ROCm device raises.

torch is imported first so that libnpfn.so binds to the HIP runtime torch
already loaded (same SONAME), which makes torch's device pointers and streams
valid inside the engine.
"""

from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .limits import check_engine_table, check_n_bars
from .weights import ModelConfig, pack_weights, synthetic_weights

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libnpfn.so")

# packed weight blobs of the last few weight sets (pack_weights costs ~30 ms per engine, paid
# again by every engine of a run_tsnpe_pfn round); keyed by the weight dict's identity, which
# the entry keeps alive, so a key is never reused by another dict
_PACK_CACHE: "Dict[Tuple[int, ModelConfig], Tuple[Dict[str, np.ndarray], np.ndarray]]" = {}
_PACK_CACHE_MAX = 3  # the regressor and classifier weight sets of a run_tsnpe_pfn round, and one more


def _packed(weights: Dict[str, np.ndarray], cfg: ModelConfig) -> np.ndarray:
    key = (id(weights), cfg)
    hit = _PACK_CACHE.get(key)
    if hit is not None and hit[0] is weights:
        return hit[1]
    blob = pack_weights(weights, cfg)
    if len(_PACK_CACHE) >= _PACK_CACHE_MAX:
        _PACK_CACHE.pop(next(iter(_PACK_CACHE)))
    _PACK_CACHE[key] = (weights, blob)
    return blob

# (name, restype, argtypes) of every entry point in include/npfn.h
_vp, _i64, _i32, _u64, _f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float


class NpfnConfig(ctypes.Structure):
    _fields_ = [
        ("d_model", ctypes.c_int32),
        ("n_heads", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("d_ff", ctypes.c_int32),
        ("n_bars", ctypes.c_int32),
        ("features_per_group", ctypes.c_int32),
        ("max_groups", ctypes.c_int32),
        ("n_estimators", ctypes.c_int32),
        ("softmax_temperature", ctypes.c_float),
        ("device", ctypes.c_int32),
        ("random_state", ctypes.c_uint64),
    ]


class NpfnProfEntry(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 48),
        ("launches", ctypes.c_int64),
        ("ms", ctypes.c_double),
        ("flops", ctypes.c_double),
        ("bytes", ctypes.c_double),
    ]


SIGNATURES = {
    "npfn_version": (ctypes.c_int, []),
    "npfn_last_error": (ctypes.c_char_p, []),
    "npfn_weights_size": (ctypes.c_size_t, [ctypes.POINTER(NpfnConfig)]),
    "npfn_engine_create": (ctypes.c_int, [ctypes.POINTER(NpfnConfig), _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "npfn_engine_destroy": (ctypes.c_int, [_vp]),
    "npfn_fit": (ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "npfn_predict": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "npfn_set_preprocessing": (ctypes.c_int, [_vp, _i32]),
    "npfn_set_average_before_softmax": (ctypes.c_int, [_vp, _i32]),
    "npfn_fit_classes": (ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "npfn_predict_proba": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "npfn_get_borders": (ctypes.c_int, [_vp, _vp, _vp]),
    "npfn_bar_sample": (ctypes.c_int, [_vp, _vp, _i64, _i32, _u64, _u64, _vp, _vp]),
    "npfn_bar_nll": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "npfn_bar_cdf": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "npfn_bar_stats": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "npfn_predict_stats": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "npfn_ar_sample": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _u64, _i64, _vp, _vp, _f, _vp]),
    "npfn_ar_sample_repeated": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i64, _u64, _i64, _vp, _vp,
                                               _f, _vp]),
    "npfn_ar_marginals": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i64, _u64, _i64, _vp, _vp, _f,
                                         _vp, _vp, _vp]),
    "npfn_ar_pair_marginals": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i64, _u64, _i64, _vp, _vp,
                                              _f, _vp, _i32, _vp, _vp, _vp]),
    "npfn_ar_log_prob": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _f, _vp]),
    "npfn_ar_log_prob_repeated": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _f, _vp]),
    "npfn_ar_score": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _f, _vp]),
    "npfn_box_support": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "npfn_compact_rows": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "npfn_box_propose": (ctypes.c_int, [_vp, _vp, _i32, _i64, _u64, _u64, _i64, _vp, _vp]),
    "npfn_predict_accept": (ctypes.c_int, [_vp, _vp, _i64, _i64, _f, _vp, _vp, _vp]),
    "npfn_restricted_box_round": (ctypes.c_int, [_vp, _vp, _vp, _i32, _f, _i64, _u64, _u64, _i64, _vp, _i64, _vp,
                                                 _vp]),
    "npfn_rank_accumulate": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "npfn_bar_cell_mass": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "npfn_pair_accumulate": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i64, _i64, _i64, _vp, _vp,
                                            ctypes.POINTER(_i32), _vp]),
    "npfn_mmd_sums": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp,
                                     ctypes.POINTER(_i32), _vp]),
    "npfn_w2_assign": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, ctypes.POINTER(_i32), _vp, _vp, _vp,
                                      ctypes.POINTER(_i32), _vp]),
    "npfn_c2st_fit": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, ctypes.POINTER(_i32), _i32, _vp, _vp, _i32,
                                     ctypes.POINTER(_i32), ctypes.POINTER(_i32), _i32, _i32, _i32, _vp, _f, _f, _f, _f,
                                     ctypes.POINTER(_i32), _vp, _vp, _vp, ctypes.POINTER(_i32), _vp]),
    "npfn_filter_stdeuclid": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    "npfn_sir_select": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _u64, _u64, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "npfn_kmeans_fit": (ctypes.c_int, [_vp, _i64, _i32, _i32, _u64, _i32, _f, _vp, _vp, _vp, _vp, _vp]),
    "npfn_kmeans_assign": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp]),
    "npfn_set_estimator_range": (ctypes.c_int, [_vp, _i32, _i32]),
    "npfn_set_estimator_set": (ctypes.c_int, [_vp, _i32, _i32, _i32]),
    "npfn_forward_targets": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "npfn_forward_logits": (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "npfn_head_sample": (ctypes.c_int, [_vp, _vp, _i32, _i64, _u64, _i64, _vp, _vp, _f, _vp]),
    "npfn_ar_fit_begin": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "npfn_ar_fit_step": (ctypes.c_int, [_vp, _i32, _vp]),
    "npfn_set_fit_token": (ctypes.c_int, [_vp, _u64]),
    "npfn_set_fit_cache": (ctypes.c_int, [_vp, _i32, _u64]),
    "npfn_fit_cache_stats": (ctypes.c_int, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_i32),
                                            ctypes.POINTER(_u64)]),
    "npfn_fit_cache_clear": (ctypes.c_int, [_vp]),
    "npfn_set_chunk_rows": (ctypes.c_int, [_vp, _i64]),
    "npfn_prof_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "npfn_prof_read": (ctypes.c_int, [_vp, ctypes.POINTER(NpfnProfEntry), _i32, ctypes.POINTER(_i32)]),
    "npfn_debug_views": (ctypes.c_int, [_vp, _vp, _i64, _i32, ctypes.POINTER(_i32)]),
    "npfn_debug_target_translation": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, ctypes.POINTER(_i32), _vp, _vp,
                                                     ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "npfn_mix_rows": (ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i32, _i32, _f, ctypes.POINTER(_i32), _vp, _vp, _i32,
                                     _vp, _vp, _u64, _u64, _i64, _u64, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _f,
                                     _vp]),
    "npfn_debug_item_attn_online": (ctypes.c_int, [ctypes.c_int]),
    "npfn_debug_item_attn_scale": (ctypes.c_int, [_f]),
    "npfn_debug_fail_row_launch": (ctypes.c_int, [_vp, _i32]),
    "npfn_item_attn_fallback": (ctypes.c_int, [_vp, ctypes.POINTER(_u64), ctypes.c_int]),
    "npfn_item_attn_fallback_causes": (ctypes.c_int, [_vp, ctypes.POINTER(_u64)]),
}

_LIB = None


class EngineError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libnpfn.so and declare every entry point (raises if missing).

    NPFN_LIB overrides the path (diagnostic builds, e.g. a ``-DNPFN_DIAG_*`` timing build, or an older build in an
    A/B run, which may lack entry points added since: those are left unbound)."""
    global _LIB
    override = path is None and bool(os.environ.get("NPFN_LIB"))
    path = path or os.environ.get("NPFN_LIB") or LIB_PATH
    if _LIB is not None and _LIB._name == path:
        return _LIB
    if not os.path.exists(path):
        raise ImportError(
            f"NPE-PFN engine library not found at {path}; build it with `make -C npe-pfn_amd` "
            "(or __graft_entry__.build()). There is no CPU fallback."
        )
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if override and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check(lib, rc: int, what: str):
    if rc != 0:
        msg = lib.npfn_last_error()
        raise EngineError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _dev_f32(t, device) -> torch.Tensor:
    t = torch.as_tensor(t)
    return t.to(device=device, dtype=torch.float32).contiguous()


MMD_KERNELS = {"rbf": 0, "multiscale": 1}   # npfn_mmd_sums' kernel codes
MMD_MAX_POOL, MMD_MAX_DIM, MMD_MAX_BANDWIDTHS, MMD_MAX_LABELLINGS = 32768, 64, 8, 4096


def check_mmd_args(z_shape, labels_shape, kernel, bandwidths) -> Tuple[int, list]:
    """(kernel code, bandwidths as floats) of an mmd_sums call on ``z`` [n_obs, N, dim] and
    ``labels`` [n_label, N]; ValueError for whatever npfn_mmd_sums would refuse.  Pure host logic,
    shared by :func:`mmd_sums` and :func:`npe_pfn.diagnostics.mmd_sums_host`."""
    if kernel not in MMD_KERNELS and kernel not in (0, 1):
        raise ValueError(f"mmd_sums: kernel must be 'rbf' (0) or 'multiscale' (1), got {kernel!r}")
    code = MMD_KERNELS.get(kernel, kernel)
    if len(z_shape) != 3 or not 1 <= z_shape[1] <= MMD_MAX_POOL or not 1 <= z_shape[2] <= MMD_MAX_DIM:
        raise ValueError(f"mmd_sums: z {tuple(z_shape)} is not [n_obs, 1 <= N <= {MMD_MAX_POOL}, 1 <= dim <= "
                         f"{MMD_MAX_DIM}]")
    if len(labels_shape) != 2 or labels_shape[1] != z_shape[1] or not 1 <= labels_shape[0] <= MMD_MAX_LABELLINGS:
        raise ValueError(f"mmd_sums: labels {tuple(labels_shape)} is not [1 <= n_label <= {MMD_MAX_LABELLINGS}, "
                         f"{z_shape[1]}]")
    bw = [float(a) for a in np.asarray(bandwidths, dtype=np.float64).reshape(-1)]
    if not 1 <= len(bw) <= MMD_MAX_BANDWIDTHS or not all(math.isfinite(a) and a > 0 for a in bw):
        raise ValueError(f"mmd_sums: need 1..{MMD_MAX_BANDWIDTHS} finite bandwidths > 0, got {bw}")
    return int(code), bw


def mmd_sums(z, labels, kernel, bandwidths, lib=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """npfn_mmd_sums on the GPU that holds ``z`` (needs no engine): ``(sums [n_obs, n_label, 2]
    int64, total [n_obs] int64, bad [n_obs] int32)`` on that device, on its current stream.  ``z``
    [n_obs, N, dim] is every observation's pooled sample, ``labels`` [n_label, N] (bool / uint8)
    marks group X per labelling, ``kernel`` is "rbf" / "multiscale" (or 0 / 1), ``bandwidths`` the
    a_b.  sums[u, p, 0] / [u, p, 1] are the fixed-point kernel sums over the ordered pairs inside
    group X / inside its complement, total[u] the sum over all pairs; the definition of every
    number: :func:`npe_pfn.diagnostics.mmd_sums_host`.  ValueError for arguments that do not fit,
    before the C call."""
    z = torch.as_tensor(z)
    if z.device.type != "cuda":
        raise ValueError("mmd_sums: z must live on the GPU (npe_pfn.diagnostics.mmd_sums_host is the CPU statement)")
    z = z.to(torch.float32).contiguous()
    labels = torch.as_tensor(labels)
    code, bw = check_mmd_args(z.shape, labels.shape, kernel, bandwidths)
    labels = (labels != 0).to(device=z.device, dtype=torch.uint8).contiguous()
    n_obs, N, dim = z.shape
    P = labels.shape[0]
    sums = torch.empty((n_obs, P, 2), dtype=torch.int64, device=z.device)
    total = torch.empty((n_obs,), dtype=torch.int64, device=z.device)
    bad = torch.empty((n_obs,), dtype=torch.int32, device=z.device)
    lib = lib or load_library()
    host_bw = (ctypes.c_float * len(bw))(*bw)
    with torch.cuda.device(z.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(z.device).cuda_stream)
        _check(lib, lib.npfn_mmd_sums(_ptr(z), n_obs, N, dim, code, ctypes.cast(host_bw, _vp), len(bw), _ptr(labels),
                                      P, _ptr(sums), _ptr(total),
                                      ctypes.cast(ctypes.c_void_p(bad.data_ptr()), ctypes.POINTER(_i32)), stream),
               "npfn_mmd_sums")
    return sums, total, bad


W2_MAX_N, W2_MAX_DIM, W2_MAX_IMAGE = 2048, 64, 32768   # npfn_w2_assign's caps (n * dim <= the image)


def check_transport_args(a_shape, b_shape) -> Tuple[int, int, int]:
    """(n_obs, n, dim) of a w2_assign call on ``a`` and ``b`` [n_obs, n, dim]; ValueError for
    whatever npfn_w2_assign would refuse, and for two sets of unequal size.  Pure host logic,
    shared by :func:`w2_assign` and :func:`npe_pfn.diagnostics.transport_costs_host`."""
    a_shape, b_shape = tuple(a_shape), tuple(b_shape)
    if len(a_shape) != 3 or len(b_shape) != 3 or a_shape[0] != b_shape[0] or a_shape[2] != b_shape[2]:
        raise ValueError(f"w2_assign: a {a_shape} and b {b_shape} are not both [n_obs, n, dim]")
    if a_shape[1] != b_shape[1]:
        raise ValueError(f"w2_assign: a has {a_shape[1]} points and b {b_shape[1]}: uniform transport between sets "
                         "of unequal size is not an assignment (an optimal plan splits mass), and the reference "
                         "harness always compares sets of equal size")
    n_obs, n, dim = a_shape
    if not 1 <= n <= W2_MAX_N or not 1 <= dim <= W2_MAX_DIM or n * dim > W2_MAX_IMAGE:
        raise ValueError(f"w2_assign: a {a_shape} is not [n_obs, 1 <= n <= {W2_MAX_N}, 1 <= dim <= {W2_MAX_DIM}] with "
                         f"n * dim <= {W2_MAX_IMAGE}")
    return n_obs, n, dim


def w2_assign(a, b, scale, lib=None):
    """npfn_w2_assign on the GPU that holds ``a`` (needs no engine): ``(assign [n_obs, n] int32,
    duals [n_obs, 2, n] int64, cost_sum [n_obs] int64, steps [n_obs] int64, bad [n_obs] int32)``
    on that device, on its current stream.  ``a`` and ``b`` [n_obs, n, dim] are the two sets of
    every observation, ``scale`` [n_obs] float64 its power of two
    (:func:`npe_pfn.diagnostics.transport_scale`).  The exact assignment under the integer costs
    round(d2 * scale); the definition of every number:
    :func:`npe_pfn.diagnostics.transport_costs_host` and
    :func:`npe_pfn.diagnostics.assignment_solve_host`.  ValueError for arguments that do not fit,
    before the C call."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.device.type != "cuda":
        raise ValueError("w2_assign: a must live on the GPU (npe_pfn.diagnostics.assignment_solve_host is the CPU "
                         "statement)")
    n_obs, n, dim = check_transport_args(a.shape, b.shape)
    scale = torch.as_tensor(scale)
    if tuple(scale.shape) != (n_obs,):
        raise ValueError(f"w2_assign: scale {tuple(scale.shape)} is not [{n_obs}]")
    a = a.to(torch.float32).contiguous()
    b = b.to(device=a.device, dtype=torch.float32).contiguous()
    scale = scale.to(device=a.device, dtype=torch.float64).contiguous()
    assign = torch.empty((n_obs, n), dtype=torch.int32, device=a.device)
    duals = torch.empty((n_obs, 2, n), dtype=torch.int64, device=a.device)
    cost_sum = torch.empty((n_obs,), dtype=torch.int64, device=a.device)
    steps = torch.empty((n_obs,), dtype=torch.int64, device=a.device)
    bad = torch.empty((n_obs,), dtype=torch.int32, device=a.device)
    lib = lib or load_library()
    i32p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(_i32))  # noqa: E731
    with torch.cuda.device(a.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _check(lib, lib.npfn_w2_assign(_ptr(a), _ptr(b), n_obs, n, dim, _ptr(scale), i32p(assign), _ptr(duals),
                                       _ptr(cost_sum), _ptr(steps), i32p(bad), stream), "npfn_w2_assign")
    return assign, duals, cost_sum, steps, bad


# npfn_c2st_fit's caps: a workgroup holds 16384 parameters in layers of at most 128 units
C2ST_MAX_DIM, C2ST_MAX_POOL, C2ST_MAX_LAYERS, C2ST_MAX_WIDTH, C2ST_MAX_PARAMS = 64, 32768, 5, 128, 16384
C2ST_MAX_FOLDS, C2ST_MAX_BATCH = 16, 4096
C2ST_BETAS, C2ST_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam's defaults


def c2st_param_count(widths) -> int:
    """Parameters of the MLP with these layer widths: sum of out * (in + 1)."""
    return sum(int(o) * (int(i) + 1) for i, o in zip(widths[:-1], widths[1:]))


def check_c2st_args(z_shape, n_first, widths, n_folds, epochs, batch_size) -> Tuple[int, int, int, int]:
    """(n_obs, n_pool, dim, P) of a c2st_fit call on ``z`` [n_obs, n_pool, dim]; ValueError for
    whatever npfn_c2st_fit would refuse.  Pure host logic, shared by :func:`c2st_fit` and
    :func:`npe_pfn.diagnostics.c2st_fit_host`."""
    z_shape = tuple(z_shape)
    if len(z_shape) != 3 or not 1 <= z_shape[2] <= C2ST_MAX_DIM:
        raise ValueError(f"c2st_fit: z {z_shape} is not [n_obs, n_pool, 1 <= dim <= {C2ST_MAX_DIM}]")
    n_obs, n_pool, dim = z_shape
    if not 2 <= n_pool <= C2ST_MAX_POOL or not 1 <= int(n_first) <= n_pool - 1:
        raise ValueError(f"c2st_fit: need 2 <= n_pool <= {C2ST_MAX_POOL} and 1 <= n_first <= n_pool - 1, got "
                         f"{n_pool} and {n_first}")
    widths = [int(w) for w in widths]
    if not 1 <= len(widths) - 1 <= C2ST_MAX_LAYERS or widths[0] != dim or widths[-1] != 2 \
            or not all(1 <= w <= C2ST_MAX_WIDTH for w in widths):
        raise ValueError(f"c2st_fit: widths {widths} are not 1..{C2ST_MAX_LAYERS} layers from dim = {dim} to 2 "
                         f"logits with every width in 1..{C2ST_MAX_WIDTH}")
    P = c2st_param_count(widths)
    if P > C2ST_MAX_PARAMS:
        raise ValueError(f"c2st_fit: widths {widths} have {P} parameters, above the {C2ST_MAX_PARAMS} that one "
                         "workgroup holds ('mlp' reaches dim 11, 'mlp_small' dim 28, 'linear' dim 64)")
    if not 2 <= int(n_folds) <= C2ST_MAX_FOLDS or int(epochs) < 1:
        raise ValueError(f"c2st_fit: need 2 <= n_folds <= {C2ST_MAX_FOLDS} and epochs >= 1, got {n_folds} and {epochs}")
    if not 1 <= int(batch_size) <= C2ST_MAX_BATCH:
        raise ValueError(f"c2st_fit: batch_size must lie in 1..{C2ST_MAX_BATCH}, got {batch_size}")
    return n_obs, n_pool, dim, P


def c2st_fit(z, n_first, fold, order, widths, init, epochs, batch_size=128, lr=1e-3, weight_decay=0.0,
             return_probs=True, return_params=False, lib=None):
    """npfn_c2st_fit on the GPU that holds ``z`` (needs no engine): ``(correct [n_obs, n_folds]
    int32, loss [n_obs, n_folds, epochs], prob [n_obs, n_pool] or None, params [n_obs, n_folds, P]
    or None, bad [n_obs] int32)`` on that device, on its current stream.  ``z`` [n_obs, n_pool, dim]
    is every observation's pooled sample (label 0 for the first ``n_first`` points), ``fold``
    [n_pool] the fold that holds each point out (:func:`npe_pfn.diagnostics.c2st_folds`), ``order``
    [epochs, n_pool] one permutation per epoch (:func:`npe_pfn.diagnostics.c2st_order`), ``widths``
    and ``init`` the network and its start (``c2st_widths``, ``c2st_init``).  Here ``order`` is
    compacted per fold (a stable boolean mask on the device drops the fold's own points), so the
    kernel trains on consecutive runs of ``batch_size`` entries.  The definition of every number:
    :func:`npe_pfn.diagnostics.c2st_fit_host`.  At most 16384 parameters in layers of at most 128
    units.  ValueError for arguments that do not fit, before the C call."""
    from .diagnostics import c2st_adam_table

    z = torch.as_tensor(z)
    if z.device.type != "cuda":
        raise ValueError("c2st_fit: z must live on the GPU (npe_pfn.diagnostics.c2st_fit_host is the CPU statement)")
    z = z.to(torch.float32).contiguous()
    fold_cpu = torch.as_tensor(fold).detach().cpu().to(torch.int64)
    n_folds = int(fold_cpu.max()) + 1 if fold_cpu.numel() else 0
    epochs, batch_size = int(epochs), int(batch_size)
    n_obs, n_pool, dim, P = check_c2st_args(z.shape, n_first, widths, n_folds, epochs, batch_size)
    order = torch.as_tensor(order)
    init = torch.as_tensor(init)
    if tuple(fold_cpu.shape) != (n_pool,) or tuple(order.shape) != (epochs, n_pool) or tuple(init.shape) != (P,):
        raise ValueError(f"c2st_fit: fold {tuple(fold_cpu.shape)}, order {tuple(order.shape)} and init "
                         f"{tuple(init.shape)} are not [{n_pool}], [{epochs}, {n_pool}] and [{P}]")
    held = torch.bincount(fold_cpu, minlength=n_folds)
    n_train = [n_pool - int(h) for h in held]
    if min(n_train) < 1:
        raise ValueError("c2st_fit: a fold holds every point out")
    dev = z.device
    fold_d = fold_cpu.to(device=dev, dtype=torch.uint8).contiguous()
    order_d = order.to(device=dev, dtype=torch.int64).clamp(0, n_pool - 1)
    order_ld = max(n_train)
    packed = torch.zeros((n_folds, epochs, order_ld), dtype=torch.int32, device=dev)
    of = fold_d[order_d]
    for f in range(n_folds):
        packed[f, :, :n_train[f]] = order_d[of != f].view(epochs, n_train[f]).to(torch.int32)
    n_steps = epochs * ((order_ld + batch_size - 1) // batch_size)
    adam = c2st_adam_table(lr, n_steps).to(dev).contiguous()
    init_d = init.to(device=dev, dtype=torch.float32).contiguous()
    correct = torch.empty((n_obs, n_folds), dtype=torch.int32, device=dev)
    loss = torch.empty((n_obs, n_folds, epochs), dtype=torch.float32, device=dev)
    prob = torch.empty((n_obs, n_pool), dtype=torch.float32, device=dev) if return_probs else None
    params = torch.empty((n_obs, n_folds, P), dtype=torch.float32, device=dev) if return_params else None
    bad = torch.empty((n_obs,), dtype=torch.int32, device=dev)
    lib = lib or load_library()
    host_w = (_i32 * len(widths))(*[int(w) for w in widths])
    host_nt = (_i32 * n_folds)(*n_train)
    i32p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), ctypes.POINTER(_i32))  # noqa: E731
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib, lib.npfn_c2st_fit(_ptr(z), n_obs, n_pool, int(n_first), dim, host_w, len(widths) - 1, _ptr(init_d),
                                      _ptr(fold_d), n_folds, i32p(packed), host_nt, order_ld, epochs, batch_size,
                                      _ptr(adam), C2ST_BETAS[0], C2ST_BETAS[1], C2ST_EPS, float(weight_decay),
                                      i32p(correct), _ptr(loss), _ptr(prob), _ptr(params), i32p(bad), stream),
               "npfn_c2st_fit")
    return correct, loss, prob, params, bad


MIX_OPS = {"log": 0, "prob": 1, "sample": 2, "nll": 3, "score": 4,   # npfn.h NPFN_MIX_*
           "group_sample": 5, "group_nll": 6, "group_score": 7}


def pack_translation(idx, share, tcancel, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device buffers of a translation table as npfn_mix_rows reads them: ``tab`` [n_bars + 1, 2]
    int32 (idx, the bits of the float32 share) and ``tcancel`` padded to n_bars + 4 bytes."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    share = np.ascontiguousarray(share, dtype=np.float32)
    tc = np.ascontiguousarray(tcancel, dtype=np.uint8)
    if idx.ndim != 1 or share.shape != idx.shape or tc.shape != (idx.shape[0] - 1,):
        raise ValueError(f"pack_translation: idx {idx.shape}, share {share.shape} and tcancel {tc.shape} are not "
                         "[n_bars + 1], [n_bars + 1] and [n_bars]")
    tab = np.stack([idx, share.view(np.int32)], axis=1)
    return (torch.from_numpy(tab).to(device), torch.from_numpy(np.concatenate([tc, np.zeros(4, np.uint8)])).to(device))


def mix_rows(op: str, logits: torch.Tensor, *, n_bars: Optional[int] = None, inv_temperature: float = 1.0,
             ett=None, tab: Optional[torch.Tensor] = None, tcancel: Optional[torch.Tensor] = None, geo: bool = False,
             bz: Optional[torch.Tensor] = None, ystats: Optional[torch.Tensor] = None, seed: int = 0,
             counter: int = 0, row_offset: int = 0, philox_row0: int = 0, per: int = 1,
             feat: Optional[torch.Tensor] = None, col: int = 0, out0: Optional[torch.Tensor] = None,
             out1: Optional[torch.Tensor] = None, ldo: Optional[int] = None, row0: int = 0,
             n_rows: Optional[int] = None, log_eps: float = math.log(1e-15), lib=None):
    """npfn_mix_rows (include/npfn.h; needs no engine) on the GPU that holds ``logits``: fp16
    [n_est, ld_rows, n_bars] for the mix ops, a float32 "prob" result [*, n_bars] for the group
    ops.  ``tab`` / ``tcancel`` come from :func:`pack_translation`, ``ett`` is a list or an int32
    device tensor.  "log" and "prob" allocate and return their output; the tails write ``feat``
    [*, ldf] / ``out0`` / ``out1`` in place and return ``(out0, out1)``.  The C call's own
    argument checks are the only ones."""
    code = MIX_OPS[op]
    group = code >= 5
    dev = logits.device
    lib = lib or load_library()
    if group:
        nb = logits.shape[-1]
        E, ld_rows = 1, 0
        if n_rows is None:
            raise ValueError("mix_rows: the group ops need n_rows")
    else:
        E, ld_rows, nb = logits.shape
        if n_rows is None:
            n_rows = ld_rows - row0
    if n_bars is not None:
        nb = n_bars
    if isinstance(ett, (list, tuple, np.ndarray)):
        ett = torch.as_tensor(np.asarray(ett, dtype=np.int32)).to(dev)
    if code == 0 and out0 is None:
        ldo = nb if ldo is None else ldo
        out0 = torch.empty((n_rows, ldo), dtype=torch.float32, device=dev)
    if code == 1 and out0 is None:
        out0 = torch.empty((n_rows, nb), dtype=torch.float32, device=dev)
    ldo = (nb if code == 0 else 1) if ldo is None else ldo
    ldf = feat.shape[-1] if feat is not None else 1
    ettp = None if ett is None else ctypes.cast(ctypes.c_void_p(ett.data_ptr()), ctypes.POINTER(_i32))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib, lib.npfn_mix_rows(code, _ptr(logits), ld_rows, row0, n_rows, E, nb, float(inv_temperature), ettp,
                                      _ptr(tab), _ptr(tcancel), int(geo), _ptr(bz), _ptr(ystats),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter), int(row_offset), int(philox_row0),
                                      int(per), _ptr(feat), ldf, int(col), _ptr(out0), _ptr(out1), int(ldo),
                                      float(log_eps), stream), "npfn_mix_rows")
    return out0 if code <= 1 else (out0, out1)


MAX_QUANTILES = 64  # npfn_bar_stats / npfn_predict_stats take at most this many levels per call


def check_quantiles(quantiles) -> list:
    """The quantile levels of a bar_stats / predict_stats call as a list of floats; ValueError
    for a level outside [0, 1] (NaN included) or more than MAX_QUANTILES of them.  Pure host
    logic: callers run it before any engine is touched."""
    qs = [float(q) for q in np.asarray(list(quantiles) if quantiles is not None else [], dtype=np.float64).reshape(-1)]
    if len(qs) > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} quantiles per call, got {len(qs)}")
    for q in qs:
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"quantiles must lie in [0, 1], got {q!r}")
    return qs


class Engine:
    """One engine handle on one device: weights resident in HBM, fit state, workspaces."""

    def __init__(self, cfg: ModelConfig = ModelConfig(), weights: Optional[Dict[str, np.ndarray]] = None,
                 device: Optional[torch.device] = None, random_state: int = 0, preprocessing: str = "ensemble"):
        """``preprocessing``: the engine's per-estimator preprocessing (:meth:`set_preprocessing`);
        the default "ensemble" is tabpfn's default and the C engine's initial mode, as for
        ``TabPFNRegressor`` (npe_pfn/tabpfn.py)."""
        if not torch.cuda.is_available():
            raise EngineError("the NPE-PFN engine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = load_library()
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise EngineError(f"engine device must be a GPU, got {self.device}")
        check_n_bars(cfg.n_bars)
        if weights is None:
            weights = synthetic_weights(cfg, seed=0)
        blob = _packed(weights, cfg)
        self.c_cfg = NpfnConfig(cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.d_ff, cfg.n_bars,
                                cfg.features_per_group, cfg.max_groups, cfg.n_estimators,
                                float(cfg.softmax_temperature), self.device.index or 0,
                                int(random_state) & 0xFFFFFFFFFFFFFFFF)
        want = self.lib.npfn_weights_size(ctypes.byref(self.c_cfg))
        if want != blob.size:
            raise EngineError(f"weight blob has {blob.size} floats, engine expects {want}")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.npfn_engine_create(ctypes.byref(self.c_cfg), blob.ctypes.data_as(ctypes.c_void_p),
                                                         blob.size, ctypes.byref(h)), "npfn_engine_create")
        self.h = h
        self.random_state = int(random_state)
        self.n_features: Optional[int] = None
        self.n_classes = 0
        self.preprocessing = self.DEFAULT_PREPROCESSING  # npfn_engine_create starts in mode 3
        self.e0, self.ne = 0, cfg.n_estimators
        self.ep_set = None  # (rank, count, stride) of npe_pfn.distributed's estimator-parallel split
        if preprocessing != self.preprocessing:
            self.set_preprocessing(preprocessing)

    def full_range(self) -> None:
        """Back to all estimators after an estimator-parallel split (the single-engine entry
        points need the whole ensemble)."""
        if self.e0 != 0 or self.ne != self.cfg.n_estimators:
            self.set_estimator_range(0, self.cfg.n_estimators)

    PREPROCESSING_MODES = {"none": 0, "quantile": 1, "quantile+power": 2, "ensemble": 3}
    DEFAULT_PREPROCESSING = "ensemble"

    def set_preprocessing(self, mode: str) -> None:
        """Per-estimator preprocessing from the next fit on (include/npfn.h
        ``npfn_set_preprocessing``): "none"; "quantile" = sklearn QuantileTransformer
        (uniform, n_quantiles=max(n//5, 2)) on even estimators [ext: tabpfn "quantile_uni"];
        "quantile+power" = that plus the Yeo-Johnson power transform on odd estimators
        [ext: tabpfn "safepower"]; "ensemble" = tabpfn's default regressor ensemble
        (quantile + original + SVD | Yeo-Johnson features, fingerprint feature, Yeo-Johnson
        target transform on half the estimators; oracle/preprocess_oracle.py MODE_ENSEMBLE)."""
        if mode not in self.PREPROCESSING_MODES:
            raise ValueError(f"preprocessing must be one of {sorted(self.PREPROCESSING_MODES)}, got {mode!r}")
        _check(self.lib, self.lib.npfn_set_preprocessing(self.h, self.PREPROCESSING_MODES[mode]),
               "npfn_set_preprocessing")
        self.preprocessing = mode
        self.n_features = None

    def set_average_before_softmax(self, enable: bool) -> None:
        """tabpfn's ``average_before_softmax`` (npfn_set_average_before_softmax): the ensemble is
        mixed as softmax(mean of the estimators' log probabilities) instead of the mean of their
        probabilities, from the next predict / AR call on."""
        _check(self.lib, self.lib.npfn_set_average_before_softmax(self.h, 1 if enable else 0),
               "npfn_set_average_before_softmax")
        self.average_before_softmax = bool(enable)

    def check_table(self, n_rows: int, n_features: int, classifier: bool = False) -> None:
        """ValueError naming the limit when a fit on [n_rows, n_features] exceeds the engine's
        capacity under its preprocessing (npe_pfn.limits; raised before any C call)."""
        check_engine_table(int(n_rows), int(n_features), self.PREPROCESSING_MODES[self.preprocessing], classifier,
                           self.cfg.max_groups)

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.lib.npfn_engine_destroy(h)
            except Exception:
                pass
            self.h = None

    @property
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------ TabPFN surface
    def fit(self, X, y) -> None:
        """npfn_fit of this engine's estimator set (a partial set is a building block of the
        estimator-parallel split: fit + forward_targets; the mixing calls need the full set)."""
        X = _dev_f32(X, self.device)
        y = _dev_f32(y, self.device).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError(f"fit: X {tuple(X.shape)} and y {tuple(y.shape)} do not match")
        self.check_table(X.shape[0], X.shape[1])
        _check(self.lib, self.lib.npfn_fit(self.h, _ptr(X), X.shape[1], _ptr(y), 1, X.shape[0], X.shape[1],
                                           self.stream), "npfn_fit")
        self.n_features = X.shape[1]
        self._keep = (X, y)  # inputs stay alive until the stream consumed them

    def predict_logits(self, Xq) -> torch.Tensor:
        if self.n_features is None:
            raise EngineError("predict before fit")
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or Xq.shape[1] != self.n_features:
            raise ValueError(f"predict: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        out = torch.empty((Xq.shape[0], self.cfg.n_bars), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_predict(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], _ptr(out), self.stream),
               "npfn_predict")
        return out

    # -------------------------------------------------------- classifier surface
    def fit_classes(self, X, y_idx, n_classes: int) -> None:
        """Classifier fit on label indices 0..n_classes-1 (npfn_fit_classes)."""
        self.full_range()
        X = _dev_f32(X, self.device)
        y = _dev_f32(y_idx, self.device).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError(f"fit: X {tuple(X.shape)} and y {tuple(y.shape)} do not match")
        self.check_table(X.shape[0], X.shape[1], classifier=True)
        _check(self.lib, self.lib.npfn_fit_classes(self.h, _ptr(X), X.shape[1], _ptr(y), 1, X.shape[0], X.shape[1],
                                                   int(n_classes), self.stream), "npfn_fit_classes")
        self.n_features = X.shape[1]
        self.n_classes = int(n_classes)
        self._keep = (X, y)

    def predict_proba(self, Xq) -> torch.Tensor:
        """[N, n_classes] estimator-mean class probabilities on the device (npfn_predict_proba)."""
        if self.n_features is None or not getattr(self, "n_classes", 0):
            raise EngineError("predict_proba before fit_classes")
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or Xq.shape[1] != self.n_features:
            raise ValueError(f"predict_proba: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        out = torch.empty((Xq.shape[0], self.n_classes), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_predict_proba(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], _ptr(out),
                                                     self.stream), "npfn_predict_proba")
        return out

    def borders(self) -> torch.Tensor:
        out = torch.empty(self.cfg.n_bars + 1, dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_get_borders(self.h, _ptr(out), self.stream), "npfn_get_borders")
        return out

    def bar_sample(self, logits: torch.Tensor, borders: torch.Tensor, counter: int) -> torch.Tensor:
        logits = _dev_f32(logits, self.device)
        borders = _dev_f32(borders, self.device)
        out = torch.empty(logits.shape[0], dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_bar_sample(_ptr(logits), _ptr(borders), logits.shape[0], logits.shape[1],
                                                  self.random_state, int(counter), _ptr(out), self.stream),
               "npfn_bar_sample")
        return out

    def bar_nll(self, logits: torch.Tensor, borders: torch.Tensor, y) -> torch.Tensor:
        logits = _dev_f32(logits, self.device)
        borders = _dev_f32(borders, self.device)
        y = _dev_f32(y, self.device).reshape(-1)
        out = torch.empty(logits.shape[0], dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_bar_nll(_ptr(logits), _ptr(borders), _ptr(y), logits.shape[0],
                                               logits.shape[1], _ptr(out), self.stream), "npfn_bar_nll")
        return out

    def bar_cdf(self, logits: torch.Tensor, borders: torch.Tensor, y) -> torch.Tensor:
        """npfn_bar_cdf: F(y_i) of the full-support bar distribution of each row of ``logits``
        [N, n_bars] (half-normal tail bars, the density of :meth:`bar_nll`), [N] on the device."""
        logits = _dev_f32(logits, self.device)
        borders = _dev_f32(borders, self.device)
        y = _dev_f32(y, self.device).reshape(-1)
        if logits.ndim != 2 or borders.shape != (logits.shape[1] + 1,) or y.shape[0] != logits.shape[0]:
            raise ValueError(f"bar_cdf: logits {tuple(logits.shape)}, borders {tuple(borders.shape)} and y "
                             f"{tuple(y.shape)} do not match")
        out = torch.empty(logits.shape[0], dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_bar_cdf(_ptr(logits), _ptr(borders), _ptr(y), logits.shape[0],
                                               logits.shape[1], _ptr(out), self.stream), "npfn_bar_cdf")
        return out

    def _stats_buffers(self, n_rows: int, quantiles, mean: bool, mode: bool):
        qs = check_quantiles(quantiles)
        q = torch.tensor(qs, dtype=torch.float32).to(self.device) if qs else None
        m = torch.empty(n_rows, dtype=torch.float32, device=self.device) if mean else None
        md = torch.empty(n_rows, dtype=torch.float32, device=self.device) if mode else None
        qo = torch.empty((len(qs), n_rows), dtype=torch.float32, device=self.device) if qs else None
        return qs, q, m, md, qo

    @staticmethod
    def _stats_dict(m, md, qo) -> Dict[str, torch.Tensor]:
        out = {}
        if m is not None:
            out["mean"] = m
        if md is not None:
            out["mode"] = md
        if qo is not None:
            out["quantiles"] = qo
        return out

    def bar_stats(self, logits: torch.Tensor, borders: torch.Tensor, quantiles=(), mean: bool = True,
                  mode: bool = True) -> Dict[str, torch.Tensor]:
        """npfn_bar_stats: the bar distribution's summaries of each row of ``logits`` [N, n_bars] --
        ``{"mean": [N], "mode": [N], "quantiles": [len(quantiles), N]}`` on the device (a key is
        absent when its statistic was not asked for); the median is the quantile 0.5."""
        logits = _dev_f32(logits, self.device)
        borders = _dev_f32(borders, self.device)
        if logits.ndim != 2 or borders.shape != (logits.shape[1] + 1,):
            raise ValueError(f"bar_stats: logits {tuple(logits.shape)} and borders {tuple(borders.shape)} do not match")
        qs, q, m, md, qo = self._stats_buffers(logits.shape[0], quantiles, mean, mode)
        _check(self.lib, self.lib.npfn_bar_stats(_ptr(logits), _ptr(borders), logits.shape[0], logits.shape[1],
                                                 _ptr(q), len(qs), _ptr(m), _ptr(md), _ptr(qo), self.stream),
               "npfn_bar_stats")
        return self._stats_dict(m, md, qo)

    def predict_stats(self, Xq, quantiles=(), mean: bool = True, mode: bool = True) -> Dict[str, torch.Tensor]:
        """npfn_predict_stats: the summaries of :meth:`bar_stats` for the predictive distribution of
        every query row, 8192 rows at a time inside the engine: the [N, n_bars] fp32 logits of
        :meth:`predict_logits` are never allocated."""
        qs = check_quantiles(quantiles)
        if self.n_features is None:
            raise EngineError("predict_stats before fit")
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or Xq.shape[1] != self.n_features:
            raise ValueError(f"predict_stats: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        qs, q, m, md, qo = self._stats_buffers(Xq.shape[0], qs, mean, mode)
        _check(self.lib, self.lib.npfn_predict_stats(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], _ptr(q), len(qs),
                                                     _ptr(m), _ptr(md), _ptr(qo), self.stream),
               "npfn_predict_stats")
        return self._stats_dict(m, md, qo)

    # -------------------------------------------------------------- fused paths
    def _ar_ctx(self, who: str, x_ctx, theta_ctx, matched: bool = True):
        """``(x_ctx, theta_ctx, n, dim_x, dim_theta)`` of an AR call, the tables on the device;
        ``matched``: they must be matrices of equal row counts."""
        x_ctx = _dev_f32(x_ctx, self.device)
        theta_ctx = _dev_f32(theta_ctx, self.device)
        if matched and (x_ctx.ndim != 2 or theta_ctx.ndim != 2 or theta_ctx.shape[0] != x_ctx.shape[0]):
            raise ValueError(f"{who}: x_ctx {tuple(x_ctx.shape)} and theta_ctx {tuple(theta_ctx.shape)} do not match")
        n, dx = x_ctx.shape
        return x_ctx, theta_ctx, n, dx, theta_ctx.shape[1]

    def _ar_unique(self, who: str, x_unique, N: int, dx: int, one_each: bool = False, of: bool = True):
        """``(x_unique, U)``: the U distinct query rows, on the device, that repeat into N rows of
        dx columns; ``one_each``: N >= U as well."""
        x_unique = _dev_f32(x_unique, self.device)
        U = x_unique.shape[0] if x_unique.ndim == 2 else 0
        if x_unique.ndim != 2 or x_unique.shape[1] != dx or U < 1 or (one_each and N < U) or N % U:
            raise ValueError(f"{who}: x_unique {tuple(x_unique.shape)} does not repeat into {N} rows"
                             + (f" of {dx}" if of else ""))
        return x_unique, U

    def ar_sample(self, x_ctx, theta_ctx, x_query, counter: int, with_log_prob: bool = False,
                  eps: float = 1e-15, row_base: int = 0,
                  x_unique: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``x_unique``: the distinct rows of ``x_query`` when ``x_query`` is
        ``x_unique.repeat_interleave(N // U, 0)`` (one observation repeated, or sample_batched's
        obs-major batch): npfn_ar_sample_repeated runs AR step 0 once per distinct row."""
        self.full_range()
        x_ctx, theta_ctx, n, dx, dth = self._ar_ctx("ar_sample", x_ctx, theta_ctx, matched=False)
        N = x_query.shape[0]
        if theta_ctx.shape[0] != n or x_query.shape[1] != dx:
            raise ValueError("ar_sample: inconsistent shapes")
        self.check_table(n, dx + dth - 1)
        theta = torch.empty((N, dth), dtype=torch.float32, device=self.device)
        lp = torch.empty(N, dtype=torch.float32, device=self.device) if with_log_prob else None
        if x_unique is not None:
            x_unique, U = self._ar_unique("ar_sample", x_unique, N, dx)
            _check(self.lib, self.lib.npfn_ar_sample_repeated(
                self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_unique), U, N, int(counter), int(row_base),
                _ptr(theta), _ptr(lp), float(eps), self.stream), "npfn_ar_sample_repeated")
        else:
            x_query = _dev_f32(x_query, self.device)
            _check(self.lib, self.lib.npfn_ar_sample(self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_query),
                                                     N, int(counter), int(row_base), _ptr(theta), _ptr(lp),
                                                     float(eps), self.stream),
                   "npfn_ar_sample")
        self.n_features = dx + dth - 1
        return theta, lp

    def ar_marginals(self, x_ctx, theta_ctx, x_unique, n_rows: int, counter: int, with_log_prob: bool = False,
                     eps: float = 1e-15, row_base: int = 0):
        """npfn_ar_marginals: :meth:`ar_sample` over ``x_unique.repeat_interleave(n_rows // U, 0)``
        that also averages, per observation and step, the mixtures the draws were taken from.
        Returns ``(theta [n_rows, dim_theta], log_prob [n_rows] or None, probs [U, dim_theta,
        n_bars], borders [dim_theta, n_bars + 1])`` on the device; ``theta`` and ``log_prob`` are
        bit for bit those of :meth:`ar_sample` with the same counter and row_base.
        ``probs[u, k]`` are the bar masses of the marginal of theta_k given ``x_unique[u]`` on
        ``borders[k]``: the mean over the observation's draws of their conditionals."""
        self.full_range()
        x_ctx, theta_ctx, n, dx, dth = self._ar_ctx("ar_marginals", x_ctx, theta_ctx)
        N = int(n_rows)
        x_unique, U = self._ar_unique("ar_marginals", x_unique, N, dx, one_each=True)
        self.check_table(n, dx + dth - 1)
        nb = self.cfg.n_bars
        theta = torch.empty((N, dth), dtype=torch.float32, device=self.device)
        lp = torch.empty(N, dtype=torch.float32, device=self.device) if with_log_prob else None
        probs = torch.empty((U, dth, nb), dtype=torch.float32, device=self.device)
        borders = torch.empty((dth, nb + 1), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_ar_marginals(
            self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_unique), U, N, int(counter), int(row_base),
            _ptr(theta), _ptr(lp), float(eps), _ptr(probs), _ptr(borders), self.stream), "npfn_ar_marginals")
        self.n_features = dx + dth - 1
        return theta, lp, probs, borders

    def ar_pair_marginals(self, x_ctx, theta_ctx, x_unique, n_rows: int, counter: int, edges,
                          with_log_prob: bool = False, eps: float = 1e-15, row_base: int = 0):
        """npfn_ar_pair_marginals: :meth:`ar_sample` over ``x_unique.repeat_interleave(n_rows // U,
        0)`` that also folds every step's row mixtures into 2-D marginals on the cells of ``edges``
        [dim_theta, G + 1] (row k strictly increasing; see :func:`npe_pfn.pair_marginals.grid_edges`).
        Returns ``(theta [n_rows, dim_theta], log_prob [n_rows] or None, pair [U, n_pairs, G, G],
        cell [U, dim_theta, G])`` on the device; ``theta`` and ``log_prob`` are bit for bit those
        of :meth:`ar_sample` with the same counter and row_base.  ``pair[u, k (k - 1) / 2 + j, a,
        c]``, j < k, is the mass of (theta_j in cell a, theta_k in cell c) given ``x_unique[u]``;
        ``cell[u, k, c]`` the mass of theta_k in cell c."""
        self.full_range()
        x_ctx, theta_ctx, n, dx, dth = self._ar_ctx("ar_pair_marginals", x_ctx, theta_ctx)
        N = int(n_rows)
        x_unique, U = self._ar_unique("ar_pair_marginals", x_unique, N, dx, one_each=True)
        edges = _dev_f32(edges, self.device)
        if edges.ndim != 2 or edges.shape[0] != dth or not bool((edges[:, 1:] > edges[:, :-1]).all()):
            raise ValueError(f"ar_pair_marginals: edges {tuple(edges.shape)} must be [{dth}, G + 1] with strictly "
                             "increasing rows")
        G = edges.shape[1] - 1
        self.check_table(n, dx + dth - 1)
        theta = torch.empty((N, dth), dtype=torch.float32, device=self.device)
        lp = torch.empty(N, dtype=torch.float32, device=self.device) if with_log_prob else None
        pair = torch.empty((U, dth * (dth - 1) // 2, G, G), dtype=torch.float32, device=self.device)
        cell = torch.empty((U, dth, G), dtype=torch.float32, device=self.device)
        _check(self.lib, self.lib.npfn_ar_pair_marginals(
            self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_unique), U, N, int(counter), int(row_base),
            _ptr(theta), _ptr(lp), float(eps), _ptr(edges), G, _ptr(pair), _ptr(cell), self.stream),
            "npfn_ar_pair_marginals")
        self.n_features = dx + dth - 1
        return theta, lp, pair, cell

    def ar_log_prob(self, x_ctx, theta_ctx, x_query, theta, eps: float = 1e-15,
                    x_unique: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x_unique``: the distinct rows ``x_query`` repeats (as in :meth:`ar_sample`)."""
        self.full_range()
        x_ctx, theta_ctx, n, dx, dth = self._ar_ctx("ar_log_prob", x_ctx, theta_ctx, matched=False)
        theta = _dev_f32(theta, self.device)
        N = x_query.shape[0]
        if theta.shape != (N, dth):
            raise ValueError("ar_log_prob: theta shape mismatch")
        self.check_table(n, dx + dth - 1)
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        if x_unique is not None:
            x_unique, U = self._ar_unique("ar_log_prob", x_unique, N, dx, of=False)
            _check(self.lib, self.lib.npfn_ar_log_prob_repeated(
                self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_unique), U, _ptr(theta), N, _ptr(out),
                float(eps), self.stream), "npfn_ar_log_prob_repeated")
        else:
            x_query = _dev_f32(x_query, self.device)
            _check(self.lib, self.lib.npfn_ar_log_prob(self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth,
                                                       _ptr(x_query), _ptr(theta), N, _ptr(out), float(eps),
                                                       self.stream),
                   "npfn_ar_log_prob")
        self.n_features = dx + dth - 1
        return out

    def ar_score(self, x_ctx, theta_ctx, x_unique, theta, eps: float = 1e-15, want_logp: bool = True,
                 want_cdf: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """npfn_ar_score: the teacher-forced pass of :meth:`ar_log_prob` with its per-step results
        kept -- ``(logp_steps, cdf_steps)``, each [N, dim_theta] on the device or None when not
        asked for.  Row i of ``theta`` [N, dim_theta] is scored under ``x_unique[i // (N // U)]``
        (U = N: one query row per theta row; U < N: obs-major repeats, step 0 once per distinct
        row).  ``logp_steps`` summed over its columns in order is :meth:`ar_log_prob`, bit for
        bit; ``cdf_steps[:, k]`` is the PIT value F_k(theta_k | x, theta_<k)."""
        if not (want_logp or want_cdf):
            raise ValueError("ar_score: nothing asked for (want_logp and want_cdf are both False)")
        self.full_range()
        x_ctx, theta_ctx, n, dx, dth = self._ar_ctx("ar_score", x_ctx, theta_ctx)
        theta = _dev_f32(theta, self.device)
        if theta.ndim != 2 or theta.shape[1] != dth:
            raise ValueError(f"ar_score: theta {tuple(theta.shape)} is not [N, {dth}]")
        N = theta.shape[0]
        x_unique, U = self._ar_unique("ar_score", x_unique, N, dx)
        self.check_table(n, dx + dth - 1)
        lp = torch.empty((N, dth), dtype=torch.float32, device=self.device) if want_logp else None
        cdf = torch.empty((N, dth), dtype=torch.float32, device=self.device) if want_cdf else None
        _check(self.lib, self.lib.npfn_ar_score(self.h, _ptr(x_ctx), _ptr(theta_ctx), n, dx, dth, _ptr(x_unique), U,
                                                _ptr(theta), N, _ptr(lp), _ptr(cdf), float(eps), self.stream),
               "npfn_ar_score")
        self.n_features = dx + dth - 1
        return lp, cdf

    # ------------------------------------------------------- support kernels
    def box_support(self, theta: torch.Tensor, low: torch.Tensor, high: torch.Tensor) -> torch.Tensor:
        """K9 mask of a box prior; scalar or broadcastable bounds are expanded to theta's
        width first (the kernel reads low[j] / high[j] for every column j)."""
        theta = _dev_f32(theta, self.device)
        if theta.ndim != 2:
            raise ValueError(f"box_support: theta must be [N, dim], got {tuple(theta.shape)}")
        dim = theta.shape[1]
        low = torch.broadcast_to(_dev_f32(low, self.device).reshape(-1), (dim,)).contiguous()
        high = torch.broadcast_to(_dev_f32(high, self.device).reshape(-1), (dim,)).contiguous()
        mask = torch.empty(theta.shape[0], dtype=torch.uint8, device=self.device)
        _check(self.lib, self.lib.npfn_box_support(_ptr(theta), theta.shape[0], theta.shape[1], _ptr(low), _ptr(high),
                                                   _ptr(mask), self.stream), "npfn_box_support")
        return mask.bool()

    def compact_rows(self, src: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        src = _dev_f32(src, self.device)
        m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        dst = torch.empty_like(src)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        _check(self.lib, self.lib.npfn_compact_rows(_ptr(src), _ptr(m), src.shape[0], src.shape[1], _ptr(dst),
                                                    _ptr(cnt), self.stream), "npfn_compact_rows")
        return dst[: int(cnt.item())]

    # ------------------------------------------- restricted prior (npfn_restricted.hip)
    def box_bounds(self, low, high, dim: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Bounds on the device, expanded to ``dim`` as :meth:`box_support` does."""
        low = torch.broadcast_to(_dev_f32(low, self.device).reshape(-1), (dim,)).contiguous()
        high = torch.broadcast_to(_dev_f32(high, self.device).reshape(-1), (dim,)).contiguous()
        return low, high

    def box_propose(self, n_rows: int, dim: int, low, high, counter: int, row_base: int = 0,
                    seed: Optional[int] = None) -> torch.Tensor:
        """[n_rows, dim] points of the box [low, high] at rows ``row_base + i`` of the Philox row
        stream (npfn_box_propose); ``seed`` defaults to the engine's random_state."""
        n_rows, dim = int(n_rows), int(dim)
        if n_rows < 0 or dim < 1:
            raise ValueError(f"box_propose: need n_rows >= 0 and dim >= 1, got {n_rows}, {dim}")
        low, high = self.box_bounds(low, high, dim)
        out = torch.empty((n_rows, dim), dtype=torch.float32, device=self.device)
        seed = self.random_state if seed is None else int(seed)
        _check(self.lib, self.lib.npfn_box_propose(_ptr(low), _ptr(high), dim, n_rows, seed & 0xFFFFFFFFFFFFFFFF,
                                                   int(counter) & 0xFFFFFFFFFFFFFFFF, int(row_base), _ptr(out),
                                                   self.stream), "npfn_box_propose")
        return out

    def predict_accept(self, Xq, threshold: float, return_prob: bool = False):
        """Bool mask ``predict_proba(Xq)[:, -1] > threshold`` on the device (npfn_predict_accept);
        with ``return_prob`` also that last-class probability, bit-equal to predict_proba's."""
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or (self.n_features is not None and Xq.shape[1] != self.n_features):
            raise ValueError(f"predict_accept: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        mask = torch.empty(Xq.shape[0], dtype=torch.uint8, device=self.device)
        prob = torch.empty(Xq.shape[0], dtype=torch.float32, device=self.device) if return_prob else None
        _check(self.lib, self.lib.npfn_predict_accept(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], float(threshold),
                                                      _ptr(mask), _ptr(prob), self.stream), "npfn_predict_accept")
        return (mask.bool(), prob) if return_prob else mask.bool()

    def restricted_box_round(self, low, high, threshold: float, n_rows: int, counter: int, row_base: int,
                             theta_out: torch.Tensor, counts: torch.Tensor, capacity: Optional[int] = None,
                             seed: Optional[int] = None) -> None:
        """One rejection round on the device (npfn_restricted_box_round): ``n_rows`` box proposals at
        Philox rows ``row_base + i``, the classifier's accept decision, and the accepted rows
        appended in order to ``theta_out`` [>= capacity, dim] at ``counts[0]``.  ``counts`` is a
        device int64[2] = (stored, accepted); nothing is read back here."""
        if (theta_out.ndim != 2 or theta_out.dtype != torch.float32 or theta_out.device != self.device
                or not theta_out.is_contiguous()):
            raise ValueError("restricted_box_round: theta_out must be a contiguous float32 [capacity, dim] tensor "
                             "on the engine's device")
        if (counts.dtype != torch.int64 or counts.numel() != 2 or counts.device != self.device
                or not counts.is_contiguous()):
            raise ValueError("restricted_box_round: counts must be a contiguous int64[2] on the engine's device")
        dim = theta_out.shape[1]
        capacity = theta_out.shape[0] if capacity is None else int(capacity)
        if not 0 <= capacity <= theta_out.shape[0]:
            raise ValueError(f"restricted_box_round: capacity {capacity} outside theta_out's {theta_out.shape[0]} rows")
        low, high = self.box_bounds(low, high, dim)
        seed = self.random_state if seed is None else int(seed)
        _check(self.lib, self.lib.npfn_restricted_box_round(
            self.h, _ptr(low), _ptr(high), dim, float(threshold), int(n_rows), seed & 0xFFFFFFFFFFFFFFFF,
            int(counter) & 0xFFFFFFFFFFFFFFFF, int(row_base), _ptr(theta_out), capacity, _ptr(counts), self.stream),
            "npfn_restricted_box_round")

    # ------------------------------------------------- coverage ranks (npfn_ranks.hip)
    def rank_accumulate(self, theta, logp, take, n_obs: int, per: int, theta_true, logp_true, ref, inv_scale,
                        counts: torch.Tensor) -> None:
        """npfn_rank_accumulate: adds the counts of one sampler round to ``counts`` [n_obs, dim + 2,
        2] (int64, on the engine's device, updated in place; zeroed by the caller before the first
        round).  ``theta`` [n_obs * per, dim] obs-major, ``logp`` [n_obs * per], ``take`` [n_obs *
        per] (bool / uint8, None = every row), ``theta_true`` [n_obs, dim], ``logp_true`` [n_obs],
        ``ref`` [n_obs, dim], ``inv_scale`` [dim].  ``logp`` / ``logp_true`` may both be None (the
        HPD column dim is left alone), ``ref`` / ``inv_scale`` too (the TARP column dim + 1).  The
        definition of every count: :func:`npe_pfn.diagnostics.rank_accumulate_host`, which this
        equals exactly.  ValueError for shapes that do not match, before the C call."""
        n_obs, per = int(n_obs), int(per)
        theta = _dev_f32(theta, self.device)
        theta_true = _dev_f32(theta_true, self.device)
        if n_obs < 0 or per < 0 or theta.ndim != 2 or theta.shape[1] < 1 or theta.shape[0] != n_obs * per:
            raise ValueError(f"rank_accumulate: theta {tuple(theta.shape)} is not [{n_obs} * {per}, dim >= 1]")
        dim = theta.shape[1]
        if theta_true.shape != (n_obs, dim):
            raise ValueError(f"rank_accumulate: theta_true {tuple(theta_true.shape)} is not [{n_obs}, {dim}]")
        if (logp is None) != (logp_true is None) or (ref is None) != (inv_scale is None):
            raise ValueError("rank_accumulate: logp / logp_true and ref / inv_scale are given in pairs")
        if logp is not None:
            logp = _dev_f32(logp, self.device).reshape(-1)
            logp_true = _dev_f32(logp_true, self.device).reshape(-1)
            if logp.shape[0] != n_obs * per or logp_true.shape[0] != n_obs:
                raise ValueError(f"rank_accumulate: logp {tuple(logp.shape)} / logp_true {tuple(logp_true.shape)} "
                                 f"do not match {n_obs} observations of {per} rows")
        if ref is not None:
            ref = _dev_f32(ref, self.device)
            inv_scale = _dev_f32(inv_scale, self.device).reshape(-1)
            if ref.shape != (n_obs, dim) or inv_scale.shape[0] != dim:
                raise ValueError(f"rank_accumulate: ref {tuple(ref.shape)} / inv_scale {tuple(inv_scale.shape)} do "
                                 f"not match [{n_obs}, {dim}] / [{dim}]")
        if take is not None:
            take = torch.as_tensor(take).to(device=self.device, dtype=torch.uint8).reshape(-1).contiguous()
            if take.shape[0] != n_obs * per:
                raise ValueError(f"rank_accumulate: take has {take.shape[0]} entries, theta {n_obs * per} rows")
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or counts.device != self.device
                or not counts.is_contiguous() or counts.shape != (n_obs, dim + 2, 2)):
            raise ValueError(f"rank_accumulate: counts must be a contiguous int64 [{n_obs}, {dim + 2}, 2] tensor on "
                             "the engine's device")
        _check(self.lib, self.lib.npfn_rank_accumulate(_ptr(theta), _ptr(logp), _ptr(take), n_obs, per, dim,
                                                       _ptr(theta_true), _ptr(logp_true), _ptr(ref), _ptr(inv_scale),
                                                       _ptr(counts), self.stream), "npfn_rank_accumulate")

    # ------------------------------------------------- pair marginals (npfn_pairs.hip)
    def bar_cell_mass(self, probs, borders, edges) -> torch.Tensor:
        """npfn_bar_cell_mass: the normalised mass of every row of ``probs`` [N, n_bars]
        (unnormalised fp32 bar masses on ``borders`` [n_bars + 1]) in the G cells between
        ``edges`` [G + 1] (strictly increasing): float64 [N, G] on the device; a row without a
        positive finite total is NaN."""
        probs = _dev_f32(probs, self.device)
        borders = _dev_f32(borders, self.device)
        edges = _dev_f32(edges, self.device)
        if probs.ndim != 2 or borders.shape != (probs.shape[1] + 1,) or edges.ndim != 1 or edges.shape[0] < 2:
            raise ValueError(f"bar_cell_mass: probs {tuple(probs.shape)}, borders {tuple(borders.shape)} and edges "
                             f"{tuple(edges.shape)} do not match")
        if not bool((edges[1:] > edges[:-1]).all()):
            raise ValueError("bar_cell_mass: edges must be strictly increasing")
        G = edges.shape[0] - 1
        out = torch.empty((probs.shape[0], G), dtype=torch.float64, device=self.device)
        _check(self.lib, self.lib.npfn_bar_cell_mass(_ptr(probs), _ptr(borders), probs.shape[0], probs.shape[1],
                                                     _ptr(edges), G, _ptr(out), self.stream), "npfn_bar_cell_mass")
        return out

    def pair_accumulate(self, w, theta, edges, r0: int, per: int, pairQ: torch.Tensor, cellQ: torch.Tensor,
                        bad: torch.Tensor) -> None:
        """npfn_pair_accumulate: adds one window of cell masses ``w`` [n, G] (float64) to the integer
        tables ``pairQ`` [U, n_prev, G, G] and ``cellQ`` [U, G] (int64) and raises ``bad`` [U]
        (int32) -- all on the engine's device, updated in place, zeroed by the caller before the
        first window.  Window row r is row ``r0 + r`` of the call and belongs to observation
        ``(r0 + r) // per``; ``theta`` [n, >= n_prev] holds the rows' earlier draws, ``edges``
        [n_prev, G + 1] their cell borders (``theta`` and ``edges`` may be None: n_prev = 0, only
        ``cellQ`` is added to).  The definition of every sum:
        :func:`npe_pfn.pair_marginals.pair_accumulate_host`, which this equals exactly.
        ValueError for shapes that do not match, before the C call."""
        r0, per = int(r0), int(per)
        w = torch.as_tensor(w).to(device=self.device, dtype=torch.float64).contiguous()
        if w.ndim != 2:
            raise ValueError(f"pair_accumulate: w {tuple(w.shape)} is not [n, G]")
        n, G = w.shape
        n_prev, ldt = 0, 0
        if (theta is None) != (edges is None):
            raise ValueError("pair_accumulate: theta and edges are given together")
        if edges is not None:
            edges = _dev_f32(edges, self.device)
            theta = _dev_f32(theta, self.device)
            if edges.ndim != 2 or edges.shape[1] != G + 1 or theta.ndim != 2 or theta.shape[0] != n \
                    or theta.shape[1] < edges.shape[0]:
                raise ValueError(f"pair_accumulate: theta {tuple(theta.shape)} / edges {tuple(edges.shape)} do not "
                                 f"match {n} rows of {G} cells")
            if not bool((edges[:, 1:] > edges[:, :-1]).all()):
                raise ValueError("pair_accumulate: every row of edges must be strictly increasing")
            n_prev, ldt = edges.shape[0], theta.shape[1]
        if per < 1 or r0 < 0:
            raise ValueError(f"pair_accumulate: need per >= 1 and r0 >= 0, got {per} and {r0}")
        U = cellQ.shape[0] if isinstance(cellQ, torch.Tensor) and cellQ.ndim == 2 else -1
        for name, t, shape, dt in (("pairQ", pairQ, (U, n_prev, G, G), torch.int64), ("cellQ", cellQ, (U, G), torch.int64),
                                   ("bad", bad, (U,), torch.int32)):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or not t.is_contiguous()
                    or tuple(t.shape) != shape):
                raise ValueError(f"pair_accumulate: {name} must be a contiguous {dt} {list(shape)} tensor on the "
                                 "engine's device")
        if n and (r0 + n - 1) // per >= U:
            raise ValueError(f"pair_accumulate: rows {r0}..{r0 + n - 1} of {per} per observation exceed {U} observations")
        _check(self.lib, self.lib.npfn_pair_accumulate(
            _ptr(w), _ptr(theta), ldt, n_prev, _ptr(edges), G, r0, n, per, _ptr(pairQ), _ptr(cellQ),
            ctypes.cast(ctypes.c_void_p(bad.data_ptr()), ctypes.POINTER(_i32)), self.stream), "npfn_pair_accumulate")

    # ------------------------------------------------- MMD two-sample sums (npfn_mmd.hip)
    def mmd_sums(self, z, labels, kernel, bandwidths) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """npfn_mmd_sums on the engine's device and stream: :func:`mmd_sums` of this module (the
        entry point needs no engine state; ``z`` and ``labels`` are moved to the engine's device).
        ValueError for arguments that do not fit, before the C call."""
        z = torch.as_tensor(z)
        labels = torch.as_tensor(labels)
        check_mmd_args(z.shape, labels.shape, kernel, bandwidths)
        return mmd_sums(z.to(self.device), labels.to(self.device), kernel, bandwidths, lib=self.lib)

    # ------------------------------------------------- exact W2 assignment (npfn_transport.hip)
    def w2_assign(self, a, b, scale):
        """npfn_w2_assign on the engine's device and stream: :func:`w2_assign` of this module (the
        entry needs no engine; this method moves the arguments to the engine's device)."""
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        check_transport_args(a.shape, b.shape)
        return w2_assign(a.to(self.device), b.to(self.device), torch.as_tensor(scale).to(self.device), lib=self.lib)

    # ------------------------------------------------- classifier two-sample test (npfn_c2st.hip)
    def c2st_fit(self, z, n_first, fold, order, widths, init, epochs, batch_size=128, lr=1e-3, weight_decay=0.0,
                 return_probs=True, return_params=False):
        """npfn_c2st_fit on the engine's device and stream: :func:`c2st_fit` of this module (the
        call needs no engine state; this method only supplies the device and the library)."""
        z = torch.as_tensor(z)
        return c2st_fit(z.to(self.device), n_first, fold, order, widths, init, epochs, batch_size, lr, weight_decay,
                        return_probs, return_params, lib=self.lib)

    def filter_stdeuclid(self, x: torch.Tensor, obs: torch.Tensor, k: int) -> torch.Tensor:
        x = _dev_f32(x, self.device)
        obs = _dev_f32(obs, self.device).reshape(-1)
        idx = torch.empty(int(k), dtype=torch.int64, device=self.device)
        _check(self.lib, self.lib.npfn_filter_stdeuclid(_ptr(x), x.shape[0], x.shape[1], _ptr(obs), int(k), _ptr(idx),
                                                        self.stream), "npfn_filter_stdeuclid")
        return idx

    def kmeans_fit(self, theta: torch.Tensor, k: int, seed: int, max_iter: int = 300,
                   tol: float = 1e-4) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """K13 (npfn_kmeans_fit): seeded k-means of theta [n, dim] -> (centers [k, dim] float32,
        labels [n] int64, counts [k] int64, n_iter [1] int64), all on the device."""
        theta = _dev_f32(theta, self.device)
        if theta.ndim != 2:
            raise ValueError(f"kmeans_fit: theta must be [n, dim], got {tuple(theta.shape)}")
        n, dim = theta.shape
        k = int(k)
        centers = torch.empty((max(k, 0), dim), dtype=torch.float32, device=self.device)
        labels = torch.empty(n, dtype=torch.int64, device=self.device)
        counts = torch.empty(max(k, 0), dtype=torch.int64, device=self.device)
        n_iter = torch.empty(1, dtype=torch.int64, device=self.device)
        _check(self.lib, self.lib.npfn_kmeans_fit(_ptr(theta), n, dim, k, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                  int(max_iter), float(tol), _ptr(centers), _ptr(labels),
                                                  _ptr(counts), _ptr(n_iter), self.stream), "npfn_kmeans_fit")
        return centers, labels, counts, n_iter

    def kmeans_assign(self, theta: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
        """K13 predict (npfn_kmeans_assign): index of the nearest of centers [k, dim] per row of theta."""
        theta = _dev_f32(theta, self.device)
        centers = _dev_f32(centers, self.device)
        if theta.ndim != 2 or centers.ndim != 2 or theta.shape[1] != centers.shape[1]:
            raise ValueError(f"kmeans_assign: theta {tuple(theta.shape)} and centers {tuple(centers.shape)} "
                             "do not match")
        labels = torch.empty(theta.shape[0], dtype=torch.int64, device=self.device)
        _check(self.lib, self.lib.npfn_kmeans_assign(_ptr(theta), theta.shape[0], theta.shape[1], _ptr(centers),
                                                     centers.shape[0], _ptr(labels), self.stream),
               "npfn_kmeans_assign")
        return labels

    # ------------------------------------------------- estimator-parallel split
    def set_estimator_range(self, e0: int, count: int) -> None:
        """Fits / forwards compute estimators [e0, e0 + count) only (npfn_set_estimator_range)."""
        _check(self.lib, self.lib.npfn_set_estimator_range(self.h, int(e0), int(count)), "npfn_set_estimator_range")
        self.e0, self.ne = int(e0), int(count)
        self.n_features = None
        self.ep_set = None  # npe_pfn.distributed's cached strided set is gone

    def set_estimator_set(self, e0: int, count: int, stride: int) -> None:
        """Fits / forwards compute estimators e0 + stride * i, i < count (npfn_set_estimator_set);
        forward_targets returns their tokens in that order."""
        _check(self.lib, self.lib.npfn_set_estimator_set(self.h, int(e0), int(count), int(stride)),
               "npfn_set_estimator_set")
        self.e0, self.ne = int(e0), int(count)
        self.n_features = None
        self.ep_set = None

    def forward_targets(self, Xq) -> torch.Tensor:
        """[count, N, 192] bf16 decoder-input tokens of this engine's estimators (npfn_forward_targets)."""
        if self.n_features is None:
            raise EngineError("forward_targets before fit")
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or Xq.shape[1] != self.n_features:
            raise ValueError(f"forward_targets: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        out = torch.empty((getattr(self, "ne", self.cfg.n_estimators), Xq.shape[0], self.cfg.d_model),
                          dtype=torch.bfloat16, device=self.device)
        _check(self.lib, self.lib.npfn_forward_targets(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], _ptr(out),
                                                       self.stream), "npfn_forward_targets")
        return out

    def forward_logits(self, Xq) -> torch.Tensor:
        """[count, N, n_bars] fp16 decoder logits of this engine's estimators, before the ensemble
        mix (npfn_forward_logits; a partial estimator range is fine)."""
        if self.n_features is None:
            raise EngineError("forward_logits before fit")
        Xq = _dev_f32(Xq, self.device)
        if Xq.ndim != 2 or Xq.shape[1] != self.n_features:
            raise ValueError(f"forward_logits: X has shape {tuple(Xq.shape)}, fit had {self.n_features} features")
        out = torch.empty((self.ne, Xq.shape[0], self.cfg.n_bars), dtype=torch.float16, device=self.device)
        _check(self.lib, self.lib.npfn_forward_logits(self.h, _ptr(Xq), Xq.shape[1], Xq.shape[0], _ptr(out),
                                                      self.stream), "npfn_forward_logits")
        return out

    def head_sample(self, tokens: torch.Tensor, counter: int, row_base: int = 0,
                    log_prob_acc: Optional[torch.Tensor] = None, eps: float = 1e-15) -> torch.Tensor:
        """Decoder + ensemble mix + bar sample of one AR step from [E, N, 192] bf16 tokens of all
        estimators (npfn_head_sample); adds the step's log density into ``log_prob_acc``."""
        if tokens.dtype != torch.bfloat16 or tokens.ndim != 3 or tokens.shape[2] != self.cfg.d_model:
            raise ValueError(f"head_sample: tokens must be bf16 [E, N, {self.cfg.d_model}], got "
                             f"{tokens.dtype} {tuple(tokens.shape)}")
        tokens = tokens.to(self.device).contiguous()
        n = tokens.shape[1]
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        if log_prob_acc is not None and (log_prob_acc.shape != (n,) or log_prob_acc.dtype != torch.float32
                                         or not log_prob_acc.is_contiguous() or log_prob_acc.device != self.device):
            raise ValueError("head_sample: log_prob_acc must be a contiguous float32 [N] tensor on the engine device")
        _check(self.lib, self.lib.npfn_head_sample(self.h, _ptr(tokens), tokens.shape[0], n, int(counter),
                                                   int(row_base), _ptr(out), _ptr(log_prob_acc), float(eps),
                                                   self.stream), "npfn_head_sample")
        return out

    def ar_fit_begin(self, x_ctx, theta_ctx) -> None:
        """npfn_ar_fit_begin: the per-step fits of an AR call on (x_ctx, theta_ctx), driven by
        :meth:`ar_fit_step` (under a fit token every step's preprocessing fit is queued at once)."""
        x_ctx = _dev_f32(x_ctx, self.device).contiguous()
        theta_ctx = _dev_f32(theta_ctx, self.device).contiguous()
        if x_ctx.ndim != 2 or theta_ctx.ndim != 2 or x_ctx.shape[0] != theta_ctx.shape[0]:
            raise ValueError(f"ar_fit_begin: x_ctx {tuple(x_ctx.shape)} and theta_ctx {tuple(theta_ctx.shape)} "
                             "do not match")
        self.check_table(x_ctx.shape[0], x_ctx.shape[1] + theta_ctx.shape[1] - 1)
        _check(self.lib, self.lib.npfn_ar_fit_begin(self.h, _ptr(x_ctx), _ptr(theta_ctx), x_ctx.shape[0],
                                                    x_ctx.shape[1], theta_ctx.shape[1], self.stream),
               "npfn_ar_fit_begin")
        self._ar_dims = (x_ctx.shape[1], theta_ctx.shape[1])
        self._keep = (x_ctx, theta_ctx)

    def ar_fit_step(self, k: int) -> None:
        """npfn_ar_fit_step: step k's fit (on x_ctx | theta_ctx[:, :k] -> theta_ctx[:, k]) becomes
        the current fit of forward_targets / head_sample."""
        _check(self.lib, self.lib.npfn_ar_fit_step(self.h, int(k), self.stream), "npfn_ar_fit_step")
        self.n_features = self._ar_dims[0] + int(k)

    def set_fit_token(self, token: int) -> None:
        """npfn_set_fit_token: ar_sample / ar_log_prob calls under one non-zero token reuse the
        per-step fits of the first (the context must be the same for all of them)."""
        _check(self.lib, self.lib.npfn_set_fit_token(self.h, int(token) & 0xFFFFFFFFFFFFFFFF), "npfn_set_fit_token")

    def set_fit_cache(self, max_sets: int = 1, max_bytes: int = 0) -> None:
        """npfn_set_fit_cache: how many sets of per-step fits the engine keeps across fit tokens
        (a call under a new token whose context table equals a cached set's, bit for bit, refits
        nothing; 0 = no reuse across tokens) and the device memory they may hold (0 = no limit)."""
        _check(self.lib, self.lib.npfn_set_fit_cache(self.h, int(max_sets), int(max_bytes)), "npfn_set_fit_cache")

    def fit_cache_stats(self) -> dict:
        """npfn_fit_cache_stats: {hits, misses, sets, bytes} of the fit cache."""
        hits, misses, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        sets = ctypes.c_int32(0)
        _check(self.lib, self.lib.npfn_fit_cache_stats(self.h, ctypes.byref(hits), ctypes.byref(misses),
                                                       ctypes.byref(sets), ctypes.byref(nbytes)),
               "npfn_fit_cache_stats")
        return {"hits": int(hits.value), "misses": int(misses.value), "sets": int(sets.value),
                "bytes": int(nbytes.value)}

    def fit_cache_clear(self) -> None:
        """npfn_fit_cache_clear: free every cached set of fits."""
        _check(self.lib, self.lib.npfn_fit_cache_clear(self.h), "npfn_fit_cache_clear")

    def set_chunk_rows(self, rows: int) -> None:
        """Query rows per forward chunk (npfn_set_chunk_rows; default 16384)."""
        _check(self.lib, self.lib.npfn_set_chunk_rows(self.h, int(rows)), "npfn_set_chunk_rows")

    # -------------------------------------------------------------- profiling
    def prof_enable(self, on: bool = True) -> None:
        _check(self.lib, self.lib.npfn_prof_enable(self.h, 1 if on else 0), "npfn_prof_enable")

    def prof_read(self) -> list:
        """Per-kernel totals since the last read: [{name, launches, ms, flops, bytes}] (synchronizes)."""
        buf = (NpfnProfEntry * 32)()
        n = ctypes.c_int32(0)
        _check(self.lib, self.lib.npfn_prof_read(self.h, buf, 32, ctypes.byref(n)), "npfn_prof_read")
        return [dict(name=buf[i].name.decode(), launches=int(buf[i].launches), ms=float(buf[i].ms),
                     flops=float(buf[i].flops), bytes=float(buf[i].bytes)) for i in range(n.value)]

    def debug_views(self, rows: int, max_cols: int = 1024) -> np.ndarray:
        """[rows, Vw] preprocessed table of the last fit / forward (npfn_debug_views; synchronous)."""
        buf = np.empty((int(rows), int(max_cols)), dtype=np.float32)
        vw = ctypes.c_int32(0)
        _check(self.lib, self.lib.npfn_debug_views(self.h, buf.ctypes.data_as(ctypes.c_void_p), int(rows),
                                                   int(max_cols), ctypes.byref(vw)), "npfn_debug_views")
        return buf.reshape(-1)[: int(rows) * vw.value].reshape(int(rows), vw.value).copy()

    def debug_target_translation(self) -> dict:
        """The last regressor fit's target-border translation on the host
        (npfn_debug_target_translation; synchronous): ``ylam``, ``ystats`` [6], ``idx`` / ``share``
        [n_bars + 1], ``tcancel`` [n_bars], ``ett`` [n_estimators] and ``translated``; without a
        target-transforming estimator ``translated`` is False and the tables are None."""
        nb, E = self.cfg.n_bars, self.cfg.n_estimators
        ylam = ctypes.c_double()
        ystats = np.zeros(6, np.float32)
        idx, share = np.zeros(nb + 1, np.int32), np.zeros(nb + 1, np.float32)
        tc, ett = np.zeros(nb, np.uint8), np.zeros(E, np.int32)
        tr = _i32(0)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(_i32))  # noqa: E731
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.npfn_debug_target_translation(
                self.h, nb, E, ctypes.cast(ctypes.byref(ylam), ctypes.c_void_p), vp(ystats), ip(idx), vp(share),
                vp(tc), ip(ett), ctypes.byref(tr)), "npfn_debug_target_translation")
        on = bool(tr.value)
        return {"translated": on, "ylam": ylam.value, "ystats": ystats, "ett": ett, "idx": idx if on else None,
                "share": share if on else None, "tcancel": tc if on else None}

    def mix_translation(self):
        """``(ett, tab, tcancel)`` device buffers of the last fit for :func:`mix_rows`, or three
        None when nothing is translated."""
        t = self.debug_target_translation()
        if not t["translated"]:
            return None, None, None
        tab, tc = pack_translation(t["idx"], t["share"], t["tcancel"], self.device)
        return torch.from_numpy(t["ett"]).to(self.device), tab, tc

    def debug_item_attn_online(self, on: bool = True) -> None:
        """Process-wide: every item-attention block also runs its online-softmax fallback pass
        (npfn_debug_item_attn_online) -- lets the tests pin both passes against the oracle."""
        _check(self.lib, self.lib.npfn_debug_item_attn_online(1 if on else 0), "npfn_debug_item_attn_online")

    def debug_item_attn_scale(self, scale: float = 1.0) -> None:
        """Process-wide: multiply every item-attention score by ``scale`` (stress runs of the
        first pass's fallback; npfn_debug_item_attn_scale).  1.0 restores the model."""
        _check(self.lib, self.lib.npfn_debug_item_attn_scale(float(scale)), "npfn_debug_item_attn_scale")

    def debug_fail_row_launch(self, n: int = 1) -> None:
        """The ``n``-th next row-kernel launch is refused by the runtime (0 = off;
        npfn_debug_fail_row_launch): the error path's test."""
        _check(self.lib, self.lib.npfn_debug_fail_row_launch(self.h, int(n)), "npfn_debug_fail_row_launch")

    def item_attn_fallback(self, reset: bool = True) -> dict:
        """Item-attention launches since the last reset: blocks / query rows that ran or took the
        online-softmax fallback pass, and their totals (npfn_item_attn_fallback; synchronizes); the
        fallback rows split by cause -- sum overflow, underflow, padding-dominated / forced
        (npfn_item_attn_fallback_causes)."""
        cause = (ctypes.c_uint64 * 2)()
        if hasattr(self.lib, "npfn_item_attn_fallback_causes"):  # an older library in an A/B run has none
            _check(self.lib, self.lib.npfn_item_attn_fallback_causes(self.h, cause), "npfn_item_attn_fallback_causes")
        buf = (ctypes.c_uint64 * 4)()
        _check(self.lib, self.lib.npfn_item_attn_fallback(self.h, buf, 1 if reset else 0), "npfn_item_attn_fallback")
        b_fb, b_all, r_fb, r_all = (int(v) for v in buf)
        r_over, r_under = int(cause[0]), int(cause[1])
        return {"blocks_fallback": b_fb, "blocks": b_all, "rows_fallback": r_fb, "rows": r_all,
                "rows_overflow": r_over, "rows_underflow": r_under,
                "rows_padding": max(r_fb - r_over - r_under, 0),
                "fallback_frac": (r_fb / r_all) if r_all else 0.0,
                "block_fallback_frac": (b_fb / b_all) if b_all else 0.0}
