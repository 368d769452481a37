"""The parity cases of npfn_c2st_fit (tests/test_gpu_c2st.py) and their host side, shared with
tests/test_c2st_host.py, which confirms on the CPU that the float64 definition alone leaves at most
one held-out point per (observation, fold) too close to 0.5 to pin its prediction.

The kernel works on tiles of ROW_TILE = 16 batch rows (npfn_c2st.hip kRows) and on 4 x 4 tiles of
every layer's [W | b]; the shapes below are the smallest that reach each of its edges."""
import functools

import torch

from npe_pfn.diagnostics import c2st_fit_host, c2st_folds, c2st_init, c2st_order, c2st_widths

ROW_TILE = 16
LR = 1e-3               # c2st_batched's default; at 1e-2 the float32 host itself drifts 1e-4 from float64 at d = 11
N_OBS = 2
MARGIN = 16.0           # x max(|host float32 - host float64|, 2^-24): the device's distance from float64
FLOOR = 2.0 ** -24      # one fp32 ulp of a loss in [0.5, 1)

# name: (d, n, m, model, n_folds, epochs, batch_size, weight_decay, init kind, data seed)
CASES = {
    # widths 1, 4, 8, 8, 4, 2: narrower than any tile; n = 23, m = 17: unequal fold and class sizes
    "d1_unequal_sets": (1, 23, 17, "mlp", 5, 3, 16, 0.0, "default", 0),
    "d3": (3, 50, 45, "mlp", 5, 3, 32, 0.0, "default", 0),            # 12, 24: no multiples of 16
    "d10": (10, 40, 40, "mlp", 5, 3, 32, 0.0, "default", 0),
    "d11_parameter_cap": (11, 40, 40, "mlp", 5, 3, 32, 0.0, "default", 0),
    "batch_tile_less_one": (3, 30, 30, "mlp", 5, 2, ROW_TILE - 1, 0.0, "default", 0),
    "batch_tile": (3, 30, 30, "mlp", 5, 2, ROW_TILE, 0.0, "default", 0),
    "batch_tile_plus_one": (3, 30, 30, "mlp", 5, 2, ROW_TILE + 1, 0.0, "default", 0),
    "batch_two_tiles": (3, 30, 30, "mlp", 5, 2, 2 * ROW_TILE, 0.0, "default", 0),
    # N = 41 in 5 folds: n_train is 32 (one fold) or 33 (four)
    "n_train_at_and_above_batch": (3, 21, 20, "mlp", 5, 3, 32, 0.0, "default", 0),
    "n_train_below_and_at_batch": (3, 21, 20, "mlp", 5, 3, 33, 0.0, "default", 0),
    "batch_above_n_train": (3, 23, 17, "mlp", 5, 4, 64, 0.0, "default", 0),
    "unequal_sets": (2, 23, 17, "mlp", 5, 3, 16, 0.0, "default", 0),
    "two_folds": (3, 20, 21, "mlp", 2, 3, 16, 0.0, "default", 0),
    "one_epoch": (3, 30, 30, "mlp", 5, 1, 16, 0.0, "default", 0),
    "mlp_small": (5, 30, 30, "mlp_small", 5, 3, 16, 0.0, "default", 0),
    "linear": (7, 30, 30, "linear", 5, 4, 16, 0.0, "default", 0),
    "weight_decay": (3, 30, 30, "mlp", 5, 3, 16, 0.01, "default", 0),
    "dead_layer": (3, 30, 30, "mlp", 5, 3, 16, 0.0, "dead", 0),
}
DEAD_LAYER = 1   # of the "dead" init: zero weights and bias -1, so none of its ReLUs ever fires


def layer_slices(widths):
    out, off = [], 0
    for i, o in zip(widths[:-1], widths[1:]):
        out.append((slice(off, off + o * i), slice(off + o * i, off + o * i + o)))
        off += o * i + o
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(z [N_OBS, n + m, d] float32, n, fold, order, widths, init, epochs, batch, lr, weight_decay)."""
    d, n, m, model, n_folds, epochs, batch, wd, kind, seed = CASES[name]
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.randn((N_OBS, n + m, d), generator=g)
    z[:, n:] += 0.7
    widths = c2st_widths(model, d)
    init = c2st_init(widths, seed=1)
    if kind == "dead":
        w, b = layer_slices(widths)[DEAD_LAYER]
        init[w], init[b] = 0.0, -1.0
    return z, n, c2st_folds(n, m, n_folds, seed=1), c2st_order(n + m, epochs, seed=1), widths, init, epochs, batch, LR, wd


@functools.lru_cache(maxsize=None)
def host(name):
    """{"f64": c2st_fit_host at float64, "f32": at float32, "bound": {"loss", "prob"}}: the bound of a
    quantity is MARGIN * max(max |f32 - f64|, FLOOR).  Computed once per case and left unchanged."""
    args = inputs(name)
    f64 = c2st_fit_host(*args, dtype=torch.float64)
    f32 = c2st_fit_host(*args, dtype=torch.float32)
    y = {"loss": float((f32[1].double() - f64[1]).abs().max()), "prob": float((f32[2].double() - f64[2]).abs().max())}
    return {"f64": f64, "f32": f32, "y": y, "bound": {k: MARGIN * max(v, FLOOR) for k, v in y.items()}}


def undecided(name):
    """bool [N_OBS, N]: the held-out points whose float64 probability is within the case's prob
    bound of 0.5; their prediction is not pinned."""
    h = host(name)
    return (h["f64"][2] - 0.5).abs() <= h["bound"]["prob"]
