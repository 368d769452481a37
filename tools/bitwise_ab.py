"""Bitwise comparison of two engine builds on the c2 shape (ensemble: two estimator groups) and on a
small ragged shape that walks every AR entry point.

usage: NPFN_LIB=<lib> python tools/bitwise_ab.py OUT.npz     (once per build)
       NPFN_LIB=<lib> python tools/bitwise_ab.py --prof OUT.json   (once per build, a run of its own)
       python tools/bitwise_ab.py --compare A.npz B.npz      (or A.json B.json)
c2: draws of npfn_ar_sample (10 AR dims, 2000 queries or NPFN_BW_ROWS), the teacher-forced log-probs and
one predict's logits.  Small shape (150 context rows, 3 + 3 dims, 4 observations x 50 rows in chunks of
64: windows of 64, 64, 64 and 8 rows that cross the observations), once each with preprocessing "none",
"ensemble" and a 250-bar model (not a multiple of 4: the generic NV = 0 mix kernels): every ar_* call
plain and with repeated rows, and bar_nll / bar_cdf with targets at a border and far in both tails.
--prof: the small shape's AR calls under the live profiler, each call's (name, launches, flops, bytes)
rows -- the launch sequence.  A refactoring that keeps the per-tile arithmetic and the launches must
match bit for bit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "npe-pfn_amd"))

if sys.argv[1] == "--compare":
    ok = True
    if sys.argv[2].endswith(".json"):
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        for k in a:
            same = a[k] == b.get(k)
            ok &= same
            print(f"{k}: {len(a[k])} profiler rows {'equal' if same else 'DIFFER: %r vs %r' % (a[k], b.get(k))}")
        sys.exit(0 if ok and set(a) == set(b) else 1)
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    for k in a.files:
        same = a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape
        ok &= same
        print(f"{k}: {'bitwise equal' if same else 'DIFFER, max |d| = %g' % np.abs(a[k] - b[k]).max()}")
    sys.exit(0 if ok and set(a.files) == set(b.files) else 1)

import torch

from npe_pfn.engine import Engine
from npe_pfn.pair_marginals import grid_edges
from npe_pfn.tasks import gaussian_linear_task
from npe_pfn.weights import ModelConfig, synthetic_weights

dev = torch.device("cuda", 0)


def small_calls(cfg, mode):
    """[(name, thunk -> tuple of tensors / None)] of the small shape; the thunks share one engine."""
    eng = Engine(cfg, synthetic_weights(cfg, seed=0), device=dev, random_state=0)
    eng.set_preprocessing(mode)
    eng.set_chunk_rows(64)
    theta, x, x_o = gaussian_linear_task(3, 150, seed=0)
    g = torch.Generator().manual_seed(2)
    xu = x_o + 0.05 * torch.randn(4, 3, generator=g)
    xq = xu.repeat_interleave(50, 0)
    th = theta[:1] + 0.3 * torch.randn(200, 3, generator=g)
    edges = grid_edges([[-1.5, 1.5]] * 3, 8)
    calls = [
        ("ar_sample", lambda: eng.ar_sample(x, theta, xq, counter=3, with_log_prob=True)),
        ("ar_sample_rep", lambda: eng.ar_sample(x, theta, xq, counter=3, with_log_prob=True, x_unique=xu)),
        ("ar_marginals", lambda: eng.ar_marginals(x, theta, xu, 200, counter=3, with_log_prob=True)),
        ("ar_pair_marginals", lambda: eng.ar_pair_marginals(x, theta, xu, 200, 3, edges, with_log_prob=True)),
        ("ar_log_prob", lambda: (eng.ar_log_prob(x, theta, xq, th),)),
        ("ar_log_prob_rep", lambda: (eng.ar_log_prob(x, theta, xq, th, x_unique=xu),)),
        ("ar_score", lambda: eng.ar_score(x, theta, xq, th)),
        ("ar_score_rep", lambda: eng.ar_score(x, theta, xu, th)),
    ]

    def bars():
        eng.fit(torch.cat([x, theta[:, :1]], 1), theta[:, 1])
        logits = eng.predict_logits(torch.cat([xq, th[:, :1]], 1)[:64])
        b = eng.borders()
        y = th[:64, 1].to(dev).clone()
        y[0], y[1], y[2], y[3], y[4] = b[0], b[cfg.n_bars // 2], b[-1], -1e6, 1e6
        return eng.bar_nll(logits, b, y), eng.bar_cdf(logits, b, y)
    return eng, calls, bars


SMALL = [("none", ModelConfig(), "none"), ("ens", ModelConfig(), "ensemble"),
         ("nb250", ModelConfig(n_layers=2, n_bars=250, max_groups=16), "ensemble")]

if sys.argv[1] == "--prof":
    rows = {}
    for tag, cfg, mode in SMALL:
        eng, calls, _ = small_calls(cfg, mode)
        eng.prof_enable(True)
        for name, run in calls:
            eng.prof_read()
            run()
            rows[f"{tag}.{name}"] = [[r["name"], r["launches"], r["flops"], r["bytes"]] for r in eng.prof_read()]
        eng.prof_enable(False)
    json.dump(rows, open(sys.argv[2], "w"), indent=0)
    print("saved", sys.argv[2])
    sys.exit(0)

out = {}
for tag, cfg, mode in SMALL:
    eng, calls, bars = small_calls(cfg, mode)
    for name, run in calls + [("bar_nll_cdf", bars)]:
        for i, t in enumerate(run()):
            out[f"{tag}.{name}.{i}"] = t.cpu().numpy()
    del eng

cfg = ModelConfig()
w = synthetic_weights(cfg, seed=0)
theta, x, x_o = gaussian_linear_task(10, 1000, seed=0)
g = torch.Generator().manual_seed(1)
NQ = int(os.environ.get("NPFN_BW_ROWS", "2000"))  # query rows (>= 4096: the engine's two AR lanes)
xq = x_o.repeat(NQ, 1) + 0.05 * torch.randn(NQ, 10, generator=g)
eng = Engine(cfg, w, device=dev, random_state=0)
eng.set_preprocessing("ensemble")
if os.environ.get("NPFN_BW_TOKEN") == "1":  # per-step fit slots, as sample() runs (the two AR lanes need them)
    eng.set_fit_token(12345)
th, lp = eng.ar_sample(x, theta, xq, counter=0, with_log_prob=True)
lp2 = eng.ar_log_prob(x, theta, xq, th)
eng.fit(torch.cat([x, theta[:, :3]], 1), theta[:, 3])
logits = eng.predict_logits(torch.cat([xq, th[:, :3].cpu()], 1)[:500])
np.savez(sys.argv[1], theta=th.cpu().numpy(), lp=lp.cpu().numpy(), lp2=lp2.cpu().numpy(),
         logits=logits.cpu().numpy(), **out)
print("saved", sys.argv[1])
