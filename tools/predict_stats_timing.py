"""Two ways to the summaries of a regressor predict on the c2 table (1000 context rows, 10
features, 10 000 query rows, default ensemble preprocessing), one GPU, one process:

  (a) Engine.predict_logits + Engine.bar_stats   -- [N, 5000] fp32 logits written and read again
  (b) Engine.predict_stats                       -- the summaries inside the engine, no [N, 5000] buffer

with tabpfn's nine default quantiles plus the median.  After a warm-up the two alternate; each
timed call ends in a device synchronise.  Prints the median, min and max of the calls and, from
the engine's profiler in a separate pair of calls, the per-launch times of the mix / summary
kernels (k_mix_log, k_bar_stats); writes the same as JSON when --out is given.

    python tools/predict_stats_timing.py [--calls 12] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "npe-pfn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from npe_pfn.engine import Engine  # noqa: E402
from npe_pfn.weights import ModelConfig, synthetic_weights  # noqa: E402

QS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.5)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=12, help="timed calls of each variant (at least 10)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("predict_stats_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    cfg = ModelConfig()
    eng = Engine(cfg, synthetic_weights(cfg, 0), device=torch.device("cuda", 0), random_state=0)
    rng = np.random.default_rng(0)
    n, F, N = 1000, 10, args.rows
    X = torch.from_numpy(rng.normal(size=(n, F)).astype(np.float32)).cuda()
    y = torch.from_numpy((rng.normal(size=n)).astype(np.float32)).cuda()
    Xq = torch.from_numpy(rng.normal(size=(N, F)).astype(np.float32)).cuda()
    eng.fit(X, y)
    borders = eng.borders()

    def via_logits():
        return eng.bar_stats(eng.predict_logits(Xq), borders, QS)

    def in_engine():
        return eng.predict_stats(Xq, QS)

    def timed(fn) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        a, b = via_logits(), in_engine()
    torch.cuda.synchronize()
    span = float(borders[-1] - borders[0])
    diff = {k: float((a[k] - b[k]).abs().max()) / span for k in ("mean", "quantiles")}
    t = {"predict_logits+bar_stats": [], "predict_stats": []}
    for _ in range(args.calls):
        t["predict_logits+bar_stats"].append(timed(via_logits))
        t["predict_stats"].append(timed(in_engine))

    eng.prof_enable(True)   # per-kernel times: a pair of calls of their own
    eng.prof_read()
    via_logits()
    in_engine()
    prof = {e["name"]: e for e in eng.prof_read()}
    eng.prof_enable(False)

    def per_launch(name):
        e = prof.get(name)
        return None if not e or not e["launches"] else {"launches": e["launches"], "ms_per_launch": e["ms"] / e["launches"],
                                                        "GB_per_s": e["bytes"] / e["ms"] / 1e6 if e["ms"] else None}

    res = {"device": torch.cuda.get_device_name(0), "table": {"n_ctx": n, "features": F, "query_rows": N},
           "quantiles": list(QS), "calls": args.calls, "warmup": args.warmup,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()},
           "predict_stats_minus_via_logits_ms": statistics.median(t["predict_stats"])
           - statistics.median(t["predict_logits+bar_stats"]),
           "max_abs_diff_over_span": diff,
           "profiler": {k: per_launch(k) for k in ("k_mix_log", "k_bar_stats")},
           "profiler_all_ms": {k: v["ms"] for k, v in prof.items()}}
    for k, v in res["ms"].items():
        print(f"{k:26s} median {v['median']:.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}) over {args.calls} calls")
    print("profiler per launch:", json.dumps(res["profiler"]))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
