"""What the exact W2 assignment costs, on one GPU in one process: one npfn_w2_assign call
(npe_pfn.engine.w2_assign) on device tensors, against what a user does without it: the integer cost
matrix of every observation on the host and scipy.optimize.linear_sum_assignment looped over the
observations, on this machine's CPU (the solver alone is timed; forming and copying the costs is
not counted against it).  Cases: M = 1 and M = 64 observations of n = 1000 draws in d = 10, and M =
64 of n = 2048 in d = 8.

Each device window is one call ending in a device synchronise.  After --warmup device windows, the
median / min / max of --runs windows per side.  The two sides' cost sums are compared (they are equal
integers) before anything is timed.  Records the solver's steps per observation and the
microseconds per step they imply for one workgroup (the call's time over the largest step count of
a wave of observations: with M <= the number of CUs every observation has a CU of its own).
Records what the calls cost; asserts nothing else.  Writes the same as JSON when --out is given.

    python tools/transport_timing.py [--runs 5] [--warmup 1] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "npe-pfn_amd"))
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

from npe_pfn.diagnostics import transport_costs_host, transport_scale  # noqa: E402
from npe_pfn.engine import w2_assign  # noqa: E402

CASES = ((1, 1000, 10), (64, 1000, 10), (64, 2048, 8))


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("transport_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "host_threads": torch.get_num_threads(), "runs": args.runs, "warmup": args.warmup, "cases": {}}
    for M, n, d in CASES:
        gen = torch.Generator(device=dev).manual_seed(1)
        a = torch.randn(M, n, d, device=dev, generator=gen)
        b = torch.randn(M, n, d, device=dev, generator=gen) + 0.25
        scale, _ = transport_scale(a, b)

        def ours():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = w2_assign(a, b, scale)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        cq = transport_costs_host(a, b)[0].cpu().numpy()

        def theirs():
            t0 = time.perf_counter()
            total = [int(c[linear_sum_assignment(c)].sum()) for c in cq]
            return (time.perf_counter() - t0) * 1e3, total

        _, (_, _, cost_sum, steps, bad) = ours()
        _, ref = theirs()
        if cost_sum.tolist() != ref or int(bad.sum()) != 0:
            sys.exit(f"transport_timing: M={M} n={n} d={d}: the device's cost sums differ from scipy's")
        for _ in range(args.warmup):   # scipy's side is warm from the comparison above
            ours()
        t = {"w2_assign": [ours()[0] for _ in range(args.runs)], "scipy_loop": [theirs()[0] for _ in range(args.runs)]}
        med = {k: statistics.median(v) for k, v in t.items()}
        st = steps.tolist()
        res["cases"][f"M={M},n={n},d={d}"] = {
            "observations": M, "n": n, "dim": d, "ms_per_call": {k: summary(v) for k, v in t.items()},
            "scipy_loop_over_w2_assign": med["scipy_loop"] / med["w2_assign"],
            "steps_per_observation": {"mean": sum(st) / M, "min": min(st), "max": max(st), "bound": n * (n + 1) // 2},
            "us_per_step_of_one_workgroup": med["w2_assign"] * 1e3 / max(st)}
        for k, v in res["cases"][f"M={M},n={n},d={d}"]["ms_per_call"].items():
            print(f"M={M:3d} n={n} d={d} {k:10s} median {v['median']:.2f} ms (min {v['min']:.2f}, max {v['max']:.2f})")
        print(f"    steps per observation: mean {sum(st) / M:.0f}, max {max(st)}; "
              f"{med['w2_assign'] * 1e3 / max(st):.3f} us per step; scipy / device = {med['scipy_loop'] / med['w2_assign']:.2f}")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
