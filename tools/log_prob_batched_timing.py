"""Scoring M true (theta, x) pairs two ways at Gaussian-linear 10-D, 1000 simulations, one GPU,
one process, TabPFN_Based_NPE_PFN with its defaults (ensemble preprocessing):

  (a) one log_prob_batched(theta[M, D], x[M, D]) call -- one teacher-forced pass, D fits
  (b) a loop of M log_prob(theta[m:m+1], x[m]) calls   -- M * D fits (the only route before
      log_prob_batched existed; log_prob itself is unchanged by it)

After a warm-up of each, the two alternate; every timed run ends in a device synchronise.  Prints
the median, min and max of the runs and the ratio of the medians; writes the same as JSON when
--out is given.  It records what the calls cost and asserts nothing.

    python tools/log_prob_batched_timing.py [--pairs 64] [--runs 5] [--warmup 1] [--out FILE.json]
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

from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN  # noqa: E402
from npe_pfn.tasks import gaussian_linear, gaussian_linear_task  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=64, help="M, the number of (theta, x) pairs")
    ap.add_argument("--sims", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("log_prob_batched_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    theta, x, _ = gaussian_linear_task(args.dim, args.sims, seed=0)
    g = torch.Generator().manual_seed(7)
    theta_o = torch.randn(args.pairs, args.dim, generator=g) * (0.1 ** 0.5)
    x_o = gaussian_linear(theta_o, generator=g)
    theta, x, theta_o, x_o = (t.to(dev) for t in (theta, x, theta_o, x_o))
    post = TabPFN_Based_NPE_PFN(regressor_init_kwargs={"random_state": 0, "device": "cuda:0"})
    post.append_simulations(theta, x)

    def batched():
        return post.log_prob_batched(theta_o, x_o)

    def looped():
        return torch.stack([post.log_prob(theta_o[m: m + 1], x_o[m])[0] for m in range(args.pairs)])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for _ in range(args.warmup):
        batched(), looped()
    names = ("log_prob_batched", "looped_log_prob")
    t = {k: [] for k in names}
    for _ in range(args.runs):
        ms, lp_b = timed(batched)
        t[names[0]].append(ms)
        ms, lp_l = timed(looped)
        t[names[1]].append(ms)
    d = (lp_b.cpu() - lp_l.cpu()).abs()

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    res = {"device": torch.cuda.get_device_name(0),
           "task": {"name": "gaussian_linear", "dim": args.dim, "simulations": args.sims, "pairs": args.pairs,
                    "preprocessing": "ensemble"},
           "runs": args.runs, "warmup": args.warmup,
           "ms": {k: summary(v) for k, v in t.items()},
           "looped_over_batched": statistics.median(t[names[1]]) / statistics.median(t[names[0]]),
           "abs_diff_of_the_two_results": {"median": float(d.median()), "max": float(d.max())}}
    for k, v in res["ms"].items():
        print(f"{k:18s} median {v['median']:.2f} ms  (min {v['min']:.2f}, max {v['max']:.2f}) over {args.runs} runs")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
