"""What the pair marginals cost beside the averaged marginals and plain sampling, at the benchmark
configuration c2 (Gaussian-linear 10-D, 1000 simulations, 10 000 draws of one observation, one
GPU, one process, TabPFN_Based_NPE_PFN with its defaults):

  (a) pair_marginals(x_o, num_draws=10_000, bins=64) -- npfn_ar_pair_marginals: the sampler's call
      plus, per step, the row mixtures through a window (k_mix_prob + k_group_sample instead of the
      fused k_mix_sample), their re-binning onto 64 cells and the integer fold of the 45 pair tables
  (b) marginals(x_o, num_draws=10_000)  -- npfn_ar_marginals: the same window, a column reduction
  (c) sample((10_000,), x=x_o)          -- npfn_ar_sample_repeated and the accept/reject step

After a warm-up of each, the three alternate; every timed call ends in a device synchronise.
Prints the median, min and max of the runs and the differences of the medians; writes the same as
JSON when --out is given.  It records what the calls cost and asserts nothing.

    python tools/pair_marginals_timing.py [--draws 10000] [--bins 64] [--runs 5] [--warmup 1] [--out FILE.json]
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
from npe_pfn.tasks import gaussian_linear_prior, gaussian_linear_task  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=10_000)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--sims", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pair_marginals_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    theta, x, x_o = (t.to(dev) for t in gaussian_linear_task(args.dim, args.sims, seed=0))
    post = TabPFN_Based_NPE_PFN(prior=gaussian_linear_prior(args.dim, device=dev),
                                regressor_init_kwargs={"random_state": 0, "device": "cuda:0"})
    post.append_simulations(theta, x)

    calls = {
        "pair_marginals": lambda: post.pair_marginals(x_o, num_draws=args.draws, bins=args.bins,
                                                      max_sampling_batch_size=args.draws),
        "marginals": lambda: post.marginals(x_o, num_draws=args.draws, max_sampling_batch_size=args.draws),
        "sample": lambda: post.sample((args.draws,), x=x_o, max_sampling_batch_size=args.draws),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    last = {}
    for _ in range(args.runs):
        for k, fn in calls.items():
            ms, last[k] = timed(fn)
            t[k].append(ms)

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    med = {k: statistics.median(v) for k, v in t.items()}
    pm = last["pair_marginals"]
    inside = torch.stack([pm.mass_inside(j, k) for k in range(args.dim) for j in range(k)])
    res = {"device": torch.cuda.get_device_name(0),
           "task": {"name": "gaussian_linear", "dim": args.dim, "simulations": args.sims, "draws": args.draws,
                    "bins": args.bins, "pairs": args.dim * (args.dim - 1) // 2, "preprocessing": "ensemble"},
           "runs": args.runs, "warmup": args.warmup,
           "ms": {k: summary(v) for k, v in t.items()},
           "pair_marginals_minus_marginals_ms": med["pair_marginals"] - med["marginals"],
           "pair_marginals_minus_sample_ms": med["pair_marginals"] - med["sample"],
           "pair_marginals_over_marginals": med["pair_marginals"] / med["marginals"],
           "min_mass_inside": float(inside.min()), "max_mass_inside": float(inside.max())}
    for k, v in res["ms"].items():
        print(f"{k:15s} median {v['median']:.2f} ms  (min {v['min']:.2f}, max {v['max']:.2f}) over {args.runs} runs")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
