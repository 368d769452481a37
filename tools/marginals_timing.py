"""What the averaged marginals cost beside plain sampling, at the benchmark configuration c2
(Gaussian-linear 10-D, 1000 simulations, 10 000 draws of one observation, one GPU, one process,
TabPFN_Based_NPE_PFN with its defaults):

  (a) marginals(x_o, num_draws=10_000)  -- npfn_ar_marginals: the sampler's call plus, per step,
      the row mixtures through a window (k_mix_prob + k_group_sample instead of the fused
      k_mix_sample) and the column reduction
  (b) sample((10_000,), x=x_o)          -- npfn_ar_sample_repeated and the accept/reject step

After a warm-up of each, the two alternate; every timed call ends in a device synchronise.  Prints
the median, min and max of the runs and the ratio of the medians; writes the same as JSON when
--out is given.  It records what the calls cost and asserts nothing.

    python tools/marginals_timing.py [--draws 10000] [--runs 5] [--warmup 1] [--out FILE.json]
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
    ap.add_argument("--sims", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("marginals_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    theta, x, x_o = (t.to(dev) for t in gaussian_linear_task(args.dim, args.sims, seed=0))
    post = TabPFN_Based_NPE_PFN(prior=gaussian_linear_prior(args.dim, device=dev),
                                regressor_init_kwargs={"random_state": 0, "device": "cuda:0"})
    post.append_simulations(theta, x)

    def marginals():
        return post.marginals(x_o, num_draws=args.draws, max_sampling_batch_size=args.draws)

    def sample():
        return post.sample((args.draws,), x=x_o, max_sampling_batch_size=args.draws)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for _ in range(args.warmup):
        marginals(), sample()
    names = ("marginals", "sample")
    t = {k: [] for k in names}
    for _ in range(args.runs):
        ms, pm = timed(marginals)
        t[names[0]].append(ms)
        ms, _ = timed(sample)
        t[names[1]].append(ms)

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"device": torch.cuda.get_device_name(0),
           "task": {"name": "gaussian_linear", "dim": args.dim, "simulations": args.sims, "draws": args.draws,
                    "preprocessing": "ensemble"},
           "runs": args.runs, "warmup": args.warmup,
           "ms": {k: summary(v) for k, v in t.items()},
           "marginals_over_sample": med["marginals"] / med["sample"],
           "marginals_minus_sample_ms": med["marginals"] - med["sample"],
           "support_fraction": float(pm.support_fraction[0]),
           "max_abs_row_sum_minus_1": float((pm.probs.double().sum(-1) - 1).abs().max())}
    for k, v in res["ms"].items():
        print(f"{k:10s} median {v['median']:.2f} ms  (min {v['min']:.2f}, max {v['max']:.2f}) over {args.runs} runs")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
