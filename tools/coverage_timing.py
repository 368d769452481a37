"""What the coverage ranks cost, on one GPU in one process:

  (a) the kernel against torch: one Engine.rank_accumulate call on device tensors of the benchmark
      configuration c5's shape (64 observations x 10 000 draws x 10 dimensions) against the same
      counts from torch expressions on the same tensors (comparisons, sum(1), the fp64 distances of
      npe_pfn.diagnostics.rank_accumulate_host).  Each timed window is --iters back-to-back calls
      ending in a device synchronise; the figure is the window over --iters.  The two results are
      compared with torch.equal before anything is timed.
  (b) the whole call against the route without it, on Gaussian-linear 10-D with 1000 simulations,
      64 observations and 1000 posterior draws each (TabPFN_Based_NPE_PFN with its defaults):
      coverage_batched(theta_true, x, 1000) -- with its default max_sampling_batch_size (blocks of
      6 observations) and with one block for all 64 -- against log_prob_batched +
      sample_batched(with_log_prob=True) + the torch ranks on the stored draws, alternating.

After a warm-up of each, median / min / max of --runs runs; every timed call ends in a device
synchronise.  It records what the calls cost and asserts nothing but the equality in (a); writes
the same as JSON when --out is given.

    python tools/coverage_timing.py [--runs 5] [--warmup 1] [--iters 20] [--out FILE.json]
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

from npe_pfn.diagnostics import rank_accumulate_host  # noqa: E402
from npe_pfn.npe_pfn import TabPFN_Based_NPE_PFN  # noqa: E402
from npe_pfn.tasks import gaussian_linear, gaussian_linear_prior, gaussian_linear_task  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, iters=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, r


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--per", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--sims", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("coverage_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    theta, x, _ = (t.to(dev) for t in gaussian_linear_task(args.dim, args.sims, seed=0))
    prior = gaussian_linear_prior(args.dim, device=dev)
    post = TabPFN_Based_NPE_PFN(prior=prior, regressor_init_kwargs={"random_state": 0, "device": "cuda:0"})
    post.append_simulations(theta, x)
    eng = post._model.engine

    # ---------------------------------------------------------------- (a) kernel against torch
    M, P, D = args.obs, args.per, args.dim
    gen = torch.Generator(device=dev).manual_seed(1)
    draws = torch.randn(M * P, D, device=dev, generator=gen)
    logp = torch.randn(M * P, device=dev, generator=gen)
    take = torch.rand(M * P, device=dev, generator=gen) < 0.67
    truth = torch.randn(M, D, device=dev, generator=gen)
    logp_true = torch.randn(M, device=dev, generator=gen)
    ref = torch.randn(M, D, device=dev, generator=gen)
    inv_scale = torch.rand(D, device=dev, generator=gen) + 0.5
    counts = torch.zeros((M, D + 2, 2), dtype=torch.int64, device=dev)

    def kernel():
        counts.zero_()
        eng.rank_accumulate(draws, logp, take, M, P, truth, logp_true, ref, inv_scale, counts)
        return counts

    def torch_form():
        # the definition with the fp32 inputs compared as they are (only the distances go to fp64)
        c = torch.zeros((M, D + 2, 2), dtype=torch.int64, device=dev)
        th, on = draws.view(M, P, D), take.view(M, P)
        c[:, :D, 0] = ((th < truth[:, None, :]) & on[:, :, None]).sum(1)
        c[:, :D, 1] = ((th == truth[:, None, :]) & on[:, :, None]).sum(1)
        lp = logp.view(M, P)
        c[:, D, 0] = ((lp > logp_true[:, None]) & on).sum(1)
        c[:, D, 1] = ((lp == logp_true[:, None]) & on).sum(1)
        d2 = torch.zeros((M, P), dtype=torch.float64, device=dev)
        d2t = torch.zeros(M, dtype=torch.float64, device=dev)
        sc = inv_scale.double()
        for k in range(D):
            a = (th[:, :, k].double() - ref[:, None, k].double()) * sc[k]
            b = (truth[:, k].double() - ref[:, k].double()) * sc[k]
            d2 = d2 + a * a
            d2t = d2t + b * b
        c[:, D + 1, 0] = ((d2 < d2t[:, None]) & on).sum(1)
        c[:, D + 1, 1] = ((d2 == d2t[:, None]) & on).sum(1)
        return c

    a_equal = torch.equal(kernel().clone(), torch_form())
    if not a_equal:
        sys.exit("coverage_timing: the kernel's counts differ from the torch form's")
    for _ in range(args.warmup):
        timed(kernel, args.iters), timed(torch_form, args.iters)
    ta = {"rank_accumulate": [], "torch": []}
    for _ in range(args.runs):
        ta["rank_accumulate"].append(timed(kernel, args.iters)[0])
        ta["torch"].append(timed(torch_form, args.iters)[0])
    table_bytes = M * P * (D * 4 + 4 + 1)

    # ---------------------------------------------------------------- (b) whole call against today's route
    n_obs, S = args.obs, args.samples
    torch.manual_seed(0)
    th_true = prior.sample((n_obs,))
    x_true = gaussian_linear(th_true)
    refs = prior.sample((n_obs,))

    def coverage():
        return post.coverage_batched(th_true, x_true, S, references=refs)

    def coverage_one_block():
        return post.coverage_batched(th_true, x_true, S, references=refs,
                                     max_sampling_batch_size=n_obs * int(S * 1.5))

    def route():
        lp_true = post.log_prob_batched(th_true, x_true)
        smp, slp = post.sample_batched(x_true, (S,), with_log_prob=True)
        c = torch.zeros((n_obs, args.dim + 2, 2), dtype=torch.int64, device=dev)
        lo, hi = theta.min(0).values, theta.max(0).values
        rank_accumulate_host(smp.reshape(n_obs * S, -1), slp.reshape(-1), None, n_obs, S, th_true, lp_true, refs,
                             1.0 / (hi - lo), c)
        return c

    fns = {"coverage_batched": coverage, "coverage_batched_one_block": coverage_one_block,
           "log_prob_batched+sample_batched+torch_ranks": route}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    tb = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():
            tb[k].append(timed(fn)[0])

    med_a = {k: statistics.median(v) for k, v in ta.items()}
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "kernel_vs_torch": {"shape": {"observations": M, "draws_per_observation": P, "dim": D},
                               "iters_per_window": args.iters, "equal": a_equal,
                               "ms_per_call": {k: summary(v) for k, v in ta.items()},
                               "torch_over_kernel": med_a["torch"] / med_a["rank_accumulate"],
                               "table_bytes": table_bytes,
                               "kernel_table_GBps": table_bytes / (med_a["rank_accumulate"] * 1e-3) / 1e9},
           "whole_call": {"task": {"name": "gaussian_linear", "dim": args.dim, "simulations": args.sims,
                                   "observations": n_obs, "posterior_samples": S, "preprocessing": "ensemble"},
                          "ms": {k: summary(v) for k, v in tb.items()}}}
    for k, v in res["kernel_vs_torch"]["ms_per_call"].items():
        print(f"(a) {k:16s} median {v['median']:.4f} ms  (min {v['min']:.4f}, max {v['max']:.4f})")
    for k, v in res["whole_call"]["ms"].items():
        print(f"(b) {k:44s} median {v['median']:.1f} ms  (min {v['min']:.1f}, max {v['max']:.1f})")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
