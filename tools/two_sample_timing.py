"""What the MMD two-sample sums cost, on one GPU in one process: one npfn_mmd_sums call
(npe_pfn.engine.mmd_sums) on device tensors of 64 observations x (1000 + 1000) pooled points x 10
dimensions, without permutations (P = 0, one labelling) and with P = 1000, against a torch
restatement of the reference's dense formula on the same device: per observation the N x N fp32
kernel matrix K (squared distances from a matrix product, the kernels summed over the
bandwidths), stored for all observations, and the within-group sums l^T K l of every labelling
from it by a batched matrix product (recomputed from the stored K for P = 1000, as a permutation
test on top of the reference's code would).

Each timed window is --iters back-to-back calls ending in a device synchronise; the figure is the
window over --iters.  After --warmup windows of each, median / min / max of --runs windows, the two
sides alternating.  The peak memory of each side is the rise of torch.cuda.max_memory_allocated
over one call (inputs excluded).  The two sides' biased MMD^2 of the observed split are compared
(they differ by fp32 rounding, not exactly) before anything is timed.  Records what the calls cost;
asserts nothing else.  Writes the same as JSON when --out is given.

    python tools/two_sample_timing.py [--runs 5] [--warmup 1] [--iters 5] [--out FILE.json]
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

from npe_pfn.diagnostics import MMD_DEFAULT_BANDWIDTHS, MMD_SCALE, permutation_labels  # noqa: E402
from npe_pfn.engine import mmd_sums  # noqa: E402


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, iters=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, r


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del r
    return rise


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--per", type=int, default=1000, help="draws per set (n = m)")
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--kernel", default="rbf", choices=sorted(MMD_DEFAULT_BANDWIDTHS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("two_sample_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    M, n, D = args.obs, args.per, args.dim
    N = 2 * n
    bw = MMD_DEFAULT_BANDWIDTHS[args.kernel]
    gen = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(M, N, D, device=dev, generator=gen)
    z[:, n:] += 0.25

    def dense_kernel():
        sq = (z * z).sum(-1)
        d2 = (sq[:, :, None] + sq[:, None, :] - 2.0 * torch.bmm(z, z.transpose(1, 2))).clamp_(min=0.0)
        K = torch.zeros_like(d2)
        for a in bw:
            K += torch.exp(-0.5 * d2 / a) if args.kernel == "rbf" else a ** 2 / (a ** 2 + d2)
        return K

    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "iters_per_window": args.iters, "kernel": args.kernel, "bandwidths": list(bw),
           "shape": {"observations": M, "n": n, "m": n, "dim": D}, "cases": {}}
    for P in (0, args.perms):
        labels = permutation_labels(n, n, P, seed=0).to(dev)
        lab_f = labels.to(torch.float32)

        def ours():
            return mmd_sums(z, labels, args.kernel, bw)

        def dense():
            K = dense_kernel()                                    # [M, N, N], stored
            LK = torch.matmul(lab_f[None], K)                     # [M, P + 1, N]
            s0 = (LK * lab_f[None]).sum(-1)
            LcK = torch.matmul((1.0 - lab_f)[None], K)
            s1 = (LcK * (1.0 - lab_f)[None]).sum(-1)
            return s0, s1, K.sum((1, 2))

        sums, total, _ = ours()
        s0, s1, tot = dense()
        stat = lambda a, b, t: (a + b - (t - a - b)) / (n * n)  # noqa: E731  (n == m)
        mine = stat(sums[:, 0, 0].double() / MMD_SCALE, sums[:, 0, 1].double() / MMD_SCALE, total.double() / MMD_SCALE)
        theirs = stat(s0[:, 0].double(), s1[:, 0].double(), tot.double())
        max_diff = float((mine - theirs).abs().max())
        del sums, total, s0, s1, tot
        mem = {"mmd_sums": peak_rise(ours), "torch_dense": peak_rise(dense)}
        for _ in range(args.warmup):
            timed(ours, args.iters), timed(dense, args.iters)
        t = {"mmd_sums": [], "torch_dense": []}
        for _ in range(args.runs):
            t["mmd_sums"].append(timed(ours, args.iters)[0])
            t["torch_dense"].append(timed(dense, args.iters)[0])
        med = {k: statistics.median(v) for k, v in t.items()}
        res["cases"][f"P={P}"] = {"labellings": P + 1, "ms_per_call": {k: summary(v) for k, v in t.items()},
                                  "torch_dense_over_mmd_sums": med["torch_dense"] / med["mmd_sums"],
                                  "peak_memory_bytes": mem,
                                  "pair_evaluations_per_s": M * N * N / (med["mmd_sums"] * 1e-3),
                                  "max_abs_diff_mmd2_biased": max_diff}
        for k, v in res["cases"][f"P={P}"]["ms_per_call"].items():
            print(f"P={P:5d} {k:12s} median {v['median']:.3f} ms (min {v['min']:.3f}, max {v['max']:.3f}), peak "
                  f"{mem[k] / 2 ** 20:.1f} MiB")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
