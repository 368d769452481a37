"""What the classifier two-sample test costs, on one GPU in one process: one c2st_batched call on
device tensors (npfn_c2st_fit, one workgroup per observation and fold), against the same training
as the reference harness does it -- torch modules, torch.optim.Adam, F.cross_entropy and autograd,
fold after fold, batch after batch, with the same folds, order and init -- on this machine's CPU
and on the same GPU (device="cuda").  Case: n = m = 1000 draws in d = 10, the "mlp" classifier and
the defaults (5 folds, 100 epochs, batches of 128); the device side at M = 1 and M = 64
observations, both torch sides at ONE observation only (64 would take the better part of an hour
on the CPU).  The M = 64 ratios multiply the torch sides' per-observation time by 64: they are
computed, not measured.

Each device window is one call ending in a device synchronise.  After --warmup windows, the median
/ min / max of --runs windows of the device side; the torch sides are warmed by one epoch of one
fold and timed over --torch-runs whole trainings.  The C2ST values of all three sides are recorded
(the torch sides round differently, so they agree to a few held-out points, not to the bit).
Records what the calls cost; asserts nothing.  Writes the same as JSON when --out is given.

    python tools/c2st_timing.py [--runs 3] [--warmup 1] [--torch-runs 1] [--out FILE.json]
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
import torch.nn.functional as F  # noqa: E402

from npe_pfn.diagnostics import c2st_batched, c2st_folds, c2st_init, c2st_order, c2st_widths  # noqa: E402

N, D, MODEL, FOLDS, EPOCHS, BATCH, LR, SEED = 1000, 10, "mlp", 5, 100, 128, 1e-3, 1
OBSERVATIONS = (1, 64)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def torch_c2st(a, b, device, epochs=EPOCHS, folds=None):
    """The reference's loop for one observation (a, b [n, d] on the CPU), trained on ``device``:
    the mean held-out accuracy over the folds."""
    n, m = a.shape[0], b.shape[0]
    mu, sd = a.mean(0), a.std(0)
    sd = torch.where(sd == 0, torch.ones_like(sd), sd)
    z = torch.cat([(a - mu) / sd, (b - mu) / sd]).to(device)
    label = (torch.arange(n + m) >= n).long().to(device)
    fold = c2st_folds(n, m, FOLDS, SEED)
    order = c2st_order(n + m, epochs, SEED).long()
    widths = c2st_widths(MODEL, a.shape[1])
    init = c2st_init(widths, SEED)
    scores = []
    for f in range(FOLDS) if folds is None else folds:
        layers, off = [], 0
        for i, o in zip(widths[:-1], widths[1:]):
            lin = torch.nn.Linear(i, o)
            with torch.no_grad():
                lin.weight.copy_(init[off:off + o * i].view(o, i))
                lin.bias.copy_(init[off + o * i:off + o * i + o])
            off += o * i + o
            layers += [lin, torch.nn.ReLU()]
        net = torch.nn.Sequential(*layers[:-1]).to(device)
        opt = torch.optim.Adam(net.parameters(), lr=LR)
        for e in range(epochs):
            row = order[e]
            row = row[fold[row] != f].to(device)
            for b0 in range(0, row.numel(), BATCH):
                idx = row[b0:b0 + BATCH]
                opt.zero_grad()
                F.cross_entropy(net(z[idx]), label[idx]).backward()
                opt.step()
        held = torch.nonzero(fold == f).reshape(-1).to(device)
        with torch.no_grad():
            scores.append(float((net(z[held]).argmax(1) == label[held]).float().mean()))
    return sum(scores) / len(scores)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-runs", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("c2st_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(max(OBSERVATIONS), N, D, generator=gen)
    b = torch.randn(max(OBSERVATIONS), N, D, generator=gen) + 0.1
    res = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "host_threads": torch.get_num_threads(), "runs": args.runs, "warmup": args.warmup, "torch_runs": args.torch_runs,
           "case": {"n": N, "m": N, "dim": D, "model": MODEL, "n_folds": FOLDS, "epochs": EPOCHS, "batch_size": BATCH,
                    "lr": LR}, "c2st_batched": {}, "torch": {}}

    for M in OBSERVATIONS:
        ad, bd = a[:M].to(dev), b[:M].to(dev)

        def ours():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = c2st_batched(ad, bd, seed=SEED)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        for _ in range(args.warmup):
            ours()
        runs = [ours() for _ in range(args.runs)]
        t = [ms for ms, _ in runs]
        res["c2st_batched"][f"M={M}"] = {"observations": M, "ms_per_call": summary(t),
                                         "ms_per_observation": statistics.median(t) / M,
                                         "c2st_of_observation_0": float(runs[0][1].c2st[0])}
        print(f"c2st_batched M={M:2d}: median {statistics.median(t):.1f} ms (min {min(t):.1f}, max {max(t):.1f}), "
              f"c2st[0] = {float(runs[0][1].c2st[0]):.4f}")

    for name, device in (("cpu", torch.device("cpu")), ("cuda", dev)):
        torch_c2st(a[0], b[0], device, epochs=1, folds=[0])   # warm-up: one epoch of one fold
        t, value = [], None
        for _ in range(args.torch_runs):
            if device.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = torch_c2st(a[0], b[0], device)
            if device.type == "cuda":
                torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        res["torch"][name] = {"observations": 1, "ms_per_observation": summary(t), "c2st": value}
        print(f"torch on {name}: median {statistics.median(t):.0f} ms for one observation, c2st = {value:.4f}")

    ratios = {}
    for name in res["torch"]:
        per_obs = res["torch"][name]["ms_per_observation"]["median"]
        ratios[name] = {
            "M=1_measured": per_obs / res["c2st_batched"]["M=1"]["ms_per_call"]["median"],
            "M=64_torch_side_multiplied_out_not_measured": 64 * per_obs / res["c2st_batched"]["M=64"]["ms_per_call"]["median"]}
        print(f"torch on {name} / c2st_batched: {ratios[name]['M=1_measured']:.2f} at M = 1 (measured), "
              f"{ratios[name]['M=64_torch_side_multiplied_out_not_measured']:.1f} at M = 64 (64 x the one torch observation)")
    res["torch_over_c2st_batched"] = ratios
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
