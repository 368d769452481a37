"""One rejection round of the restricted prior, two ways, at config c4's classifier context
(5 000 + 5 000 rows, 2 features, default ensemble preprocessing) with 10 000 proposals per
round, one GPU, one process:

  (a) Engine.restricted_box_round + the 16-byte readback of its counters
      -- proposals, forward, accept decision and ordered append on the device
  (b) the reference's shape of a round on the public calls: torch.rand proposals on the host
      -> TabPFNClassifier.predict_proba (numpy) -> mask -> boolean index
      (restricted_prior.py:25-28 inside sbi's rejection loop)

After a warm-up the two alternate; each timed round ends in a device synchronise.  Prints the
median, min, max and interquartile range of the rounds; writes the same as JSON when --out is
given.  It records what a round costs and asserts nothing.

    python tools/restricted_timing.py [--rounds 20] [--warmup 3] [--out FILE.json]
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

from npe_pfn.tabpfn import TabPFNClassifier  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20, help="timed rounds of each variant (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10000, help="proposals per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error("--rounds must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("restricted_timing: needs a ROCm GPU (no fallback: a CPU run measures nothing)")

    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    n_half, dim, N = 5000, 2, args.rows
    valid = torch.randn(n_half, dim, device=dev, generator=g) * 0.3 + 0.2
    invalid = torch.rand(n_half, dim, device=dev, generator=g) * 2 - 1
    clf = TabPFNClassifier(random_state=0, device="cuda:0")  # preprocessing="ensemble" is the default
    clf.fit(torch.cat([invalid, valid]), torch.cat([torch.zeros(n_half), torch.ones(n_half)]))
    eng = clf.engine
    low, high = eng.box_bounds(-1.0, 1.0, dim)
    # a threshold both outcomes occur at: the median probability of one batch of proposals
    thr = float(eng.predict_proba(eng.box_propose(N, dim, low, high, counter=0))[:, -1].median())

    theta_out = torch.empty((N, dim), dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    state = {"row_base": 0}

    def device_round():
        counts.zero_()
        eng.restricted_box_round(low, high, thr, N, 0, state["row_base"], theta_out, counts)
        state["row_base"] += N
        return counts.tolist()  # the round's one readback

    def host_round():
        theta = torch.rand(N, dim) * 2 - 1
        mask = torch.as_tensor(clf.predict_proba(theta)[:, -1] > thr)
        return theta[mask]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for _ in range(args.warmup):
        device_round(), host_round()
    names = ("restricted_box_round+readback", "rand+predict_proba+mask+index")
    t = {k: [] for k in names}
    accepted = {k: [] for k in names}
    for _ in range(args.rounds):
        ms, c = timed(device_round)
        t[names[0]].append(ms)
        accepted[names[0]].append(c[1])
        ms, kept = timed(host_round)
        t[names[1]].append(ms)
        accepted[names[1]].append(int(kept.shape[0]))

    def summary(v):
        q = statistics.quantiles(v, n=4)
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "q1": q[0], "q3": q[2]}

    res = {"device": torch.cuda.get_device_name(0),
           "context": {"rows": 2 * n_half, "features": dim, "preprocessing": clf.preprocessing},
           "proposals_per_round": N, "threshold": thr, "rounds": args.rounds, "warmup": args.warmup,
           "ms": {k: summary(v) for k, v in t.items()},
           "mean_accepted_per_round": {k: statistics.mean(v) for k, v in accepted.items()},
           "device_minus_host_ms": statistics.median(t[names[0]]) - statistics.median(t[names[1]])}
    for k, v in res["ms"].items():
        print(f"{k:32s} median {v['median']:.3f} ms  (min {v['min']:.3f}, max {v['max']:.3f}, "
              f"quartiles {v['q1']:.3f} .. {v['q3']:.3f}) over {args.rounds} rounds")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
