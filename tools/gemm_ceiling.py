"""Ceiling for the decoder head GEMM: torch.matmul in bf16 on the same shape.

bench.py c2 runs the bar-head product [E * rows, d_ff] x [d_ff, n_bars] = [80 000, 768] x
[768, 5000] once per AR step (10 per call) in k_gemm<EPI_LOGIT>.  This times the vendor GEMM
behind torch.matmul on that shape (fp32 accumulation, bf16 output -- the engine writes fp16 rows,
the same bytes).  It is a yardstick for the kernel tables only and never enters the product.

usage: python tools/gemm_ceiling.py [--m 80000] [--k 768] [--n 5000] [--iters 50]
Prints one JSON line: ms per product, TF/s, and ms per c2 call (10 products).
"""
import argparse
import json

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=80_000)
ap.add_argument("--k", type=int, default=768)
ap.add_argument("--n", type=int, default=5000)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
a = torch.randn(args.m, args.k, device=dev, generator=g).to(torch.bfloat16)
w = torch.randn(args.n, args.k, device=dev, generator=g).to(torch.bfloat16)   # [N, K], as the engine keeps W2
out = torch.empty(args.m, args.n, device=dev, dtype=torch.bfloat16)
for _ in range(args.warmup):
    torch.matmul(a, w.t(), out=out)
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
t0.record()
for _ in range(args.iters):
    torch.matmul(a, w.t(), out=out)
t1.record()
torch.cuda.synchronize()
ms = t0.elapsed_time(t1) / args.iters
flops = 2.0 * args.m * args.n * args.k
print(json.dumps({"shape": [args.m, args.k, args.n], "dtype": "bf16", "ms_per_product": round(ms, 4),
                  "tflops": round(flops / ms / 1e9, 1), "ms_per_c2_call": round(10 * ms, 3),
                  "device": torch.cuda.get_device_name(0)}))
