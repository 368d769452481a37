"""Golden outputs of the small forward at every row-tile and key-tile boundary (the oracle alone).

    python tests/golden/make_golden_forward_shapes.py      (~2 min on 8 cores; no GPU, no reference)

For every case of tests/forward_shapes_ref.py (CASES: the token-count edges, the context-row and
query-block edges, the mixed ensemble launch, the per-sublayer kernels' own boundary) the CPU
oracle (oracle/tabpfn_oracle.py) runs twice, bf16-emulating and plain fp32, on
ModelConfig(n_layers=3, n_bars=250, n_estimators=2) with synthetic_weights(cfg, seed=0) and
random_state 3.  Writes tests/golden/forward_shapes.npz with, per case, under "<name>/...":

* shape           [F, n, N, E, random_state]: the inputs are redrawn from these (table())
* tokens_per_row  [E] tokens per row the fit produced for each estimator
* rows            the query rows stored at full resolution (edge_rows(): every row up to 33
                  query rows, the rows at the tile and block edges past that)
* probs           [E, len(rows), 250] float16: the emulating oracle's softmax(logits_e / T)
* tokens          [E, len(rows), 192] bf16 bits: its target_tokens
* coarse          [E, N, 25] float16, cases with more than 33 query rows only: the same
                  probabilities of EVERY row summed over bins of 10 bars
* d_ref           largest per-row, per-estimator TV between the emulating and the fp32 oracle
* t_ref           largest per-row, per-estimator relative L2 distance of their tokens

d_ref and t_ref are taken over every row at full resolution.  float16 probabilities are within
2^-11 relative of the oracle's, i.e. within 2.5e-4 TV, a fiftieth of the smallest bound (4 d_ref)
the tests derive from them.  Every row at full resolution would be 3 MB, hence rows / coarse.
"""

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "npe-pfn_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import forward_shapes_ref as fs  # noqa: E402


def main():
    out = {}
    for case in fs.CASES:
        t0 = time.time()
        g = fs.golden_arrays(case)
        if case.name == "C_F254":
            assert tuple(g["tokens_per_row"]) == fs.SET_C_TOKENS, g["tokens_per_row"]
        else:
            assert set(g["tokens_per_row"]) == {case.C}, g["tokens_per_row"]
        assert np.isfinite(g["probs"].astype(np.float64)).all()
        for k, v in g.items():
            out[f"{case.name}/{k}"] = v
        print(f"{case.name:12s} tokens per row {tuple(g['tokens_per_row'])} n {case.n:3d} N {case.N:3d} "
              f"rows stored {len(g['rows']):3d}  d_ref {g['d_ref']:.5f}  t_ref {g['t_ref']:.5f}  "
              f"({time.time() - t0:.1f} s)", flush=True)
    path = os.path.join(HERE, fs.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print(f"wrote {fs.GOLDEN_FILE}: {os.path.getsize(path)} bytes, {len(fs.CASES)} cases")


if __name__ == "__main__":
    main()
