"""numpy restatement of the restricted prior's rejection round (include/npfn.h
``npfn_box_propose`` / ``npfn_restricted_box_round``) and of the kept counts of
``NPE_PFN_RestrictedPrior.append_simulations``.

Test infrastructure only: written from the statements in the header and in DESIGN.md, not from
the product's code, so that the two can be held against each other.  Every intermediate of the
proposals is float32, rounded operation by operation.
"""
from __future__ import annotations

import numpy as np

from oracle.philox import uniforms


def proposals(low, high, n: int, seed: int, counter: int, row_base: int = 0) -> np.ndarray:
    """out[i, j] = min(low[j] + u * (high[j] - low[j]), high[j]) with
    u = uniforms(seed, counter + j, row row_base + i); [n, dim] float32."""
    low = np.asarray(low, dtype=np.float32).reshape(-1)
    high = np.asarray(high, dtype=np.float32).reshape(-1)
    dim = low.shape[0]
    out = np.empty((n, dim), dtype=np.float32)
    for j in range(dim):
        u = uniforms(seed, counter + j, n, row_base).astype(np.float32)
        span = np.float32(high[j] - low[j])
        t = (u * span).astype(np.float32)
        x = (low[j] + t).astype(np.float32)
        out[:, j] = np.minimum(x, high[j])
    assert out.dtype == np.float32
    return out


def append(theta_out: np.ndarray, counts, rows: np.ndarray, mask: np.ndarray, capacity: int):
    """The ordered append: accepted ``rows`` go, in order, to theta_out[counts[0]:] while they
    fit below ``capacity``.  Returns (theta_out copy, [stored, accepted])."""
    theta_out = np.array(theta_out, dtype=np.float32, copy=True)
    stored, accepted = int(counts[0]), int(counts[1])
    acc = np.asarray(rows, dtype=np.float32)[np.asarray(mask, dtype=bool)]
    take = max(0, min(acc.shape[0], capacity - stored))
    theta_out[stored:stored + take] = acc[:take]
    assert 0 <= stored <= capacity
    return theta_out, [min(capacity, stored + acc.shape[0]), accepted + acc.shape[0]]


def kept_counts(n0: int, n1: int, max_rows: int):
    """(rows of class 0, rows of class 1) kept for the classifier fit: each class at most
    H = max_rows // 2, except that a class takes the room the other leaves below H, as far as
    it has distinct rows."""
    half = max_rows // 2
    if n0 >= half and n1 >= half:
        return half, half
    if n1 < half and n0 < half:
        return n0, n1
    if n1 < half:
        return min(n0, max_rows - n1), n1
    return n0, min(n1, max_rows - n0)


def next_batch(remaining: int, accepted: int, proposed: int, max_bs: int) -> int:
    """The rejection loop's batch schedule after the first batch min(n, max_bs)."""
    rate = accepted / proposed
    return min(max_bs, max(int(1.5 * remaining / max(rate, 1e-12)), 100))


def sample_stream(predict_last, low, high, n: int, seed: int, counter: int, threshold: float, max_bs: int):
    """First n accepted rows of the row stream, driven round by round on the schedule;
    ``predict_last(rows) -> p`` is the classifier's last-class probability.
    Returns (samples [n, dim], accepted, proposed)."""
    dim = np.asarray(low).reshape(-1).shape[0]
    out = np.zeros((n, dim), dtype=np.float32)
    counts = [0, 0]
    proposed = 0
    batch = min(n, max_bs)
    while counts[0] < n:
        rows = proposals(low, high, batch, seed, counter, proposed)
        mask = np.asarray(predict_last(rows)) > np.float32(threshold)
        out, counts = append(out, counts, rows, mask, n)
        proposed += batch
        batch = next_batch(n - counts[0], counts[1], proposed, max_bs)
    return out, counts[1], proposed
