"""The MMD of the reference's evaluation harness (scripts/evaluate_ropefm.py:283-320), in our own
words and in fp64: squared distances from ``torch.cdist``, the kernels summed over the bandwidths,
``mean(XX) + mean(YY) - 2 mean(XY)`` -- which is the reference's ``mean(XX + YY - 2 XY)`` at n == m
and its natural reading at n != m.  Test infrastructure only; runs on the CPU.
"""
import torch

BANDWIDTHS = {"rbf": (10.0, 15.0, 20.0, 50.0), "multiscale": (0.2, 0.5, 0.9, 1.3)}


def kernel_sum(x, y, kernel, bandwidths):
    d2 = torch.cdist(x, y) ** 2
    out = torch.zeros_like(d2)
    for a in bandwidths:
        out = out + (torch.exp(-0.5 * d2 / a) if kernel == "rbf" else a ** 2 / (a ** 2 + d2))
    return out


def mmd2(x, y, kernel="rbf", bandwidths=None) -> float:
    """Biased MMD^2 of x [n, d] against y [m, d], fp64."""
    x, y = torch.as_tensor(x).to(torch.float64), torch.as_tensor(y).to(torch.float64)
    bw = BANDWIDTHS[kernel] if bandwidths is None else bandwidths
    return float(kernel_sum(x, x, kernel, bw).mean() + kernel_sum(y, y, kernel, bw).mean()
                 - 2.0 * kernel_sum(x, y, kernel, bw).mean())
