"""Timing of the Monte-Carlo softmax link ``lip_link_mc`` next to the torch expression it replaces (``randn`` -> affine ->
``softmax`` -> ``mean`` over an (S, n, K) float32 tensor of logit draws), and of the two kernel paths of the variance
form on either side of the launcher's switch.

Prints one JSON line per case:
  * diag_kernel / diag_torch, factor_kernel / factor_torch at (n, K, S) = (256, 10, 1000), diag at (256, 1000, 1000):
    the time of ``--iters`` calls, ten times as many at K <= 64 (CUDA events on the current stream around the whole
    loop, which ends in a synchronise; a call is ``link.mc_predictive``, output allocation and flag check included;
    warm-up loops first; median, min and max over ``--reps`` loops), the peak of ``torch.cuda.max_memory_allocated``
    above the resident operands during one call, and the largest difference between the two routes' probabilities
    (two Monte-Carlo estimates from different generators: it measures the sampling noise, about 1 / sqrt(S)).
  * switch_K<k>_lane / switch_K<k>_wave: the variance form at (256, k, 1000) forced onto the lane-per-draw and the
    wave-per-draw path (``lip_debug_link_lane_max_k``), for the K around the switch.

    python scripts/link_bench.py [--iters 20] [--reps 5] [--warmup 1] [--dry-run]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from evidence_bench import peak_over  # noqa: E402
from kfac_bench import emit, timed  # noqa: E402
from lip_amd import _native as nv  # noqa: E402
from lip_amd.link import mc_predictive  # noqa: E402

F64 = torch.float64
SHAPES = [("diag", 256, 10, 1000), ("factor", 256, 10, 1000), ("diag", 256, 1000, 1000)]
SWITCH_K = (8, 16, 24, 32, 40, 48, 64)


def operands(form, n, K, dev):
    g = torch.Generator().manual_seed(7)
    mean = (16.0 * torch.rand(n, K, dtype=F64, generator=g) - 8.0).to(dev)
    if form == "diag":
        return mean, (2.0 * torch.rand(n, K, dtype=F64, generator=g)).square().to(dev), None
    A = torch.randn(n, K, 2 * K, dtype=F64, generator=g) * (1.2 / (2 * K) ** 0.5)
    return mean, None, torch.linalg.cholesky(A @ A.transpose(-1, -2)).float().to(dev)


def torch_link(mean, var, L, S):
    """the expression the kernel replaces: an (S, n, K) float32 tensor of draws, softmax, mean"""
    m = mean.float()
    eps = torch.randn((S,) + tuple(m.shape), device=m.device, dtype=torch.float32)
    z = m + (var.float().sqrt() * eps if L is None else torch.einsum("nkj,snj->snk", L, eps))
    return torch.softmax(z, dim=-1).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true", help="build the operands on the CPU, print the shapes and stop")
    args = ap.parse_args()
    if args.dry_run:
        for form, n, K, S in SHAPES:
            mean, var, L = operands(form, n, K, "cpu")
            print(dict(form=form, n=n, K=K, S=S, draws_bytes=4 * S * n * K, torch_probs=tuple(torch_link(mean, var, L, 8).shape)))
        return
    if not torch.cuda.is_available():
        raise SystemExit("link_bench.py times the device kernel: no GPU found")
    dev = torch.device("cuda")
    lib = nv.load()
    for form, n, K, S in SHAPES:
        mean, var, L = operands(form, n, K, dev)
        iters = args.iters * (10 if K <= 64 else 1)          # the small shapes take tens of microseconds a call
        shape = dict(n=n, K=K, S=S, iters=iters)

        def kernel_loop(it=iters):
            for _ in range(it):
                out = mc_predictive(mean, f_var=var, factor=L, num_samples=S, seed=1)
            return out

        def torch_loop(it=iters):
            for _ in range(it):
                out = torch_link(mean, var, L, S)
            return out

        diff = float((kernel_loop(1)[0].float() - torch_loop(1)).abs().max())
        emit(f"{form}_kernel", timed(kernel_loop, args.reps, args.warmup), peak_extra_bytes=peak_over(lambda: kernel_loop(1)),
             max_abs_diff=diff, **shape)
        emit(f"{form}_torch", timed(torch_loop, args.reps, args.warmup), peak_extra_bytes=peak_over(lambda: torch_loop(1)),
             max_abs_diff=diff, **shape)
        del mean, var, L
        torch.cuda.empty_cache()
    before = lib.lip_debug_link_lane_max_k(-1)
    try:
        for K in SWITCH_K:
            mean, var, _ = operands("diag", 256, K, dev)
            for name, cap in (("lane", 64), ("wave", 0)):
                lib.lip_debug_link_lane_max_k(cap)
                emit(f"switch_K{K}_{name}", timed(lambda: [mc_predictive(mean, f_var=var, num_samples=1000, seed=1)
                                                           for _ in range(10 * args.iters)], args.reps, args.warmup),
                     n=256, K=K, S=1000, iters=10 * args.iters)
    finally:
        lib.lip_debug_link_lane_max_k(before)


if __name__ == "__main__":
    main()
