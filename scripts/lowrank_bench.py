"""Timing of the low-rank Laplace posterior at the CIFAR config (ResNet1M, D = 1.08 M, K = 10): the matrix-free fit over
M examples bound in chunks, the closed-form predictive of a 256-image batch, and the marginal variance through
``lip_cols_wsqsum`` next to the torch expression it replaces.

Prints one JSON line per case:
  * cols_wsqsum      the kernel alone on random (rank, D) rows, into a vector at hand (--kernel-only stops after it)
  * bind             binding the M examples in chunks (the primal passes; once, wall clock)
  * ggn_block        one P-probe GGN-vp block over all chunks (one pass over the data)
  * fit              compute_ggn_lowrank: power_iters + 2 passes and the dense steps
  * predict          predict_lla_lowrank, 256 test images, cov="diag", on the cached fit
  * variance         LowRankNormal.variance() (lip_cols_wsqsum, the zero fill and the (1 - q) / a epilogue)
  * variance_torch   (s[:, None] * Ut.double() ** 2).sum(0): two (rank, D) float64 temporaries
  * variance_torch32 the same expression in float32 (what a user short of memory would write); its error is printed
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions (min, max).

    python scripts/lowrank_bench.py [--reps 10] [--warmup 3] [--m 1000] [--chunk 50] [--rank 248] [--oversample 8] [--kernel-only]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from kfac_bench import emit, timed  # noqa: E402
from lip_amd import krylov, lowrank  # noqa: E402
from lip_amd.ggn import clear_engine_cache  # noqa: E402
from lip_amd.lla import posterior_lla_lowrank, predict_lla_lowrank  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402
from lip_amd.utils import flatten_nn_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--rank", type=int, default=248)
    ap.add_argument("--oversample", type=int, default=8)
    ap.add_argument("--power-iters", type=int, default=1)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    g = torch.Generator().manual_seed(280300)
    Z = torch.rand(args.m, 32, 32, 3, generator=g).to(dev)
    Xnew = torch.rand(256, 32, 32, 3, generator=g).to(dev)
    D = flatten_nn_params(state.params)[0].numel()
    rows = torch.randn(args.rank, D, device=dev)
    w = torch.rand(args.rank, device=dev, dtype=torch.float64)
    acc = torch.zeros(D, device=dev, dtype=torch.float64)
    emit("cols_wsqsum", timed(lambda: krylov.cols_wsqsum(rows, w, out=acc), args.reps, args.warmup), rank=args.rank, D=D,
         bytes_read=4 * rows.numel())
    del rows, w, acc
    if args.kernel_only:
        return
    P = args.rank + args.oversample
    chunk = args.chunk if args.chunk < args.m else None
    shape = dict(M=args.m, chunk=args.chunk, rank=args.rank, P=P, power_iters=args.power_iters)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    matvec, _ = lowrank.ggn_operator(state, Z, "classifier", chunk)
    torch.cuda.synchronize()
    emit("bind", ((time.perf_counter() - t0) * 1e3,) * 3, **shape)
    V = torch.randn(P, D, device=dev)
    emit("ggn_block", timed(lambda: matvec(V), args.reps, args.warmup), D=D, **shape)
    del matvec, V
    torch.cuda.empty_cache()

    solver = dict(oversample=args.oversample, power_iters=args.power_iters)
    fit = lambda: lowrank.compute_ggn_lowrank(state, Z, "classifier", args.rank, example_chunk=chunk, **solver)   # noqa: E731
    ms = timed(fit, args.reps, args.warmup)                       # every call binds the chunks again: part of a fit
    lam, U, info = fit()
    emit("fit", ms, passes=info["passes"], dropped=info["dropped"], residual_max=float(info["residual"].max()),
         lam_max=float(lam[0]), lam_min=float(lam[-1]), **shape)
    del U
    clear_engine_cache()
    torch.cuda.empty_cache()

    alpha = 1e-3 * float(lam[0])
    kw = dict(rank=args.rank, example_chunk=chunk, **solver)
    post = posterior_lla_lowrank(state, Z, "classifier", alpha, **kw)          # fills the one-entry fit cache
    emit("predict", timed(lambda: predict_lla_lowrank(state, Xnew, Z, "classifier", alpha, cov="diag", **kw), args.reps,
                          args.warmup), **shape)
    emit("variance", timed(post.variance, args.reps, args.warmup), bytes_read=4 * post.Ut.numel(), **shape)
    t64 = lambda: (1.0 - (post.s[:, None] * post.Ut.double() ** 2).sum(0)) / post.a       # noqa: E731
    t32 = lambda: (1.0 - (post.s.float()[:, None] * post.Ut ** 2).sum(0)) / post.a        # noqa: E731
    emit("variance_torch", timed(t64, args.reps, args.warmup), **shape)
    emit("variance_torch32", timed(t32, args.reps, args.warmup), **shape)
    v = post.variance()
    emit("variance_error", (0.0, 0.0, 0.0), torch64=float((v - t64()).abs().max() / v.abs().max()),
         torch32=float((v - t32().double()).abs().max() / v.abs().max()))


if __name__ == "__main__":
    main()
