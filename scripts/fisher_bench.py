"""Timing and accuracy of the Monte-Carlo and empirical Fisher fits (``lip_amd.fisher``) next to the exact GGN fits.

Prints one JSON line per case:
  * head_sample      ``lip_head_sample`` alone at (n, K, S) = (256, 1000, 16) and (1000, 10, 64): time and achieved write
                     bandwidth 4 S n K / t (--kernel-only stops after it)
  * diag / kfac      ``compute_ggn_diag`` / ``compute_kfac_factors`` on warm bindings, per curvature: exact (K one-hot
                     probes), MCFisher(1), MCFisher(10), EmpiricalFisher — at ResNet-50, K = 1000 (--r50-n images of
                     --r50-res pixels) and at the CIFAR config (ResNet1M, K = 10, --n examples in one binding)
  * mc_error         relative L1 error sum|d_mc - d| / sum|d| of the MC diagonal against the exact one at the CIFAR
                     config for S = 1, 4, 16 over --m examples in chunks of --chunk (seeds 0..2, the mean and the worst)
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions (min, max).

    python scripts/fisher_bench.py [--reps 5] [--warmup 2] [--n 50] [--m 1000] [--chunk 50] [--r50-n 8] [--r50-res 224] [--kernel-only]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from kfac_bench import emit, timed  # noqa: E402
from lip_amd.fisher import EmpiricalFisher, MCFisher, sample_head_cotangents  # noqa: E402
from lip_amd.ggn import clear_engine_cache, compute_ggn_diag, compute_kfac_factors  # noqa: E402
from lip_amd.scalemodels import ResNet1M, ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402


def fits(tag, state, Z, K, chunk, reps, warmup, exact_reps):
    g = torch.Generator().manual_seed(5)
    specs = [("exact", None), ("mc1", MCFisher(1, 1)), ("mc10", MCFisher(10, 1)),
             ("ef", EmpiricalFisher(torch.randint(0, K, (Z.shape[0],), generator=g)))]
    for what, fn in (("diag", lambda s: compute_ggn_diag(state, Z, "classifier", example_chunk=chunk, curvature=s)),
                     ("kfac", lambda s: compute_kfac_factors(state, Z, "classifier", example_chunk=chunk, curvature=s))):
        base = None
        for name, spec in specs:
            r = exact_reps if spec is None else reps
            ms = timed(lambda: fn(spec), r, min(warmup, r))
            base = ms[0] if spec is None else base
            emit(f"{what}/{tag}/{name}", ms, M=Z.shape[0], K=K, chunk=chunk, exact_over_this=round(base / ms[0], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--r50-n", type=int, default=8)
    ap.add_argument("--r50-res", type=int, default=224)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")

    for n, K, S in ((256, 1000, 16), (1000, 10, 64)):
        p = torch.softmax(4.0 * torch.randn(n, K, device=dev), dim=-1).contiguous()
        ms = timed(lambda: sample_head_cotangents(p, S, 3), 20, 5)
        emit("head_sample", ms, n=n, K=K, S=S, bytes_written=4 * S * n * K, GBps=round(4 * S * n * K / ms[0] / 1e6, 1))
    if args.kernel_only:
        return

    g = torch.Generator().manual_seed(280300)
    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    Z = torch.rand(args.m, 32, 32, 3, generator=g).to(dev)
    chunk = args.chunk if args.chunk < args.m else None
    fits("cifar", state, Z[:args.n].contiguous(), 10, None, args.reps, args.warmup, args.reps)      # one cached binding
    exact = compute_ggn_diag(state, Z, "classifier", example_chunk=chunk).double()
    for S in (1, 4, 16):
        errs = [float((compute_ggn_diag(state, Z, "classifier", example_chunk=chunk, curvature=MCFisher(S, seed)).double()
                       - exact).abs().sum() / exact.abs().sum()) for seed in range(3)]
        emit("mc_error", (0.0, 0.0, 0.0), S=S, M=args.m, rel_l1_mean=round(sum(errs) / 3, 4), rel_l1_worst=round(max(errs), 4))
    del exact
    clear_engine_cache()
    torch.cuda.empty_cache()

    state = create_state(ResNet50(1000, input_shape=(args.r50_res, args.r50_res, 3)), seed=1, dtype=torch.float32)
    Z = torch.rand(args.r50_n, args.r50_res, args.r50_res, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    fits("resnet50", state, Z, 1000, None, args.reps, args.warmup, 1)


if __name__ == "__main__":
    main()
