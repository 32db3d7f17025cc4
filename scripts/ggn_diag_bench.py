"""Timing of the exact GGN diagonal (compute_ggn_diag / lip_vjp_sqsum) against the route it replaces.

Prints one JSON line per case:
  * cifar_diag      compute_ggn_diag at the CIFAR config (ResNet1M, n = 50, K = 10)
  * cifar_rows_sq   (vjp_rows(one-hots, "l") ** 2).sum((0, 1)) on the same binding: the (n K, D) factor-row route
  * r50_diag        compute_ggn_diag of ResNet-50 at 224 x 224, K = 1000, 2 images (the rows route would need ~200 GB)
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/ggn_diag_bench.py [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from lip_amd.ggn import compute_ggn_diag, get_engine  # noqa: E402
from lip_amd.scalemodels import ResNet1M, ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def emit(case, ms, **kw):
    med, lo, hi = ms
    print(json.dumps(dict(case=case, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-r50", action="store_true")
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = torch.device("cuda")

    net = ResNet1M(10)
    state = create_state(net, seed=1231231234, dtype=torch.float32)
    Z = torch.rand(50, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    full = 49000
    eng = get_engine(state, Z, "classifier")
    emit("cifar_diag", timed(lambda: compute_ggn_diag(state, Z, "classifier", full_set_size=full), reps, args.warmup),
         D=eng.D, n=eng.n, K=eng.K, intermediate_bytes=0)
    E = torch.eye(eng.K, device=dev)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()
    emit("cifar_rows_sq", timed(lambda: (eng.vjp_rows(E, "l") ** 2).sum((0, 1)), reps, args.warmup),
         D=eng.D, n=eng.n, K=eng.K, intermediate_bytes=4 * eng.n * eng.K * eng.D)
    emit("cifar_rows_only", timed(lambda: eng.vjp_rows(E, "l"), reps, args.warmup), D=eng.D, n=eng.n, K=eng.K)

    if not args.skip_r50:
        net50 = ResNet50(1000)
        st50 = create_state(net50, seed=3, dtype=torch.float32)
        Z50 = torch.rand(2, 224, 224, 3, generator=torch.Generator().manual_seed(3)).to(dev)
        e50 = get_engine(st50, Z50, "classifier")
        emit("r50_diag", timed(lambda: compute_ggn_diag(st50, Z50, "classifier"), reps, args.warmup),
             D=e50.D, n=e50.n, K=e50.K, probe_chunk=e50.chunk, rows_route_bytes=4 * e50.n * e50.K * e50.D)


if __name__ == "__main__":
    main()
