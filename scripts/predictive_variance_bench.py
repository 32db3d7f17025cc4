"""Timing and peak memory of the closed-form predictive variances against the routes they replace.

One JSON line per case; ``--case`` picks a group so that each can run as a step of its own:
  * cifar     ResNet1M, 50 inducing images, N = 49 000, a test batch of 256 images, K = 10
      cifar_predict_diag     predict_lla_diag (the posterior's GGN diagonal + one weighted-norm sweep)
      cifar_wnorm_sweep      the weighted-norm sweep alone (vjp_wnorm of K one-hot probes)
      cifar_rows_weighted    the rows route: vjp_rows (P, n, D), then the weighted square sum in torch
      cifar_diag_sampled     predict_lla_diag_scalable with 200 draws
  * marginals the same config:
      cifar_variances        predict_lla_variances
      cifar_marginals        predict_lla_marginals (the (B, K, D) rows and float64 products, batches of 64)
  * r50       ResNet-50 at 224 x 224, K = 1000, 2 inducing and 2 test images (the rows would take 205 GB)
      r50_predict_diag, r50_wnorm_sweep, r50_diag_sampled
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions; peak memory is
``torch.cuda.max_memory_allocated`` over one call, less what was allocated before it.

    python scripts/predictive_variance_bench.py --case cifar [--reps 7] [--warmup 2]
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
from lip_amd.ggn import get_engine  # noqa: E402
from lip_amd.lla import (posterior_lla_diag, predict_lla_diag, predict_lla_diag_scalable, predict_lla_marginals,  # noqa: E402
                         predict_lla_variances)
from lip_amd.scalemodels import ResNet1M, ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), peak


def emit(case, res, **kw):
    med, lo, hi, peak = res
    print(json.dumps(dict(case=case, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                          peak_bytes=int(peak), **kw)), flush=True)


def onehots(eng):
    return torch.eye(eng.K, device=eng.device)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["cifar", "marginals", "r50"], required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=200)
    args = ap.parse_args()
    reps, wu = max(3, args.reps), max(1, args.warmup)
    dev = torch.device("cuda")
    alpha = 0.005

    if args.case in ("cifar", "marginals"):
        state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
        g = torch.Generator().manual_seed(280300)
        Z = torch.rand(50, 32, 32, 3, generator=g).to(dev)
        X = torch.rand(256, 32, 32, 3, generator=g).to(dev)
        full, mt = 49000, "classifier"
        eng = get_engine(state, X, mt)
        dims = dict(D=eng.D, B=eng.n, K=eng.K)
        if args.case == "cifar":
            emit("cifar_predict_diag", timed(lambda: predict_lla_diag(state, X, Z, mt, alpha, full_set_size=full), reps, wu), **dims)
            w = posterior_lla_diag(state, Z, mt, alpha, full_set_size=full).variance()
            E = onehots(eng)
            emit("cifar_wnorm_sweep", timed(lambda: eng.vjp_wnorm(E, w, "raw"), reps, wu), **dims)
            emit("cifar_rows_weighted", timed(lambda: (eng.vjp_rows(E, "raw") ** 2) @ w, reps, wu),
                 rows_bytes=4 * eng.K * eng.n * eng.D, **dims)
            emit("cifar_diag_sampled", timed(lambda: predict_lla_diag_scalable(state, X, Z, mt, alpha, key=1, full_set_size=full,
                                                                               num_samples=args.draws), reps, wu),
                 draws=args.draws, **dims)
        else:
            emit("cifar_variances", timed(lambda: predict_lla_variances(state, X, Z, mt, alpha, full_set_size=full), reps, wu), **dims)
            emit("cifar_marginals", timed(lambda: predict_lla_marginals(state, X, Z, mt, alpha, full_set_size=full), reps, wu),
                 batch=64, **dims)
        return

    state = create_state(ResNet50(1000), seed=3, dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    Z = torch.rand(2, 224, 224, 3, generator=g).to(dev)
    X = torch.rand(2, 224, 224, 3, generator=g).to(dev)
    mt = "classifier"
    eng = get_engine(state, X, mt)
    dims = dict(D=eng.D, B=eng.n, K=eng.K, probe_chunk=eng.chunk, rows_route_bytes=4 * eng.K * eng.n * eng.D)
    emit("r50_predict_diag", timed(lambda: predict_lla_diag(state, X, Z, mt, alpha), reps, wu), **dims)
    w = posterior_lla_diag(state, Z, mt, alpha).variance()
    E = onehots(eng)
    emit("r50_wnorm_sweep", timed(lambda: eng.vjp_wnorm(E, w, "raw"), reps, wu), **dims)
    emit("r50_diag_sampled", timed(lambda: predict_lla_diag_scalable(state, X, Z, mt, alpha, key=1, num_samples=args.draws),
                                   reps, wu), draws=args.draws, **dims)


if __name__ == "__main__":
    main()
