"""Timing of the last-layer Laplace fit (compute_ggn_last_layer / lip_ll_ggn) and predictive (lip_ll_predict) at the
CIFAR config (ResNet1M, K = 10), against the route that gave the same matrix before: the materialised factor's
last-layer columns and a float64 Gram.

Prints one JSON line per case:
  * fit50_kernel / fit50_whole       n = 50 inducing points: lip_ll_ggn alone on a bound engine / compute_ggn_last_layer
                                     from a cold engine cache (binding and primal pass included)
  * fit2048_kernel / fit2048_whole   n = 2048, example_chunk = 256: the eight lip_ll_ggn calls alone / the whole call
  * factor50_route                   materialize_factor(eng)[:, sl] and a float64 Gram on a bound engine, n = 50
  * predict256_full / predict256_diag  lip_ll_predict on a bound 256-image test batch
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/last_layer_bench.py [--reps 10] [--warmup 3]
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
from lip_amd.ggn import ExampleChunkedGGN, clear_engine_cache, get_engine, materialize_factor  # noqa: E402
from lip_amd.last_layer import _predict_cov, compute_ggn_last_layer, last_layer_slice  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
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
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = torch.device("cuda")

    net = ResNet1M(10)
    state = create_state(net, seed=1231231234, dtype=torch.float32)
    off, F, K = last_layer_slice(state)
    DL = (F + 1) * K
    shape = dict(F=F, K=K, DL=DL)
    full = 49000
    g = torch.Generator().manual_seed(280300)

    Z = torch.rand(50, 32, 32, 3, generator=g).to(dev)
    eng = get_engine(state, Z, "classifier")
    G = torch.zeros(DL, DL, device=dev, dtype=torch.float64)
    emit("fit50_kernel", timed(lambda: eng.last_layer_ggn(G), reps, args.warmup), n=50, **shape)

    def whole50():
        clear_engine_cache()
        return compute_ggn_last_layer(state, Z, "classifier", full_set_size=full)

    emit("fit50_whole", timed(whole50, reps, args.warmup), n=50, **shape)
    eng = get_engine(state, Z, "classifier")

    def factor_route():
        Wl = materialize_factor(eng)[:, off:off + DL].double()
        return Wl.T @ Wl

    emit("factor50_route", timed(factor_route, reps, args.warmup), n=50, D=eng.D, **shape)
    ref = factor_route()
    new = compute_ggn_last_layer(state, Z, "classifier")
    emit("fit50_agreement", (0.0, 0.0, 0.0), rel=float((new - ref).abs().max() / ref.abs().max()))

    Zb = torch.rand(2048, 32, 32, 3, generator=g).to(dev)
    engines = ExampleChunkedGGN(state, Zb, "classifier", full_set_size=full, example_chunk=256).engines

    def kernels2048():
        for e in engines:
            e.last_layer_ggn(G)

    emit("fit2048_kernel", timed(kernels2048, reps, args.warmup), n=2048, example_chunk=256, **shape)
    del engines
    emit("fit2048_whole", timed(lambda: compute_ggn_last_layer(state, Zb, "classifier", full_set_size=full, example_chunk=256),
                                reps, args.warmup), n=2048, example_chunk=256, **shape)

    X = torch.rand(256, 32, 32, 3, generator=g).to(dev)
    et = get_engine(state, X, "classifier")
    R = torch.randn(DL, DL, device=dev, dtype=torch.float64)
    S = R @ R.T / DL + torch.eye(DL, device=dev, dtype=torch.float64)
    emit("predict256_full", timed(lambda: _predict_cov(et, S, False), reps, args.warmup), B=256, **shape)
    emit("predict256_diag", timed(lambda: _predict_cov(et, S, True), reps, args.warmup), B=256, **shape)


if __name__ == "__main__":
    main()
