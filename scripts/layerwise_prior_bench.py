"""Timing of the layer-wise prior's device work at the CIFAR config (ResNet1M, n = 50, K = 10, P = 256 probes).

Prints one JSON line per case:
  * ggn_vp           lip_ggn_vp with a scalar alpha (the fused prior term)
  * ggn_vp_diag      lip_ggn_vp_diag with the expanded precisions of a "layer" GroupedPrior (the extra streaming pass)
  * grouped_grams    the per-group Grams of the materialised factor (one lip_dot_nt_f64 call per segment)
  * gram_from_factor the single Gram the scalar fit builds, for comparison
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/layerwise_prior_bench.py [--reps 10] [--warmup 3] [--probes 256]
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
from lip_amd.ggn import get_engine, gram_from_factor, grouped_grams, materialize_factor  # noqa: E402
from lip_amd.prior import GroupedPrior  # noqa: E402
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
    ap.add_argument("--probes", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda")

    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    Z = torch.rand(50, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    scale = 49000 / 50
    eng = get_engine(state, Z, "classifier")
    prior = GroupedPrior(state.params, 1.0, "layer")
    values = torch.exp(torch.linspace(-3.0, 3.0, prior.G, dtype=torch.float64))
    a = prior.with_values(values).vector(dev)
    V = torch.randn(args.probes, eng.D, device=dev)
    Y = torch.empty_like(V)
    common = dict(P=args.probes, D=eng.D, groups=prior.G)
    emit("ggn_vp", timed(lambda: eng.ggn_vp(V, scale, 0.5, out=Y), args.reps, args.warmup), **common)
    emit("ggn_vp_diag", timed(lambda: eng.ggn_vp_diag(V, scale, a, out=Y), args.reps, args.warmup), **common)
    del V, Y
    Wm = materialize_factor(eng, 1.0)
    segments = sum(len(prior.segments(g)) for g in range(prior.G))
    emit("grouped_grams", timed(lambda: grouped_grams(Wm, prior), args.reps, args.warmup), d=Wm.shape[0], D=eng.D,
         groups=prior.G, segments=segments)
    emit("gram_from_factor", timed(lambda: gram_from_factor(Wm), args.reps, args.warmup), d=Wm.shape[0], D=eng.D)


if __name__ == "__main__":
    main()
