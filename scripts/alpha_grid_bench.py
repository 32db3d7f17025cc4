"""Timing of the one-pass grid of prior precisions (``predict_lla_kfac_grid``) against the calls it replaces, at the CIFAR
config (ResNet1M, D = 1.08 M, n = 50 inducing images, K = 10, B = 256 test points).

Prints one JSON line per case:
  * fit/cifar                 the KFAC fit alone (factors, eigendecompositions, the remainder's diagonal), the cache dropped
  * predict/cifar/plain       one predict_lla_kfac(cov="diag") call on a cached fit
  * grid/cifar/G              predict_lla_kfac_grid with G = 1, 8, 32 scales on a cached fit (over_plain: the ratio of the
                              medians to the plain call)
  * loop/cifar/8              the path without the grid: 8 predict_lla_kfac(cov="diag") calls at 8 distinct precisions,
                              each of which refits (the fit cache is keyed by the prior); over_grid8: its median over the
                              G = 8 grid call's
  * grid_vs_loop              max|grid slice - looped call| / max|looped call| over the 8 precisions
peak_mib / held_mib: as scripts/kfac_predict_bench.py measures them (the working set of one call above the level before
it, from dropped scratch buffers; the part the engines keep afterwards).  One process, warm bindings, CUDA-event timing on
the current stream, warm-ups first, median of the timed repetitions (min, max).

    python scripts/alpha_grid_bench.py [--reps 10] [--warmup 3] [--n 50] [--B 256]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from kfac_bench import emit  # noqa: E402
from kfac_predict_bench import timed_with_peak  # noqa: E402
from lip_amd import kfac  # noqa: E402
from lip_amd.lla import predict_lla_kfac, predict_lla_kfac_grid  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--B", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda")
    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    Z = torch.rand(args.n, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    X = torch.rand(args.B, 32, 32, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    alpha = 1.0
    shape = dict(n=args.n, K=10, B=args.B)

    def fit():
        kfac._FIT_CACHE.clear()
        return kfac._cached_fit(state, Z, "classifier", alpha, None, None)

    def plain(a=alpha):
        return predict_lla_kfac(state, X, Z, "classifier", a, cov="diag", batch=args.B)

    def grid(scales):
        return predict_lla_kfac_grid(state, X, Z, "classifier", alpha, scales, batch=args.B)

    def scales(G):
        return [10.0 ** (-2.0 + 4.0 * g / max(1, G - 1)) for g in range(G)]

    ms, peak, held = timed_with_peak(fit, args.reps, args.warmup)
    emit("fit/cifar", ms, peak_mib=peak, held_mib=held, **shape)
    one, peak, held = timed_with_peak(plain, args.reps, args.warmup)
    emit("predict/cifar/plain", one, peak_mib=peak, held_mib=held, **shape)
    grid_ms = {}
    for G in (1, 8, 32):
        s = scales(G)
        grid_ms[G], peak, held = timed_with_peak(lambda: grid(s), args.reps, args.warmup)
        emit(f"grid/cifar/{G}", grid_ms[G], peak_mib=peak, held_mib=held, over_plain=round(grid_ms[G][0] / one[0], 3), G=G, **shape)
    s8 = scales(8)
    loop, peak, held = timed_with_peak(lambda: [plain(alpha * s) for s in s8], args.reps, args.warmup)
    emit("loop/cifar/8", loop, peak_mib=peak, held_mib=held, over_grid8=round(loop[0] / grid_ms[8][0], 2), **shape)
    var = grid(s8)[1]
    worst = 0.0
    for g, s in enumerate(s8):
        ref = plain(alpha * s)[1]
        worst = max(worst, float((var[g] - ref).abs().max() / ref.abs().max()))
    emit("grid_vs_loop", (0.0, 0.0, 0.0), rel=worst)


if __name__ == "__main__":
    main()
