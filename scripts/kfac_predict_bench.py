"""Timing of the closed-form KFAC predictive (``predict_lla_kfac(cov="diag")``): the rows route against the backward-sweep
route at the CIFAR config (ResNet1M, D = 1.08 M, n = 50 inducing images, K = 10, B = 256 test points), and the sweep route
alone at ResNet-50 (K = 1000, 224 x 224, two test images, a fit under ``MCFisher(1)``), where the rows route does not exist.

Prints one JSON line per case:
  * predict/cifar/rows        predict_lla_kfac(cov="diag", route="rows"): lip_vjp_rows and lip_kfac_predict per block
  * predict/cifar/sweep       predict_lla_kfac(cov="diag", route="sweep"): lip_vjp_eigen_wnorm, no rows (rows_over_this:
                              the ratio of the medians)
  * sweep_vs_rows             max|var_sweep - var_rows| / max|var_rows|
  * fit/resnet50/mc1          the first call at ResNet-50: the KFAC fit under MCFisher(1) and one predictive (timed once)
  * predict/resnet50/sweep    predict_lla_kfac(cov="diag", route="sweep", curvature=MCFisher(1)) on --r50-b test images
peak_mib: the whole working set of one call, measured apart from the timing: the scratch buffers that the cached engines
hold are dropped, then the peak of torch's allocator over one call is taken above its level before it.  It counts the
route's scratch (which an engine allocates on the first call and keeps: held_mib, the part still held afterwards) and
its transient blocks alike; the fit, the bindings and the probe workspace that both routes share are not counted.
One process, warm bindings and a cached fit, CUDA-event timing on the current stream, warm-ups first, median of the timed
repetitions (min, max).

    python scripts/kfac_predict_bench.py [--reps 5] [--warmup 2] [--n 50] [--B 256] [--r50-n 2] [--r50-b 2] [--r50-res 224]
                                         [--no-cifar] [--no-r50]
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
from lip_amd import ggn as _ggn  # noqa: E402
from lip_amd.fisher import MCFisher  # noqa: E402
from lip_amd.ggn import clear_engine_cache  # noqa: E402
from lip_amd.lla import predict_lla_kfac  # noqa: E402
from lip_amd.scalemodels import ResNet1M, ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402


def timed_with_peak(fn, reps, warmup):
    """(timed(fn), peak MiB of one call from dropped scratch buffers, MiB of scratch the engines hold after it)"""
    ms = timed(fn, reps, warmup)
    for eng in _ggn._ENGINE_CACHE.values():
        eng._scratches.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    held = sum(t.numel() * t.element_size() for eng in _ggn._ENGINE_CACHE.values() for t in eng._scratches.values())
    return ms, round(peak / 2 ** 20, 1), round(held / 2 ** 20, 1)


def cifar(args, dev):
    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    Z = torch.rand(args.n, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    X = torch.rand(args.B, 32, 32, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    alpha = 1.0
    shape = dict(n=args.n, K=10, B=args.B)

    def predict(route):
        return predict_lla_kfac(state, X, Z, "classifier", alpha, cov="diag", batch=args.B, route=route)

    rows, peak_rows, held_rows = timed_with_peak(lambda: predict("rows"), args.reps, args.warmup)
    emit("predict/cifar/rows", rows, peak_mib=peak_rows, held_mib=held_rows, **shape)
    sweep, peak_sweep, held_sweep = timed_with_peak(lambda: predict("sweep"), args.reps, args.warmup)
    emit("predict/cifar/sweep", sweep, peak_mib=peak_sweep, held_mib=held_sweep, rows_over_this=round(rows[0] / sweep[0], 2),
         **shape)
    vr, vs = predict("rows")[1], predict("sweep")[1]
    emit("sweep_vs_rows", (0.0, 0.0, 0.0), rel=float((vs - vr).abs().max() / vr.abs().max()))


def resnet50(args, dev):
    res = args.r50_res
    state = create_state(ResNet50(1000, input_shape=(res, res, 3)), seed=1, dtype=torch.float32)
    Z = torch.rand(args.r50_n, res, res, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    X = torch.rand(args.r50_b, res, res, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    spec = MCFisher(1, 1)
    shape = dict(M=args.r50_n, B=args.r50_b, K=1000, res=res)

    def predict():
        return predict_lla_kfac(state, X, Z, "classifier", 1.0, cov="diag", batch=args.r50_b, curvature=spec, route="sweep")

    emit("fit/resnet50/mc1", timed(predict, 1, 0), **shape)          # the first call fits; the fit is cached from here on
    sweep, peak, held = timed_with_peak(predict, args.reps, args.warmup)
    mean, var = predict()
    emit("predict/resnet50/sweep", sweep, peak_mib=peak, held_mib=held, finite=bool(torch.isfinite(var).all()), var_min=float(var.min()),
         var_max=float(var.max()), **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--r50-n", type=int, default=2)
    ap.add_argument("--r50-b", type=int, default=2)
    ap.add_argument("--r50-res", type=int, default=224)
    ap.add_argument("--no-r50", action="store_true")
    ap.add_argument("--no-cifar", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    if not args.no_cifar:
        cifar(args, dev)
        clear_engine_cache()
        torch.cuda.empty_cache()
    if not args.no_r50:
        resnet50(args, dev)


if __name__ == "__main__":
    main()
