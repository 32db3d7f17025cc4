"""Timing of the EKFAC second moments (``compute_ekfac_scales``): the rows route against the backward-sweep route at the
CIFAR config (ResNet1M, D = 1.08 M, n = 50 inducing images, K = 10), and the sweep route under the Fisher specs at
ResNet-50 (K = 1000), next to the device part of the KFAC fit they come on top of.

Prints one JSON line per case:
  * kfac_factors           every A_l and S_l: the input Grams and one lip_vjp_kron sweep (LinearizedNet.kfac_factors)
  * factor_rows            the M K factor rows alone: lip_vjp_rows ('l') in the class blocks of the pass
  * scales/cifar/rows      compute_ekfac_scales(moments="rows"): those rows and lip_kfac_eigen_sqsum on every layer block
  * scales/cifar/sweep     compute_ekfac_scales(moments="sweep"): lip_vjp_eigen, no rows (rows_over_this: the ratio)
  * sweep_vs_rows          worst block of max|Lam_sweep - Lam_rows| / max|Lam_rows|
  * trace                  max over the blocks of |Lam_l.sum() - sum of compute_ggn_diag over the slice| / that sum (sweep)
  * kfac/resnet50/<spec>   compute_kfac_factors(curvature=spec) at ResNet-50, --r50-n images of --r50-res pixels
  * scales/resnet50/<spec> compute_ekfac_scales(moments="sweep", curvature=spec) there; spec = mc1, mc10, ef.  The bases
                           are dense orthonormal reflectors I - 2 v v^T / v^T v (the time does not depend on their values)
One process, warm bindings, CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions
(min, max).

    python scripts/ekfac_bench.py [--reps 5] [--warmup 2] [--n 50] [--r50-n 8] [--r50-res 224] [--no-r50]
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
from lip_amd import ekfac  # noqa: E402
from lip_amd.fisher import EmpiricalFisher, MCFisher  # noqa: E402
from lip_amd.ggn import clear_engine_cache, compute_ekfac_scales, compute_ggn_diag, compute_kfac_factors, get_engine  # noqa: E402
from lip_amd.scalemodels import ResNet1M, ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402

F64 = torch.float64


def reflector(m, g, dev):
    v = torch.randn(m, generator=g, dtype=F64).to(dev)
    return (torch.eye(m, device=dev, dtype=F64) - (2.0 / float(v @ v)) * torch.outer(v, v)).contiguous()


def cifar(args, dev):
    state = create_state(ResNet1M(10), seed=1231231234, dtype=torch.float32)
    Z = torch.rand(args.n, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    eng = get_engine(state, Z, "classifier")
    blocks = eng.kfac_blocks()
    As = [torch.zeros(b.Mt, b.Mt, device=dev, dtype=F64) for b in blocks]
    Ss = [torch.zeros(b.N, b.N, device=dev, dtype=F64) for b in blocks]
    class_blocks = eng._class_blocks(None)
    shape = dict(D=eng.D, n=args.n, K=eng.K, blocks=len(blocks), class_blocks=len(class_blocks))
    emit("kfac_factors", timed(lambda: eng.kfac_factors(As, Ss), args.reps, args.warmup), **shape)
    for A in As:
        A.zero_()
    for S in Ss:
        S.zero_()
    eng.kfac_factors(As, Ss)
    bases = ekfac.orthonormal_bases(blocks, As, Ss, True)
    emit("factor_rows", timed(lambda: [eng._one_hot_rows(k0, k1, "l") for k0, k1 in class_blocks], args.reps, args.warmup), **shape)
    rows = timed(lambda: compute_ekfac_scales(state, Z, "classifier", bases, moments="rows"), args.reps, args.warmup)
    emit("scales/cifar/rows", rows, **shape)
    sweep = timed(lambda: compute_ekfac_scales(state, Z, "classifier", bases, moments="sweep"), args.reps, args.warmup)
    emit("scales/cifar/sweep", sweep, rows_over_this=round(rows[0] / sweep[0], 2), **shape)
    Lr = compute_ekfac_scales(state, Z, "classifier", bases, moments="rows")
    Ls = compute_ekfac_scales(state, Z, "classifier", bases, moments="sweep")
    emit("sweep_vs_rows", (0.0, 0.0, 0.0), rel=max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(Ls, Lr)))
    diag = compute_ggn_diag(state, Z, "classifier").double()
    worst = max(abs(float(Lam.sum()) - float(diag[b.off:b.off + b.Mt * b.N].sum())) / float(diag[b.off:b.off + b.Mt * b.N].sum())
                for b, Lam in zip(blocks, Ls))
    emit("trace", (0.0, 0.0, 0.0), rel=worst)


def resnet50(args, dev):
    res, n = args.r50_res, args.r50_n
    state = create_state(ResNet50(1000, input_shape=(res, res, 3)), seed=1, dtype=torch.float32)
    Z = torch.rand(n, res, res, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    g = torch.Generator().manual_seed(5)
    specs = [("mc1", MCFisher(1, 1)), ("mc10", MCFisher(10, 1)), ("ef", EmpiricalFisher(torch.randint(0, 1000, (n,), generator=g)))]
    blocks = get_engine(state, Z, "classifier").kfac_blocks()
    bases = [(reflector(b.Mt, g, dev), reflector(b.N, g, dev)) for b in blocks]
    shape = dict(M=n, K=1000, res=res, blocks=len(blocks))
    for name, spec in specs:
        kf = timed(lambda: compute_kfac_factors(state, Z, "classifier", curvature=spec), args.reps, args.warmup)
        emit(f"kfac/resnet50/{name}", kf, **shape)
        sw = timed(lambda: compute_ekfac_scales(state, Z, "classifier", bases, moments="sweep", curvature=spec), args.reps, args.warmup)
        emit(f"scales/resnet50/{name}", sw, over_kfac_factors=round(sw[0] / kf[0], 2), **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--r50-n", type=int, default=8)
    ap.add_argument("--r50-res", type=int, default=224)
    ap.add_argument("--no-r50", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    cifar(args, dev)
    if args.no_r50:
        return
    clear_engine_cache()
    torch.cuda.empty_cache()
    resnet50(args, dev)


if __name__ == "__main__":
    main()
