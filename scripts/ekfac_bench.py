"""Timing of the EKFAC scales pass at the CIFAR config (ResNet1M, D = 1.08 M, n = 50 inducing images, K = 10) next to
the device part of the KFAC fit it comes on top of.

Prints one JSON line per case:
  * kfac_factors     every A_l and S_l: the input Grams and one lip_vjp_kron sweep (LinearizedNet.kfac_factors)
  * factor_rows      the M K factor rows alone: lip_vjp_rows ('l') in the class blocks of the pass
  * scales_pass      LinearizedNet.kfac_eigen_sqsums: those rows and lip_kfac_eigen_sqsum on every layer block
  * trace            max over the blocks of |Lam_l.sum() - sum of compute_ggn_diag over the slice| / that sum
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/ekfac_bench.py [--reps 10] [--warmup 3] [--n 50]
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
from lip_amd.ggn import compute_ggn_diag, get_engine  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402

F64 = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda")
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
    Lams = [torch.zeros(b.Mt, b.N, device=dev, dtype=F64) for b in blocks]
    emit("factor_rows", timed(lambda: [eng._one_hot_rows(k0, k1, "l") for k0, k1 in class_blocks], args.reps, args.warmup), **shape)
    emit("scales_pass", timed(lambda: eng.kfac_eigen_sqsums(bases, Lams), args.reps, args.warmup), **shape)
    for Lam in Lams:
        Lam.zero_()
    eng.kfac_eigen_sqsums(bases, Lams)
    diag = compute_ggn_diag(state, Z, "classifier").double()
    worst = max(abs(float(Lam.sum()) - float(diag[b.off:b.off + b.Mt * b.N].sum())) / float(diag[b.off:b.off + b.Mt * b.N].sum())
                for b, Lam in zip(blocks, Lams))
    emit("trace", (0.0, 0.0, 0.0), rel=worst)


if __name__ == "__main__":
    main()
