"""Timing of the Kronecker-factored posterior over all layers at the CIFAR config (ResNet1M, D = 1.08 M, n = 50 inducing
images, K = 10), against two yardsticks: ``compute_ggn_diag`` at the same binding (one square-sum backward sweep) and the
same input Grams through the library (torch float64 matmuls on unfolded, up-cast copies).

Prints one JSON line per case:
  * fit_input_grams / fit_input_grams_library   every A_l: lip_kfac_input_gram per block / unfold().double() Grams
  * fit_kron_sweep                              every S_l: one lip_vjp_kron sweep of K one-hot probes
  * fit_eigh                                    the host algebra: two eigh calls per block, V and R
  * ggn_diag                                    compute_ggn_diag, the square-sum sweep
  * predict256_diag                             predict_lla_kfac(cov="diag") for B = 256 points (rows + lip_kfac_predict)
  * predict256_rows                             the Jacobian rows of those points alone (lip_vjp_rows)
  * agreement                                   max relative difference of the two routes' input Grams
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/kfac_bench.py [--reps 10] [--warmup 3] [--n 50] [--B 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lip_amd  # noqa: E402,F401
from lip_amd import kfac  # noqa: E402
from lip_amd.ggn import compute_ggn_diag, get_engine  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402

F64 = torch.float64


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


def library_grams(eng):
    """every A_l through torch: unfold the cached activation, up-cast, one float64 matmul"""
    tens = eng.cn.net.tensors
    out = []
    for b in eng.kfac_blocks():
        u = b.unit
        ih, iw, c = tens[u.src]
        oh, ow, _ = tens[u.dst]
        a = eng.prim[b.src:b.src + eng.n * ih * iw * c].reshape(eng.n, ih, iw, c).permute(0, 3, 1, 2)
        hi_h = max((oh - 1) * u.stride + u.kh - ih - u.pad_h, 0)
        hi_w = max((ow - 1) * u.stride + u.kw - iw - u.pad_w, 0)
        cols = F.unfold(F.pad(a, (u.pad_w, hi_w, u.pad_h, hi_h)), (u.kh, u.kw), stride=u.stride)      # (n, c kh kw, T)
        P = cols.reshape(eng.n, c, u.kh * u.kw, -1).permute(0, 3, 2, 1).reshape(-1, u.kh * u.kw * c).double()
        if b.bias:
            P = torch.cat([torch.ones(P.shape[0], 1, device=P.device, dtype=F64), P], dim=1)
        out.append(P.T @ P)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--B", type=int, default=256)
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = torch.device("cuda")
    net = ResNet1M(10)
    state = create_state(net, seed=1231231234, dtype=torch.float32)
    Z = torch.rand(args.n, 32, 32, 3, generator=torch.Generator().manual_seed(280300)).to(dev)
    full, alpha = 49000, 0.005
    eng = get_engine(state, Z, "classifier")
    blocks = eng.kfac_blocks()
    As = [torch.zeros(b.Mt, b.Mt, device=dev, dtype=F64) for b in blocks]
    Ss = [torch.zeros(b.N, b.N, device=dev, dtype=F64) for b in blocks]
    shape = dict(D=eng.D, n=args.n, K=eng.K, blocks=len(blocks))

    t_a = timed(lambda: eng.kfac_input_grams(As), reps, args.warmup)
    t_l = timed(lambda: library_grams(eng), reps, args.warmup)
    emit("fit_input_grams", t_a, **shape)
    emit("fit_input_grams_library", t_l, ratio_kernel_over_library=round(t_a[0] / t_l[0], 2))
    emit("fit_kron_sweep", timed(lambda: eng.kfac_output_grams(Ss), reps, args.warmup), **shape)
    emit("ggn_diag", timed(lambda: compute_ggn_diag(state, Z, "classifier", full_set_size=full), reps, args.warmup), **shape)
    for A in As:
        A.zero_()
    for S in Ss:
        S.zero_()
    eng.kfac_factors(As, Ss)
    lib = library_grams(eng)
    emit("agreement", (0.0, 0.0, 0.0), rel_A=max(float((A - L).abs().max() / L.abs().max()) for A, L in zip(As, lib)))
    rows = [torch.full((b.Mt,), alpha, dtype=F64) for b in blocks]
    emit("fit_eigh", timed(lambda: kfac.fit_blocks(blocks, As, Ss, rows, full / args.n, args.n, True), reps, args.warmup), **shape)

    X = torch.rand(args.B, 32, 32, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    kfac.predict_lla_kfac(state, X[:2], Z, "classifier", alpha, full_set_size=full, cov="diag")          # the fit, cached
    emit("predict256_diag", timed(lambda: kfac.predict_lla_kfac(state, X, Z, "classifier", alpha, full_set_size=full, cov="diag",
                                                                batch=args.B), reps, args.warmup), B=args.B, **shape)
    ex = get_engine(state, X, "classifier")
    emit("predict256_rows", timed(lambda: ex._one_hot_rows(0, ex.K, "raw"), reps, args.warmup), B=args.B)


if __name__ == "__main__":
    main()
