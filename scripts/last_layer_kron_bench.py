"""Timing of the Kronecker-factored last-layer fit (lip_ll_kron_factors) and predictive (lip_ll_kron_predict) at the
ResNet-50 head, n = 4096 examples, F = 2048, K = 1000, on synthetic float32 features and softmax probabilities, against
the same sums through the library: torch float64 matmuls on up-cast copies.

Prints one JSON line per case:
  * fit_kernel / fit_library          both factors: lip_ll_kron_factors / [1, Phi].double() Gram and
                                      diag(sum p) - p^T p on p.double()
  * fit_eigh                          the host algebra after the factors: the two eigh calls, V and R
  * predict256_diag_kernel / _library B = 256 variances: lip_ll_kron_predict(diag) / ((phit V)^2 R) (Ub o Ub)^T
  * agreement                         max relative difference of the two routes' results
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/last_layer_kron_bench.py [--reps 10] [--warmup 3] [--n 4096] [--F 2048] [--K 1000] [--B 256]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from lip_amd import _native as nv  # noqa: E402
from lip_amd.last_layer_kron import factor_posterior  # noqa: E402

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


def scratch_of(lib, query, n, F, K, dev):
    d = ctypes.c_int64(0)
    nv.check(getattr(lib, query)(n, F, K, ctypes.byref(d)), query)
    return torch.empty(max(1, d.value), device=dev, dtype=F64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--B", type=int, default=256)
    args = ap.parse_args()
    reps, n, F, K, B = max(10, args.reps), args.n, args.F, args.K, args.B
    dev = torch.device("cuda")
    lib = nv.load()
    shape = dict(n=n, F=F, K=K)
    g = torch.Generator().manual_seed(280300)
    Phi = torch.relu(torch.randn(n, F, generator=g)).to(dev)
    Pr = torch.softmax(3.0 * torch.randn(n, K, generator=g), dim=1).to(dev)

    A = torch.zeros(F + 1, F + 1, device=dev, dtype=F64)
    Bf = torch.zeros(K, K, device=dev, dtype=F64)
    fs = scratch_of(lib, "lip_ll_kron_factors_scratch", n, F, K, dev)

    def fit_kernel():                                               # adds into A and Bf: zeroed once before the comparison
        nv.check(lib.lip_ll_kron_factors(Phi.data_ptr(), F, Pr.data_ptr(), n, F, K, A.data_ptr(), Bf.data_ptr(), fs.data_ptr(),
                                         fs.numel(), nv.stream_ptr()), "lip_ll_kron_factors")

    def fit_library():
        pt = torch.cat([torch.ones(n, 1, device=dev, dtype=F64), Phi.double()], dim=1)
        p = Pr.double()
        return pt.T @ pt, torch.diag(p.sum(0)) - p.T @ p

    t_k = timed(fit_kernel, reps, args.warmup)
    t_l = timed(fit_library, reps, args.warmup)
    emit("fit_kernel", t_k, scratch_mb=round(fs.numel() * 8 / 2 ** 20, 1), **shape)
    emit("fit_library", t_l, ratio_kernel_over_library=round(t_k[0] / t_l[0], 2), **shape)
    A.zero_()
    Bf.zero_()
    fit_kernel()
    A_l, B_l = fit_library()
    emit("fit_agreement", (0.0, 0.0, 0.0), rel_A=float((A - A_l).abs().max() / A_l.abs().max()),
         rel_Bf=float((Bf - B_l).abs().max() / B_l.abs().max()))

    a_rows = torch.full((F + 1,), 1e-3 * float(A.diagonal().max()) * float(Bf.diagonal().max()) / n, dtype=F64)
    emit("fit_eigh", timed(lambda: factor_posterior(A, Bf, a_rows, 1.0 / n, True), reps, args.warmup), **shape)
    V, R, Ub, _, _ = factor_posterior(A, Bf, a_rows, 1.0 / n, True)

    X = torch.relu(torch.randn(B, F, generator=g)).to(dev)
    out = torch.empty(B, K, device=dev, dtype=F64)
    ps = scratch_of(lib, "lip_ll_kron_predict_scratch", B, F, K, dev)

    def predict_kernel():
        nv.check(lib.lip_ll_kron_predict(X.data_ptr(), F, B, F, K, V.data_ptr(), R.data_ptr(), Ub.data_ptr(), out.data_ptr(), 1,
                                         ps.data_ptr(), ps.numel(), nv.stream_ptr()), "lip_ll_kron_predict")

    def predict_library():
        pt = torch.cat([torch.ones(B, 1, device=dev, dtype=F64), X.double()], dim=1)
        return ((pt @ V) ** 2 @ R) @ (Ub * Ub).T

    p_k = timed(predict_kernel, reps, args.warmup)
    p_l = timed(predict_library, reps, args.warmup)
    emit("predict256_diag_kernel", p_k, B=B, F=F, K=K)
    emit("predict256_diag_library", p_l, ratio_kernel_over_library=round(p_k[0] / p_l[0], 2), B=B, F=F, K=K)
    ref = predict_library()
    emit("predict_agreement", (0.0, 0.0, 0.0), rel=float((out - ref).abs().max() / ref.abs().max()))


if __name__ == "__main__":
    main()
