"""Timing of one subnetwork Laplace fit at the CIFAR config (ResNet1M, n = 50 inducing points, K = 10, S = 4096 indices
chosen by "largest_variance"), split into its stages, against the torch composition that gave the same block before
(index_select, .double(), matmul) on the same rows.

Prints one JSON line per case:
  * select              subnetwork_indices("largest_variance"): one square-accumulating sweep and a sort
  * sweep               eng.vjp_rows of the K one-hot probes, 'l' mode: the (K, n, D) float32 rows both routes read
  * gather              lip_sub_gather: the (K n, S) float32 panel
  * gather_gram         lip_sub_gram on the rows already in memory: gather + Gram tiles + assembly
  * gram                gather_gram - gather (medians)
  * torch_composition   rows.index_select(1, idx).double(), then P^T P added into G
  * agreement           max|G_new - G_torch| and max|G_torch| after one call each, and how many selected columns are nonzero
  * ..._strided         the same five on S evenly strided indices (every column on a cache line of its own)
  * fit_whole           eng.subnetwork_gram: sweep + gather + Gram
  * predict_full_sweep / predict_full   the 'raw' sweep of K probes on the largest test batch whose rows fit one 2 GiB
                        block, and eng.subnetwork_predict (full form) on it, that sweep included
  * predict256_diag     eng.subnetwork_predict (diag form, class blocks) on a bound 256-image test batch, sweeps included
CUDA-event timing on the current stream, warm-ups first, median of the timed repetitions.

    python scripts/subnetwork_bench.py [--reps 10] [--warmup 3] [--size 4096]
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
from lip_amd.ggn import get_engine  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.subnetwork import subnetwork_indices  # noqa: E402
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
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = torch.device("cuda")
    lib = nv.load()

    net = ResNet1M(10)
    state = create_state(net, seed=1231231234, dtype=torch.float32)
    full = 49000
    g = torch.Generator().manual_seed(280300)
    Z = torch.rand(50, 32, 32, 3, generator=g).to(dev)
    eng = get_engine(state, Z, "classifier")
    n, K, D, S = eng.n, eng.K, eng.D, args.size
    shape = dict(n=n, K=K, D=D, S=S)

    def select():
        return subnetwork_indices(state, "largest_variance", S, Z=Z, model_type="classifier", alpha=1.0, full_set_size=full)

    emit("select", timed(select, reps, args.warmup), **shape)
    idx = select().to(dev)

    emit("sweep", timed(lambda: eng._one_hot_rows(0, K, "l"), reps, args.warmup), **shape)
    rows = eng._one_hot_rows(0, K, "l")
    R = K * n
    W = rows.reshape(R, D)

    st = nv.stream_ptr()
    doubles = ctypes.c_int64(0)
    nv.check(lib.lip_sub_gram_scratch(R, S, ctypes.byref(doubles)), "lip_sub_gram_scratch")
    scratch = torch.empty(doubles.value, device=dev, dtype=torch.float64)
    panel = torch.empty(R, S, device=dev, dtype=torch.float32)
    G = torch.zeros(S, S, device=dev, dtype=torch.float64)
    Gt = torch.zeros(S, S, device=dev, dtype=torch.float64)

    # the selected set (where the ranking picks parameters no example reaches, its columns are zero: the arithmetic is
    # the same, but the agreement figure is 0 / 0), and an evenly strided one: every column on another cache line
    strided = (torch.arange(S, device=dev, dtype=torch.int64) * (D // S)).contiguous()
    for tag, ix in (("", idx), ("_strided", strided)):
        def gather():
            nv.check(lib.lip_sub_gather(W.data_ptr(), D, D, R, ix.data_ptr(), S, panel.data_ptr(), st), "lip_sub_gather")

        def gather_gram():
            nv.check(lib.lip_sub_gram(W.data_ptr(), D, D, R, ix.data_ptr(), S, G.data_ptr(), scratch.data_ptr(),
                                      scratch.numel(), st), "lip_sub_gram")

        def torch_route():
            P = W.index_select(1, ix).double()
            Gt.addmm_(P.T, P)

        t_gather = timed(gather, reps, args.warmup)
        emit("gather" + tag, t_gather, **shape)
        t_both = timed(gather_gram, reps, args.warmup)
        emit("gather_gram" + tag, t_both, scratch_mib=round(doubles.value * 8 / 2 ** 20, 1), **shape)
        d = t_both[0] - t_gather[0]
        emit("gram" + tag, (d, d, d), **shape)                       # the difference of the two medians, no spread
        emit("torch_composition" + tag, timed(torch_route, reps, args.warmup), **shape)
        G.zero_()
        Gt.zero_()
        gather_gram()
        torch_route()
        emit("agreement" + tag, (0.0, 0.0, 0.0), max_abs_diff=float((G - Gt).abs().max()), max_abs=float(Gt.abs().max()),
             nonzero_columns=int((panel != 0).any(0).sum()), symmetric=bool(torch.equal(G, G.T)))

    Gw = torch.zeros(S, S, device=dev, dtype=torch.float64)
    emit("fit_whole", timed(lambda: eng.subnetwork_gram(idx, Gw), reps, args.warmup), **shape)
    G.zero_()
    nv.check(lib.lip_sub_gram(W.data_ptr(), D, D, R, idx.data_ptr(), S, G.data_ptr(), scratch.data_ptr(), scratch.numel(), st),
             "lip_sub_gram")
    del rows, W, panel, scratch, Gt, Gw

    # the full form binds no more points than one 2 GiB row block holds (predict_lla_subnetwork sizes its batches so)
    Bf = int(min(256, (eng.ROW_BLOCK_BYTES // (4 * D)) // K))
    X = torch.rand(256, 32, 32, 3, generator=g).to(dev)
    Sigma = torch.linalg.inv(G * (full / n) + torch.eye(S, device=dev, dtype=torch.float64)).contiguous()
    et = get_engine(state, X[:Bf], "classifier")
    emit("predict_full_sweep", timed(lambda: et._one_hot_rows(0, K, "raw"), reps, args.warmup), B=Bf, **shape)
    emit("predict_full", timed(lambda: et.subnetwork_predict(idx, Sigma, False), reps, args.warmup), B=Bf, **shape)
    et = get_engine(state, X, "classifier")
    emit("predict256_diag", timed(lambda: et.subnetwork_predict(idx, Sigma, True), reps, args.warmup), B=256, **shape)


if __name__ == "__main__":
    main()
