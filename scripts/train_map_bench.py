"""Timing of MAP training on the engine (``lip_amd.train_map``) at the reference's CIFAR MAP config: ResNet1M, batch 256, Adam.

Prints one JSON line per case:
  * step             ``MapTrainer.step`` (host clock around the call, which ends in a device-to-host read of the loss)
  * stage/*          the six calls of a step on their own (CUDA events): load, train primal, refresh, loss head, backward, Adam
  * op/*             the per-op-kind times inside the two train tapes (``lip_engine_profile``), with the achieved bytes/s of
                     the statistics and BN-backward ops (4 R N and 12 R N bytes per op) and of the Adam kernel (28 D bytes
                     with a scalar precision: theta, m, v read and written, g read)
  * kernel/*         the statistics, BN-backward and Adam kernels alone on tensors far larger than the 256 MiB Infinity Cache
                     (R = 2^22 rows of 32 channels; D = 2^26): their streaming rate, which the CIFAR config's 8 - 34 MB
                     tensors and ~10 us launches do not show
  * base/engine      one ``lip_engine_primal`` + one ``lip_vjp`` with P = 1 on a 256-example binding: the same convolution
                     work without this module's kernels
  * base/torch       one float32 torch-autograd step of the same network in train mode (``F.conv2d`` / ``F.batch_norm``,
                     ``torch.optim.Adam``): what a user without the engine's train tapes would run
  * epoch            49 000 images in batches of 256 (191 full batches and a tail of 104) from device-resident data, then the
                     test accuracy on a CIFAR-SHAPED SYNTHETIC set (ten fixed random templates plus noise): there is no data
                     set here, so the accuracy of a real run is not measured
Warm-ups first, median of the timed repetitions (min, max).

    python scripts/train_map_bench.py [--reps 10] [--warmup 3] [--batch 256] [--images 49000] [--no-epoch] [--no-torch | --torch-only]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lip_amd  # noqa: E402,F401
from kfac_bench import emit, timed  # noqa: E402
from lip_amd import _native as nv  # noqa: E402
from lip_amd.engine import LinearizedNet  # noqa: E402
from lip_amd.netspec import _get  # noqa: E402
from lip_amd.scalemodels import ResNet1M  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402
from lip_amd.train_map import Adam, MapTrainer  # noqa: E402


def host_timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def torch_step_fn(net, state, x, y, alpha, lr):
    """a float32 autograd step of the layer program in train mode on NCHW tensors"""
    leaves = []

    def leaf(path):
        t = _get(state.params, path).detach().to("cuda", torch.float32).clone().requires_grad_(True)
        leaves.append(t)
        return t

    prog = []
    for u in net.units:
        if u.kind == "conv":
            prog.append((u, leaf(u.kernel), leaf(u.bias) if u.bias is not None else None,
                         leaf(u.bn_scale) if u.bn_scale is not None else None, leaf(u.bn_bias) if u.bn_scale is not None else None,
                         torch.zeros(u.cout, device="cuda"), torch.ones(u.cout, device="cuda")))
        else:
            prog.append((u, None, None, None, None, None, None))
    opt = torch.optim.Adam(leaves, lr=lr)
    xn = x.permute(0, 3, 1, 2).contiguous()

    def step():
        vals = {0: xn}
        for u, W, b, gam, bet, rm, rv in prog:
            a = vals[u.src]
            if u.kind == "meanpool":
                vals[u.dst] = a.mean(dim=(2, 3), keepdim=True)
                continue
            if u.kind == "view":
                vals[u.dst] = a.reshape(a.shape[0], -1, 1, 1)
                continue
            oh, ow, _ = net.tensors[u.dst]
            h, w = a.shape[2], a.shape[3]
            hi_h = max((oh - 1) * u.stride + u.kh - h - u.pad_h, 0)
            hi_w = max((ow - 1) * u.stride + u.kw - w - u.pad_w, 0)
            ap = F.pad(a, (u.pad_w, hi_w, u.pad_h, hi_h)) if (u.pad_h or u.pad_w or hi_h or hi_w) else a
            z = F.conv2d(ap, W.reshape(u.kh, u.kw, u.cin, u.cout).permute(3, 2, 0, 1), b, stride=u.stride)
            if gam is not None:
                z = F.batch_norm(z, rm, rv, gam, bet, training=True, momentum=0.01, eps=u.bn_eps)
            if u.res is not None:
                z = z + vals[u.res]
            vals[u.dst] = torch.relu(z) if u.act == "relu" else z
        logits = vals[net.out].reshape(xn.shape[0], -1)
        loss = F.cross_entropy(logits, y) + 0.5 * alpha * sum((t * t).sum() for t in leaves)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--images", type=int, default=49000)
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="skip base/torch (its first call builds the library's conv kernels)")
    ap.add_argument("--torch-only", action="store_true", help="step and base/torch only")
    args = ap.parse_args()
    dev = torch.device("cuda")
    n, alpha, lr = args.batch, 1e-4, 1e-3
    g = torch.Generator().manual_seed(280300)
    net = ResNet1M(10)
    state = create_state(net, seed=1231231234, dtype=torch.float32, randomize_bn=False)
    # CIFAR-shaped synthetic set: ten fixed random templates plus noise
    templates = torch.randn(10, 32, 32, 3, generator=g)

    def synth(count, seed):
        gg = torch.Generator().manual_seed(seed)
        y = torch.randint(0, 10, (count,), generator=gg)
        return (0.5 * templates[y] + torch.randn(count, 32, 32, 3, generator=gg)).to(dev), y.to(dev)

    x, y = synth(n, 1)
    tr = MapTrainer(state, "classifier", alpha, Adam(lr))
    lib = tr.lib
    D = tr.D

    ms = host_timed(lambda: tr.step(x, y), args.reps, args.warmup)
    emit("step", ms, batch=n, D=D)
    step_ms = ms[0]
    if args.torch_only:
        ms_t = host_timed(torch_step_fn(net, state, x, y, alpha, lr), args.reps, args.warmup)
        emit("base/torch", ms_t, step_over_this=round(step_ms / ms_t[0], 3), torch=torch.__version__)
        return

    b, t = tr._load(x, y)
    st = nv.stream_ptr()
    stages = [
        ("load", lambda: tr._load(x, y)),
        ("train_primal", lambda: nv.check(lib.lip_train_primal(b.h, st), "primal")),
        ("refresh", lambda: nv.check(lib.lip_train_refresh(b.h, st), "refresh")),
        ("loss_head", lambda: tr._loss_head(b, t)),
        ("backward", lambda: nv.check(lib.lip_train_backward(b.h, nv.ptr(b.U), nv.ptr(tr.grad), st), "backward")),
        ("adam", lambda: nv.check(lib.lip_train_adam(nv.ptr(tr.theta), nv.ptr(tr.m), nv.ptr(tr.v), nv.ptr(tr.grad), 0, alpha, lr, 0.9,
                                                     0.999, 1e-8, 10, D, tr._out.data_ptr() + 16, tr._adam_scratch.data_ptr(),
                                                     tr._adam_scratch.numel(), st), "adam")),
    ]
    total = 0.0
    for name, fn in stages:
        ms = timed(fn, args.reps, args.warmup)
        total += ms[0]
        extra = dict(GBps=round(28 * D / ms[0] / 1e6, 1), bytes=28 * D) if name == "adam" else {}
        emit(f"stage/{name}", ms, **extra)
    emit("stage/sum", (total, total, total), step_over_sum=round(step_ms / total, 3))

    # per-op-kind times inside the train tapes
    names = {v: k[3:].lower() for k, v in vars(nv).items() if k.startswith("OP_")}
    nbytes = {nv.OP_BN_STATS: 0, nv.OP_BN_TRAIN_BWD: 0}
    for tape in b.cn.train_tapes:
        for op in tape:
            if op.kind in nbytes:
                nbytes[op.kind] += (4 if op.kind == nv.OP_BN_STATS else 12) * op.n_img * op.OH * op.OW * op.N
    nv.check(lib.lip_engine_profile(b.h, 1), "profile")
    acc = {}
    for _ in range(args.reps):
        nv.check(lib.lip_train_primal(b.h, st), "primal")
        nv.check(lib.lip_train_backward(b.h, nv.ptr(b.U), nv.ptr(tr.grad), st), "backward")
        k_ms, k_cnt = (C.c_double * 16)(), (C.c_int64 * 16)()
        nv.check(lib.lip_engine_profile_read(b.h, k_ms, k_cnt, 16), "profile_read")
        for k in range(16):
            if k_cnt[k]:
                acc.setdefault(k, []).append((k_ms[k], k_cnt[k]))
    nv.check(lib.lip_engine_profile(b.h, 0), "profile")
    for k, rows in sorted(acc.items()):
        v = [r[0] for r in rows]
        extra = dict(bytes=nbytes[k], GBps=round(nbytes[k] / statistics.median(v) / 1e6, 1)) if k in nbytes else {}
        emit(f"op/{names[k]}", (statistics.median(v), min(v), max(v)), launches=rows[0][1], **extra)

    # the three streaming kernels alone, far past the Infinity Cache
    R, N = 1 << 22, 32
    z, xh = torch.randn(R, N, device=dev), torch.randn(R, N, device=dev)
    out = torch.empty_like(z)
    vec = [torch.randn(N, device=dev) for _ in range(8)]
    q = C.c_int64(0)
    nv.check(lib.lip_train_bn_stats_scratch(R, N, C.byref(q)), "scratch")
    scr = torch.empty(q.value, device=dev, dtype=torch.float64)
    ms = timed(lambda: nv.check(lib.lip_train_bn_stats(nv.ptr(z), R, N, 0, nv.ptr(vec[0]), 1e-5, 0.99, nv.ptr(vec[1]), 0, nv.ptr(vec[2]),
                                                       nv.ptr(vec[3]), nv.ptr(vec[4]), nv.ptr(vec[5]), scr.data_ptr(), scr.numel(), st),
                                "bn_stats"), args.reps, args.warmup)
    emit("kernel/bn_stats", ms, R=R, N=N, bytes=4 * R * N, GBps=round(4 * R * N / ms[0] / 1e6, 1))
    ms = timed(lambda: nv.check(lib.lip_train_bn_backward(nv.ptr(z), nv.ptr(xh), nv.ptr(vec[6]), nv.ptr(vec[7]), R, N, nv.ptr(out), st),
                                "bn_backward"), args.reps, args.warmup)
    emit("kernel/bn_train_bwd", ms, R=R, N=N, bytes=12 * R * N, GBps=round(12 * R * N / ms[0] / 1e6, 1))
    del z, xh, out
    Db = 1 << 26
    th, m1, v1, gr = (torch.randn(Db, device=dev) for _ in range(4))
    v1.abs_()
    nv.check(lib.lip_train_adam_scratch(Db, C.byref(q)), "scratch")
    scr = torch.empty(q.value, device=dev, dtype=torch.float64)
    reg = torch.zeros(1, device=dev, dtype=torch.float64)
    ms = timed(lambda: nv.check(lib.lip_train_adam(nv.ptr(th), nv.ptr(m1), nv.ptr(v1), nv.ptr(gr), 0, alpha, lr, 0.9, 0.999, 1e-8, 10, Db,
                                                   reg.data_ptr(), scr.data_ptr(), scr.numel(), st), "adam"), args.reps, args.warmup)
    emit("kernel/adam", ms, D=Db, bytes=28 * Db, GBps=round(28 * Db / ms[0] / 1e6, 1))
    del th, m1, v1, gr

    # the same convolution work on the existing tapes: one primal pass and one P = 1 backward sweep
    eng = LinearizedNet(tr.state(), x, "classifier")
    U = torch.randn(1, n, 10, device=dev)
    ms_p = timed(lambda: nv.check(eng.lib.lip_engine_primal(eng.h, nv.stream_ptr()), "primal"), args.reps, args.warmup)
    ms_v = timed(lambda: eng.vjp(U, "raw"), args.reps, args.warmup)
    emit("base/engine_primal", ms_p)
    emit("base/engine_vjp_p1", ms_v)
    base = ms_p[0] + ms_v[0]
    emit("base/engine", (base, ms_p[1] + ms_v[1], ms_p[2] + ms_v[2]), step_over_this=round(step_ms / base, 3))
    del eng

    if not args.no_torch:
        ms_t = host_timed(torch_step_fn(net, state, x, y, alpha, lr), args.reps, args.warmup)
        emit("base/torch", ms_t, step_over_this=round(step_ms / ms_t[0], 3), torch=torch.__version__)

    if args.no_epoch:
        return
    X, Y = synth(args.images, 2)
    Xt, Yt = synth(1000, 3)
    batches = [(X[i:i + n], Y[i:i + n]) for i in range(0, args.images, n)]
    tr = MapTrainer(state, "classifier", alpha, Adam(lr))
    tr.step(*batches[0])
    tr.step(*batches[-1])                                       # both batch sizes bound and warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for xb, yb in batches:
        loss = tr.step(xb, yb)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    nll, acc1 = tr.evaluate([(Xt[i:i + 250], Yt[i:i + 250]) for i in range(0, 1000, 250)])
    print(__import__("json").dumps(dict(case="epoch", seconds=round(sec, 3), images=args.images, steps=len(batches),
                                        images_per_s=round(args.images / sec, 1), last_train_loss=round(loss, 4),
                                        synthetic_test_nll=round(nll, 4), synthetic_test_acc=round(acc1, 4))), flush=True)


if __name__ == "__main__":
    main()
