"""Case table of tests/test_small_ops.py: one synthetic non-GEMM op per row, with the census label of the code path it
must take (csrc/lip_small.hip) and the error bound of every output.

Shared with tests/test_small_ops_cpu.py, which pins the float64 emulator on the same geometries against
torch.nn.functional / autograd.

Bounds are in units of 2^-24 * Mag and count float32 roundings, so they hold for any summation order:
  REDUCE red0 R + 8, red1 R + 9; POOL_FWD HW + 2; POOL_BWD out 4, its sums n HW + 8; window average KH KW + 3; max-pool
  cotangent (windows covering a pixel) + 2, its sums n IH IW + 8; HEAD K + 8; PRIMAL_POST 8 on a (none / relu) and xhat.
Gathers (max-pool value, argmax and tangent) and the derivative of none / relu are bitwise.  tanh, GELU and softmax
take the measured constants of test_small_ops.py ("tanh", "gelu", "softmax" below).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from lip_amd import _native as nv
from small_op_harness import FLT_MIN, RefSpec, SmallSpec

F64 = torch.float64
ROWS_ROUTES = {"reduce/rows"}          # the per-example form of reduce_kernel: lip_vjp_rows only (test_rows_and_sqsum)


@dataclass
class Case:
    name: str
    route: str
    spec: SmallSpec
    tol: Dict[str, Tuple]                              # output -> (k, kref) | "exact" | "tanh" | "gelu" | "softmax"
    det: bool = True                                   # no float atomics into an output: a second run is bitwise equal
    relu_skip: bool = False                            # ReLU: dphi is not compared where |y| is below its own rounding
    extra: Optional[str] = None                        # a further assertion of test_small_ops.py, by name
    refuse: bool = False                               # the engine must return LIP_ERR_ARG and write nothing


# ------------------------------------------------------------------------------------------------ REDUCE
def reduce(name, route, N, R, P, red0=True, red1=False, shift=0, odd=False, xshift=0, xspace="V"):
    refs = {"a": RefSpec(R * N, pp=True, shift=shift, odd=odd)}
    tol = {}
    if red1:
        refs["xhat2"] = RefSpec(R * N, space=xspace, shift=xshift)
        refs["red1"] = RefSpec(N, pp=True, space="Y", role="acc")
        tol["red1"] = (R + 9, R)
    if red0:
        refs["red0"] = RefSpec(N, pp=True, space="Y", role="acc")
        tol["red0"] = (R + 8, R)
    return Case(name, route, SmallSpec(nv.OP_REDUCE, P, 1, R, 1, N, refs), tol, det=False)


def _reduce_cases():
    cs = [
        reduce("red_N1", "reduce/fixed", 1, 100, 3),
        reduce("red_N2_R15", "reduce/fixed", 2, 15, 1, red1=True),
        reduce("red_N3_R16", "reduce/atomic", 3, 16, 3, red0=False, red1=True),
        reduce("red_N10_R129", "reduce/atomic", 10, 129, 3, red1=True),
        reduce("red_N40_R100", "reduce/quad", 40, 100, 3, red1=True),                 # 10 quads: 25 row groups, 6 idle threads
        reduce("red_N64_R1", "reduce/quad", 64, 1, 1, red1=True),
        reduce("red_N64_R4097", "reduce/quad", 64, 4097, 1, red1=True),               # rpb 16, 257 row blocks, the last of one row
        reduce("red_N12_R4097_P64_rpb128", "reduce/quad", 12, 4097, 64, red1=True),   # 33 x 64 blocks of 128 rows, ragged
        reduce("red_N4_R2049_P64_rpb64", "reduce/quad", 4, 2049, 64),                 # 33 x 64 blocks of 64 rows
        reduce("red_N4_R1025_P64_rpb32", "reduce/quad", 4, 1025, 64, red0=False, red1=True),
        reduce("red_N256_R129", "reduce/quad", 256, 129, 3, red0=False, red1=True),
        reduce("red_N1000_R16", "reduce/quad", 1000, 16, 3, red1=True),               # 250 quads: one row group
        reduce("red_N1024_R15", "reduce/quad", 1024, 15, 1),                          # 256 quads
        reduce("red_N1028_R100", "reduce/quad_wide", 1028, 100, 3, red1=True),        # 257 quads: thread 0 takes two
        reduce("red_N2048_R129", "reduce/quad_wide", 2048, 129, 1, red1=True),
        reduce("red_N8192_R16", "reduce/quad_wide", 8192, 16, 3, red1=True),          # 2 N floats = the 64 KB of LDS
        # N % 4 == 0 but not 16-byte aligned: the fall-backs
        reduce("red_N64_gshift", "reduce/fixed", 64, 100, 3, red1=True, shift=1),
        reduce("red_N256_xshift", "reduce/fixed", 256, 15, 1, red1=True, xshift=1),
        reduce("red_N40_gshift", "reduce/atomic", 40, 100, 3, red1=True, shift=1),
        reduce("red_N1028_gshift", "reduce/atomic", 1028, 16, 1, shift=3),
        reduce("red_N64_odd", "reduce/mixed", 64, 100, 3, red1=True, odd=True),       # probe 0 quads, probes 1, 2 fixed channel
        reduce("red_N40_xhat_prim", "reduce/quad", 40, 16, 3, red1=True, xspace="P"),
    ]
    c = reduce("red_N8193_refused", "", 8193, 2, 1)
    c.refuse = True
    return cs + [c]


# ------------------------------------------------------------------------------------------------ POOL_FWD / POOL_BWD
def pool_fwd(name, route, C, HW, P, n=2, shift=0, odd=False):
    refs = {"a": RefSpec(n * HW * C, pp=True, shift=shift, odd=odd), "out": RefSpec(n * C, pp=True, space="Y", role="out")}
    spec = SmallSpec(nv.OP_POOL_FWD, P, n, HW, 1, C, refs, fscale=float(torch.tensor(1.0 / HW, dtype=torch.float32)))
    return Case(name, route, spec, {"out": (HW + 2, HW)})


def _relu_mask(count):
    return lambda g: (torch.randn(1, count, generator=g, dtype=F64) > 0).to(F64)


def pool_bwd(name, route, C, HW, P, n=2, dphi=False, red0=False, red1=False, shift=0, odd=False, dshift=0, dspace="V", mask=False):
    cnt = n * HW * C
    refs = {"a": RefSpec(n * C, pp=True), "out": RefSpec(cnt, pp=True, space="Y", role="out", shift=shift, odd=odd)}
    tol = {"out": (4, 1)}
    if dphi:
        refs["dphi"] = RefSpec(cnt, space=dspace, shift=dshift, data=_relu_mask(cnt) if mask else None)
    if red1:
        refs["xhat2"] = RefSpec(cnt)
        refs["red1"] = RefSpec(C, pp=True, space="Y", role="acc")
        tol["red1"] = (n * HW + 8, n * HW)
    if red0:
        refs["red0"] = RefSpec(C, pp=True, space="Y", role="acc")
        tol["red0"] = (n * HW + 8, n * HW)
    spec = SmallSpec(nv.OP_POOL_BWD, P, n, HW, 1, C, refs, fscale=float(torch.tensor(1.0 / HW, dtype=torch.float32)))
    return Case(name, route, spec, tol, det=not (red0 or red1))


def _pool_cases():
    return [
        pool_fwd("pf_C1_HW49", "pool_fwd/fixed", 1, 49, 3),
        pool_fwd("pf_C3_HW15", "pool_fwd/atomic", 3, 15, 1),
        pool_fwd("pf_C10_HW17", "pool_fwd/atomic", 10, 17, 3),
        pool_fwd("pf_C12_HW16", "pool_fwd/quad", 12, 16, 3),
        pool_fwd("pf_C64_HW64", "pool_fwd/fixed", 64, 64, 3),
        pool_fwd("pf_C64_HW64_shift", "pool_fwd/fixed", 64, 64, 1, shift=1),
        pool_fwd("pf_C256_HW1", "pool_fwd/fixed", 256, 1, 3),
        pool_fwd("pf_C512_HW49", "pool_fwd/quad", 512, 49, 3),
        pool_fwd("pf_C1028_HW17", "pool_fwd/quad", 1028, 17, 1),                       # 257 quads: thread 0 takes two
        pool_fwd("pf_C2048_HW49", "pool_fwd/quad", 2048, 49, 3),
        pool_fwd("pf_C12_shift", "pool_fwd/atomic", 12, 16, 3, shift=1),
        pool_fwd("pf_C512_shift", "pool_fwd/atomic", 512, 15, 1, shift=2),
        pool_fwd("pf_C512_odd", "pool_fwd/mixed", 512, 16, 3, odd=True),
        pool_bwd("pb_C1_HW16", "pool_bwd/fixed", 1, 16, 3, red0=True),
        pool_bwd("pb_C3_HW15", "pool_bwd/atomic", 3, 15, 1, red0=True),
        pool_bwd("pb_C10_HW17", "pool_bwd/atomic", 10, 17, 3, dphi=True, red0=True, red1=True),
        pool_bwd("pb_C12_HW16_plain", "pool_bwd/quad", 12, 16, 3),
        pool_bwd("pb_C12_HW49", "pool_bwd/quad", 12, 49, 3, dphi=True, red0=True, red1=True, mask=True),
        pool_bwd("pb_C64_HW64", "pool_bwd/fixed", 64, 64, 3, dphi=True, red0=True, red1=True),
        pool_bwd("pb_C64_HW17_plain", "pool_bwd/fixed", 64, 17, 1, shift=1),
        pool_bwd("pb_C256_HW1", "pool_bwd/fixed", 256, 1, 3, red0=True),
        pool_bwd("pb_C512_HW49", "pool_bwd/quad", 512, 49, 3, dphi=True, red1=True),
        pool_bwd("pb_C1028_HW17", "pool_bwd/quad", 1028, 17, 1, red0=True, red1=True),  # 257 quads: two trips
        pool_bwd("pb_C2048_HW49", "pool_bwd/quad", 2048, 49, 3, dphi=True, red0=True, red1=True, mask=True),
        pool_bwd("pb_C12_outshift", "pool_bwd/atomic", 12, 15, 3, dphi=True, red0=True, red1=True, shift=1),
        pool_bwd("pb_C512_dshift", "pool_bwd/atomic", 512, 16, 1, dphi=True, red0=True, dshift=1),
        pool_bwd("pb_C512_odd", "pool_bwd/mixed", 512, 17, 3, dphi=True, red0=True, red1=True, odd=True),
        pool_bwd("pb_C12_dphi_prim", "pool_bwd/quad", 12, 15, 3, n=1, dphi=True, red0=True, dspace="P"),
    ]


# ------------------------------------------------------------------------------------------------ window pools
def out_size(I, k, s, pad):
    return (I + 2 * pad - k) // s + 1


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def first_argmax(x, k, s, pad):
    """max over KH x KW windows of x (n, IH, IW, C) and the linear pixel index ih * IW + iw of the FIRST maximum in
    (kh, kw) order — the rule the engine documents; written without the emulator's loops over output pixels.
    k and pad: one number for both axes or an (H axis, W axis) pair."""
    n, IH, IW, C = x.shape
    (KH, KW), (ph, pw) = _pair(k), _pair(pad)
    OH, OW = out_size(IH, KH, s, ph), out_size(IW, KW, s, pw)
    xp = torch.full((n, IH + 2 * ph + KH + s, IW + 2 * pw + KW + s, C), -math.inf, dtype=x.dtype)
    xp[:, ph:ph + IH, pw:pw + IW] = x
    pix = torch.full((IH + 2 * ph + KH + s, IW + 2 * pw + KW + s), -1.0, dtype=F64)
    pix[ph:ph + IH, pw:pw + IW] = (torch.arange(IH)[:, None] * IW + torch.arange(IW)[None, :]).to(F64)
    best = torch.full((n, OH, OW, C), -math.inf, dtype=x.dtype)
    arg = torch.full((n, OH, OW, C), -1.0, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            v = xp[:, kh:kh + s * OH:s, kw:kw + s * OW:s]
            q = pix[kh:kh + s * OH:s, kw:kw + s * OW:s][None, :, :, None].expand_as(v)
            better = v > best
            best = torch.where(better, v, best)
            arg = torch.where(better, q, arg)
    return best, arg


MAPS = {"randn": lambda x: x, "relu": lambda x: x.clamp_min(0), "const": lambda x: torch.full_like(x, 0.75)}


def _map(kind, n, IH, IW, C):
    return lambda g: MAPS[kind](torch.randn(n, IH, IW, C, generator=g, dtype=F64)).float().double().reshape(1, -1)


def _argmax_of(kind, n, IH, IW, C, k, s, pad):
    """argmax of a map drawn from a generator of its own (the probes' tangents are independent of it).  f.swapped is
    the argmax the SAME buffer gives when its two axes are exchanged (IW x IH pixels, KW x KH window, pad_w / pad_h):
    what a primal pass with the axes mixed up would have cached (tests/test_small_ops_cpu.py: swap sensitivity)."""
    def x():
        return MAPS[kind](torch.randn(n, IH, IW, C, generator=torch.Generator().manual_seed(1234), dtype=F64)).float().double()

    def f(g):
        return first_argmax(x(), k, s, pad)[1].reshape(1, -1)

    f.swapped = lambda: first_argmax(x().reshape(n, IW, IH, C), _pair(k)[::-1], s, _pair(pad)[::-1])[1].reshape(1, -1)
    return f


def maxpool(name, route, which, C, I, k, s, pad, P=1, n=2, avg=False, kind="randn", odd=False, shift=0, dphi=False,
            red0=False, red1=False, mask=True):
    """I, k, pad: one number for both axes or an (H axis, W axis) pair"""
    (IH, IW), (KH, KW), (ph, pw) = _pair(I), _pair(k), _pair(pad)
    OH, OW = out_size(IH, KH, s, ph), out_size(IW, KW, s, pw)
    cin, cout = n * IH * IW * C, n * OH * OW * C
    tol = {}
    det = True
    kavg = (KH * KW + 3, KH * KW)
    if which == "primal":
        refs = {"a": RefSpec(cin, data=_map(kind, n, IH, IW, C)), "out": RefSpec(cout, space="Y", role="out")}
        if not avg:
            refs["aux0"] = RefSpec(cout, space="Y", role="out")
            tol = {"out": "exact", "aux0": "exact"}
        else:
            tol = {"out": kavg}
        kindop = nv.OP_MAXPOOL_PRIMAL
    elif which == "fwd":
        refs = {"a": RefSpec(cin, pp=True, odd=odd, shift=shift), "out": RefSpec(cout, pp=True, space="Y", role="out")}
        if not avg:
            refs["aux0"] = RefSpec(cout, data=_argmax_of(kind, n, IH, IW, C, k, s, pad))
        tol = {"out": kavg if avg else "exact"}
        kindop = nv.OP_MAXPOOL_FWD
    else:
        refs = {"a": RefSpec(cout, pp=True, odd=odd, shift=shift), "out": RefSpec(cin, pp=True, space="Y", role="out")}
        if not avg:
            refs["aux0"] = RefSpec(cout, data=_argmax_of(kind, n, IH, IW, C, k, s, pad))
        cover = ((KH + s - 1) // s) * ((KW + s - 1) // s)
        tol = {"out": kavg if avg else (cover + 2, 1)}
        if dphi:
            refs["dphi"] = RefSpec(cin, data=_relu_mask(cin) if mask else None)
        if red1:
            refs["xhat2"] = RefSpec(cin)
            refs["red1"] = RefSpec(C, pp=True, space="Y", role="acc")
            tol["red1"] = (n * IH * IW + 8, n * IH * IW)
        if red0:
            refs["red0"] = RefSpec(C, pp=True, space="Y", role="acc")
            tol["red0"] = (n * IH * IW + 8, n * IH * IW)
        det = not (red0 or red1)
        kindop = nv.OP_MAXPOOL_BWD
    spec = SmallSpec(kindop, P, n, OH, OW, C, refs, IH=IH, IW=IW, KH=KH, KW=KW, stride=s, pad=ph, pad_w=pw)
    return Case(name, route, spec, tol, det=det)


W321, W220, W311 = (3, 2, 1), (2, 2, 0), (3, 1, 1)


def _maxpool_cases():
    cs = []
    # ---- primal: every window on odd / even maps, tie maps, the window average
    for C, I, w, kind in ((3, 17, W321, "randn"), (4, 16, W321, "relu"), (10, 16, W220, "relu"), (12, 17, W311, "relu"),
                          (64, 16, W321, "const"), (64, 17, W311, "const"), (1024, 6, W220, "relu"), (2048, 5, W321, "randn")):
        cs.append(maxpool(f"mpp_C{C}_I{I}_w{w[0]}{w[1]}{w[2]}_{kind}", "maxpool_primal/max", "primal", C, I, *w, kind=kind))
    for C, I, w in ((3, 17, W321), (10, 16, W220), (64, 16, W311)):
        cs.append(maxpool(f"mpp_avg_C{C}_I{I}_w{w[0]}{w[1]}{w[2]}", "maxpool_primal/avg", "primal", C, I, *w, avg=True))
    # more than 8192 * 256 outputs: the second trip of the grid-stride loop
    cs.append(maxpool("mpp_C64_I64_n33_trip2", "maxpool_primal/max", "primal", 64, 64, *W321, n=33, kind="relu"))
    # ---- tangent
    for C, I, w, kind, P in ((3, 17, W321, "randn", 3), (4, 16, W321, "relu", 3), (10, 16, W220, "relu", 1),
                             (12, 17, W311, "relu", 3), (64, 16, W321, "const", 3), (1024, 6, W220, "relu", 2),
                             (2048, 5, W321, "randn", 1)):
        cs.append(maxpool(f"mpf_C{C}_I{I}_w{w[0]}{w[1]}{w[2]}_{kind}", "maxpool_fwd/max", "fwd", C, I, *w, P=P, kind=kind))
    cs.append(maxpool("mpf_C64_odd", "maxpool_fwd/max", "fwd", 64, 16, *W321, P=3, kind="relu", odd=True))
    for C, I, w, P in ((3, 17, W321, 3), (10, 16, W220, 1), (64, 16, W311, 3)):
        cs.append(maxpool(f"mpf_avg_C{C}_I{I}_w{w[0]}{w[1]}{w[2]}", "maxpool_fwd/avg", "fwd", C, I, *w, P=P, avg=True))
    # more than 4096 * 256 outputs per probe
    cs.append(maxpool("mpf_C64_I64_n17_trip2", "maxpool_fwd/max", "fwd", 64, 64, *W321, P=2, n=17, kind="relu"))
    # ---- cotangent: quad needs C % 4 == 0 and 256 % (C / 4) == 0 (12: 3 quads; 2048: 512 quads -> scalar)
    B = dict(dphi=True, red0=True, red1=True)
    cs += [
        maxpool("mpb_C3_I17", "maxpool_bwd/scalar", "bwd", 3, 17, *W321, P=3, red0=True),
        maxpool("mpb_C4_I16_relu", "maxpool_bwd/quad", "bwd", 4, 16, *W321, P=3, kind="relu", **B),
        maxpool("mpb_C10_I16_lenet", "maxpool_bwd/scalar", "bwd", 10, 16, *W220, P=1, kind="relu", **B),
        maxpool("mpb_C12_I17_w311", "maxpool_bwd/scalar", "bwd", 12, 17, *W311, P=3, kind="relu", **B),
        maxpool("mpb_C64_I16_const", "maxpool_bwd/quad", "bwd", 64, 16, *W321, P=3, kind="const", **B),
        maxpool("mpb_C64_I17_w311_const", "maxpool_bwd/quad", "bwd", 64, 17, *W311, P=3, kind="const", dphi=True, red1=True, mask=False),
        maxpool("mpb_C64_plain", "maxpool_bwd/quad", "bwd", 64, 16, *W220, P=2, kind="relu"),
        maxpool("mpb_C1024_I6", "maxpool_bwd/quad", "bwd", 1024, 6, *W220, P=2, kind="relu", **B),
        maxpool("mpb_C2048_I5", "maxpool_bwd/scalar", "bwd", 2048, 5, *W321, P=1, **B),
        maxpool("mpb_C64_odd", "maxpool_bwd/scalar", "bwd", 64, 16, *W321, P=3, kind="relu", odd=True, **B),
        maxpool("mpb_C64_shift", "maxpool_bwd/scalar", "bwd", 64, 16, *W321, P=1, kind="relu", shift=1, **B),
        maxpool("mpb_avg_C3_I17", "maxpool_bwd/scalar/avg", "bwd", 3, 17, *W321, P=3, avg=True, **B),
        maxpool("mpb_avg_C10_I16_lenet", "maxpool_bwd/scalar/avg", "bwd", 10, 16, *W220, P=1, avg=True, red0=True),
        maxpool("mpb_avg_C64_I16_w311", "maxpool_bwd/quad/avg", "bwd", 64, 16, *W311, P=3, avg=True, **B),
        maxpool("mpb_avg_C16_I16_lenet", "maxpool_bwd/quad/avg", "bwd", 16, 16, *W220, P=2, avg=True),
        # the second trip: more than 2048 * 256 inputs per probe (scalar); P = 64 and more than 128 * 256 quads per probe
        maxpool("mpb_C12_I33_n41_trip2", "maxpool_bwd/scalar", "bwd", 12, 33, *W321, P=2, n=41, kind="relu", **B),
        maxpool("mpb_C64_I33_P64_trip2", "maxpool_bwd/quad", "bwd", 64, 33, *W321, P=64, n=2, kind="relu", **B),
    ]
    return cs + _an_maxpool_cases()


def _an_maxpool_cases():
    """non-square maps, windows and paddings ("an_..."): 17 x 12 with a 3 x 2 window, padding (1, 0), stride 2 on the
    (odd, even) map; 6 x 16 with a 2 x 3 window, padding (0, 1).  Two images each.  Exchanging the two axes in the op
    descriptor fails the check of every one of them (tests/test_small_ops_cpu.py).  The cached argmax ih * IW + iw of
    the max pools is bitwise: a swapped IH / IW shows there."""
    A, Bm = ((17, 12), (3, 2), 2, (1, 0)), ((6, 16), (2, 3), 1, (0, 1))
    B2 = ((6, 16), (2, 3), 2, (0, 1))
    B = dict(dphi=True, red0=True, red1=True)
    return [
        maxpool("an_mpp_C3_17x12", "maxpool_primal/max", "primal", 3, *A),
        maxpool("an_mpp_C64_6x16_const", "maxpool_primal/max", "primal", 64, *Bm, kind="const"),
        maxpool("an_mpp_avg_C10_6x16_s2", "maxpool_primal/avg", "primal", 10, *B2, avg=True),
        maxpool("an_mpp_avg_C3_17x12", "maxpool_primal/avg", "primal", 3, *A, avg=True),
        maxpool("an_mpf_C4_17x12_relu", "maxpool_fwd/max", "fwd", 4, *A, P=3, kind="relu"),
        maxpool("an_mpf_C64_6x16_const", "maxpool_fwd/max", "fwd", 64, *Bm, P=2, kind="const"),
        maxpool("an_mpf_avg_C3_6x16", "maxpool_fwd/avg", "fwd", 3, *Bm, P=2, avg=True),
        maxpool("an_mpf_avg_C64_17x12", "maxpool_fwd/avg", "fwd", 64, *A, P=3, avg=True),
        maxpool("an_mpb_C3_17x12", "maxpool_bwd/scalar", "bwd", 3, *A, P=3, **B),
        maxpool("an_mpb_C10_6x16_relu", "maxpool_bwd/scalar", "bwd", 10, *Bm, P=2, kind="relu", **B),
        maxpool("an_mpb_C64_17x12_relu", "maxpool_bwd/quad", "bwd", 64, *A, P=3, kind="relu", **B),
        maxpool("an_mpb_C64_6x16_const", "maxpool_bwd/quad", "bwd", 64, *Bm, P=3, kind="const", **B),
        maxpool("an_mpb_avg_C3_17x12", "maxpool_bwd/scalar/avg", "bwd", 3, *A, P=3, avg=True, **B),
        maxpool("an_mpb_avg_C10_6x16_s2", "maxpool_bwd/scalar/avg", "bwd", 10, *B2, P=1, avg=True, red0=True),
        maxpool("an_mpb_avg_C64_6x16", "maxpool_bwd/quad/avg", "bwd", 64, *Bm, P=3, avg=True, **B),
        maxpool("an_mpb_avg_C16_17x12", "maxpool_bwd/quad/avg", "bwd", 16, *A, P=2, avg=True),
    ]


# ------------------------------------------------------------------------------------------------ PRIMAL_POST
ACTS = ("none", "relu", "tanh", "gelu")


def _spread(count):
    """randn scaled so that |y| spans 1e-3 ... 8: tanh saturation, GELU's negative lobe"""
    def f(g):
        e = torch.rand(1, count, generator=g, dtype=F64) * (math.log10(8.0) + 3.0) - 3.0
        return torch.randn(1, count, generator=g, dtype=F64).sign() * 10.0 ** e
    return f


def primal_post(name, act, variant, N, R, out2=True, cspace="V", zero=False):
    cnt = R * N
    z = _spread(cnt)
    if zero:
        z = lambda g: torch.where(torch.rand(1, cnt, generator=g, dtype=F64) > 0.5, torch.randn(1, cnt, generator=g, dtype=F64),
                                  torch.zeros(1, cnt, dtype=F64))
    refs = {"a": RefSpec(cnt, data=z), "out": RefSpec(cnt, space="Y", role="out")}
    t = {0: (8, 1), 1: (8, 1), 2: "tanh", 3: "gelu"}[act]
    tol = {"out": t}
    if out2:
        refs["out2"] = RefSpec(cnt, space="Y", role="out")
        tol["out2"] = "exact" if act < 2 else t
    if variant == "bias":
        refs["e0"] = RefSpec(N, data=0.5)
    if variant in ("bn", "bn_res"):
        refs["e1"] = RefSpec(N)                                            # gamma
        refs["scale"] = RefSpec(N, data=0.5)                               # beta
        refs["aux0"] = RefSpec(N, data=0.5, space=cspace)                  # mean
        refs["aux1"] = RefSpec(N, space=cspace, data=lambda g: 0.5 + 1.5 * torch.rand(1, N, generator=g, dtype=F64))
        refs["out3"] = RefSpec(cnt, space="Y", role="out")
        tol["out3"] = (8, 1)
    if variant == "bn_res":
        refs["res"] = RefSpec(cnt)
    spec = SmallSpec(nv.OP_PRIMAL_POST, 1, 1, R, 1, N, refs, act=act)
    route = f"primal_post/{ACTS[act]}" + ("/bn" if variant in ("bn", "bn_res") else "")
    return Case(name, route, spec, tol, relu_skip=act == 1 and out2 and not zero)


def _primal_post_cases():
    cs = []
    Ns = (1, 3, 64, 1000)
    i = 0
    for act in range(4):
        for variant in ("plain", "bias", "bn", "bn_res"):
            N = Ns[(i + act) % 4]
            cs.append(primal_post(f"pp_{ACTS[act]}_{variant}_N{N}", act, variant, N, 37 if N >= 64 else 1500, out2=i % 5 != 4))
            i += 1
    cs += [
        primal_post("pp_relu_bn_const_stats", 1, "bn", 64, 50, cspace="C"),
        primal_post("pp_gelu_trip2", 3, "bn_res", 64, 16400),              # more than 4096 * 256 elements
        primal_post("pp_relu_trip2", 1, "bias", 64, 16400),
        primal_post("pp_relu_exact_zeros", 1, "plain", 64, 100, zero=True),
    ]
    cs[-1].extra = "relu_zeros"
    return cs


# ------------------------------------------------------------------------------------------------ SOFTMAX / HEAD
KS = (1, 2, 10, 63, 64, 65, 100, 1000)


def softmax(name, K, n, data):
    refs = {"a": RefSpec(n * K, data=data), "out": RefSpec(n * K, space="Y", role="out"), "out2": RefSpec(n * K, space="Y", role="out")}
    c = Case(name, "softmax", SmallSpec(nv.OP_SOFTMAX, 1, n, 1, 1, K, refs), {"out": "softmax", "out2": "softmax"})
    c.extra = "softmax"
    return c


def _shift_rows(K):
    """row 0: multiples of 2^-10 below 8; row 1: the same + 1e4, exactly representable, so both rows have ONE reference"""
    def f(g):
        r = (torch.randn(K, generator=g, dtype=F64).clamp(-7, 7) * 1024).round() / 1024
        return torch.stack([r, r + 1.0e4]).reshape(1, -1)
    return f


def _softmax_cases():
    cs = []
    for i, K in enumerate(KS):
        cs.append(softmax(f"sm_K{K}_x1", K, 5 if i % 2 == 0 else 1, 1.0))
        cs.append(softmax(f"sm_K{K}_x30", K, 1 if i % 2 == 0 else 5, 30.0))
    cs.append(softmax("sm_const_row", 100, 1, lambda g: torch.full((1, 100), 3.25, dtype=F64)))
    for K in (10, 65, 1000):
        c = softmax(f"sm_shift_K{K}", K, 2, _shift_rows(K))
        c.extra = "softmax_shift"
        cs.append(c)
    return cs


def _probs(n, K, root):
    def f(g):
        p = torch.softmax(torch.randn(n, K, generator=torch.Generator().manual_seed(77), dtype=F64) * 2.0, -1)
        return (p.sqrt() if root else p).reshape(1, -1)
    return f


HEAD_MODES = {"ggn": nv.HEAD_GGN, "lt": nv.HEAD_LT, "l": nv.HEAD_L, "out": nv.HEAD_OUT, "in": nv.HEAD_IN}


def head(name, mode, classifier, K, n, P):
    m = HEAD_MODES[mode]
    rin, rout, idle = {"ggn": ("a", "out", "out2"), "lt": ("a", "out2", "out"), "out": ("a", "out2", "out"),
                       "l": ("out2", "out", "a"), "in": ("out2", "out", "a")}[mode]
    refs = {rin: RefSpec(n * K, pp=True, space="H"), rout: RefSpec(n * K, pp=True, space="Y", role="out"),
            idle: RefSpec(n * K, pp=True, space="V", role="idle")}
    if classifier:
        refs["aux0"] = RefSpec(n * K, data=_probs(n, K, False))
        refs["aux1"] = RefSpec(n * K, data=_probs(n, K, True))
    spec = SmallSpec(nv.OP_HEAD, P, n, 1, 1, K, refs, classifier=classifier, head_mode=m, head_c=0.7)
    route = f"head/{mode}" if classifier and mode in ("ggn", "lt", "l") else "head/scale"
    return Case(name, route, spec, {rout: (K + 8, K)})


def _head_cases():
    cs = []
    i = 0
    for mode in HEAD_MODES:
        for classifier in (1, 0):
            for j in range(2 if classifier and mode in ("ggn", "lt", "l") else 1):
                K = KS[i % len(KS)]
                cs.append(head(f"head_{mode}_{'cls' if classifier else 'reg'}_K{K}", mode, classifier, K, 5 if i % 2 else 1, 3 if i % 3 else 1))
                i += 1
    # every K through the three softmax-factor actions
    for K in KS:
        for mode in ("ggn", "lt", "l"):
            nm = f"head_{mode}_cls_K{K}"
            if all(c.name != nm for c in cs):
                cs.append(head(nm, mode, 1, K, 2, 3))
    return cs


CASES: List[Case] = (_reduce_cases() + _pool_cases() + _maxpool_cases() + _primal_post_cases() + _softmax_cases()
                     + _head_cases())
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALL_ROUTES = {c.route for c in CASES if c.route} | ROWS_ROUTES
