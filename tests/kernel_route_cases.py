"""Case table of tests/test_kernel_routes.py: one synthetic op per row, with the launch route it must take.

Shared with the CPU test of the reference (tests/test_kernel_routes_cpu.py), which checks the float64 emulator on the
same geometries.  Expected routes assume the 256 CUs of an MI355X where ``cu`` is set: the few-probe tile rule, split-K
and the probe-batched split depend on the CU count.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

from lip_amd import _native as nv
from op_harness import OpSpec, SegSpec


@dataclass
class Case:
    name: str
    route: str
    spec: OpSpec
    prec: int = 0                     # lip_set_precision
    wino: int = 1                     # lip_set_winograd
    split_k: int = 1                  # lip_set_split_k
    tol: str = "exact"                # "exact" | "wino" | "x3"
    cu: bool = False                  # route depends on the CU count
    det: bool = True                  # no float atomics: a second run is bitwise equal


def _axes(H, W, k, kw, pad, pad_w):
    """the W-axis side, window and padding default to those of the H axis (a window of another width: to its own SAME)"""
    kw = kw or k
    pad = (k - 1) // 2 if pad is None else pad
    if pad_w is None:
        pad_w = pad if kw == k else (kw - 1) // 2
    return W or H, kw, pad, pad_w


def conv(n, H, C, N, P, k=3, s=1, pad=None, W=None, mode=0, OH=None, OW=None, epi=None, nseg=1, kw=None, pad_w=None, **rest):
    """one implicit GEMM over an n x H x W x C map with a k x kw window; mode 1 is the transposed conv onto OH x OW."""
    W, kw, pad, pad_w = _axes(H, W, k, kw, pad, pad_w)
    seg_kw = {x: rest.pop(x) for x in list(rest) if x in SegSpec.__dataclass_fields__}
    if mode == 0:
        OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad_w - kw) // s + 1
    else:
        OH = OH or H * s
        OW = OW or (OH if W == H else W * s)
    segs = [SegSpec(H, W, C, k, kw, s, pad, mode, pad_w=pad_w, **seg_kw) for _ in range(nseg)]
    return OpSpec(nv.OP_IGEMM, segs, n, OH, OW, N, P, epi=dict(epi or {}), **rest)


def wgrad(n, H, C, N, P, k=3, s=1, pad=None, W=None, epi=None, kw=None, pad_w=None, OH=None, OW=None, **rest):
    W, kw, pad, pad_w = _axes(H, W, k, kw, pad, pad_w)
    OH = OH or (H + 2 * pad - k) // s + 1
    OW = OW or (W + 2 * pad_w - kw) // s + 1
    return OpSpec(nv.OP_WGRAD, [SegSpec(H, W, C, k, kw, s, pad, 0, pad_w=pad_w)], n, OH, OW, N, P, epi=dict(epi or {}), **rest)


def dense_wgrad(n, C, N, P, **kw):
    return OpSpec(nv.OP_WGRAD, [SegSpec(1, 1, C, 1, 1, 1, 0, 0)], n, 1, 1, N, P, **kw)


T6 = ("2,2,1,2", "2,2,2,2", "2,2,1,1", "4,1,1,2", "2,1,1,1", "4,1,1,1")
# a geometry per tile of the direct conv kernels (3 x 3, pad 1 over an H x H map; N the 16-byte-aligned column count):
#   N > 64: R <= 64 -> <2,2,1,2>, else <2,2,2,2>; 33..64: <2,2,1,1> / <4,1,1,2>; <= 32: <2,1,1,1> / <4,1,1,1>.
# R > 64 takes the 128-row tiles only with >= 2 * 256 blocks of 128 rows (the few-probe rule): 8 row tiles x 64 probes
IG = {"2,2,1,2": dict(n=1, H=8, N=128, P=3, cu=False), "2,2,2,2": dict(n=1, H=32, N=128, P=64, cu=True),
      "2,2,1,1": dict(n=1, H=8, N=64, P=2, cu=False), "4,1,1,2": dict(n=1, H=32, N=64, P=64, cu=True),
      "2,1,1,1": dict(n=1, H=8, N=32, P=7, cu=False), "4,1,1,1": dict(n=1, H=32, N=32, P=64, cu=True)}


def _igemm_cases() -> List[Case]:
    cs = []
    for t in T6:
        g = IG[t]
        n, H, N, P, cu = g["n"], g["H"], g["N"], g["P"], g["cu"]
        adirect = t.startswith("4,1")
        # plain conv (mode 0), C = 16: the fast kernel (no Winograd: C % 32 != 0); N % 4 decides the dwordx4 B loads
        if not adirect:
            cs.append(Case(f"fast{t}", f"igemm_fast<{t}>", conv(n, H, 16, N - 1, P, a_pp=True), cu=cu))
            cs.append(Case(f"fast{t}_bv4", f"igemm_fast<{t}>/bv4", conv(n, H, 16, N, P, b_pp=True, epi={"scale": "shared"}), cu=cu))
        else:
            cs.append(Case(f"adirect{t}", f"igemm_adirect<{t}>", conv(n, H, 16, N - 1, P, a_pp=True, epi={"e0": "probe"}), cu=cu))
            cs.append(Case(f"adirect{t}_bv4", f"igemm_adirect<{t}>/bv4",
                           conv(n, H, 16, N, P, b_pp=True, epi={"scale": "shared", "e1": "probe", "xhat": "shared", "dphi": "shared"}), cu=cu))
        # stride-2 data gradient (mode 1) onto the even H x H map: parity-class row order
        cs.append(Case(f"fast{t}_par", f"igemm_fast<{t}>/par", conv(n, H // 2, 16, N - 1, P, s=2, mode=1, OH=H, a_pp=True), cu=cu))
        cs.append(Case(f"fast{t}_par_bv4", f"igemm_fast<{t}>/par/bv4",
                       conv(n, H // 2, 16, N, P, s=2, mode=1, OH=H, b_pp=True, epi={"res": "probe", "dphi": "shared"}), cu=cu))
        # split precision (bf16x3)
        cs.append(Case(f"fast{t}_x3", f"igemm_fast<{t}>/x3", conv(n, H, 16, N, P, a_pp=True, epi={"e0": "shared"}), prec=1, tol="x3", cu=cu))
        cs.append(Case(f"fast{t}_x3_par", f"igemm_fast<{t}>/x3/par", conv(n, H // 2, 16, N - 1, P, s=2, mode=1, OH=H, b_pp=True),
                       prec=1, tol="x3", cu=cu))
        # the generic kernel: C % 16 != 0
        cs.append(Case(f"generic{t}", f"igemm<{t}>", conv(n, H, 17, N, P, a_pp=True), cu=cu))
    cs += [
        # ---- sizes and channel counts of the direct kernels
        Case("generic_N1_C1", "igemm<2,1,1,1>", conv(1, 8, 1, 1, 2)),
        Case("generic_N3_C3", "igemm<2,1,1,1>", conv(1, 5, 3, 3, 1, epi={"scale": "shared", "e0": "shared"})),
        Case("fast_N33", "igemm_fast<2,2,1,1>", conv(1, 8, 16, 33, 3, epi={"red0": ""}), det=False),
        Case("fast_N65", "igemm_fast<2,2,1,2>", conv(1, 8, 16, 65, 2, epi={"red1": "", "xhat2": "shared"}), det=False),
        Case("fast_N129", "igemm_fast<2,2,1,2>", conv(1, 8, 16, 129, 2, epi={"e0": "probe", "red0": "", "red1": "", "xhat2": "shared"}), det=False),
        Case("fast_N31_R63", "igemm_fast<2,1,1,1>", conv(1, 9, 32, 31, 2, W=7)),
        Case("generic_C17_N63_R49", "igemm<2,2,1,1>", conv(1, 7, 17, 63, 9, epi={"red0": ""}), det=False),
        Case("fast_C64_N16", "igemm_fast<2,1,1,1>/bv4", conv(1, 4, 64, 16, 8, k=1)),
        # transposed stride 2 onto an ODD map: no parity-class order
        Case("tconv_odd", "igemm_fast<2,2,1,1>/bv4", conv(1, 4, 16, 64, 2, s=2, mode=1, OH=7)),
        Case("tconv_odd_generic", "igemm<2,2,1,1>", conv(1, 4, 17, 48, 2, s=2, mode=1, OH=7)),
        # ---- K cursor of igemm_adirect_kernel (n = 1, 32 x 32 output, P = 64 as IG["4,1,1,1"]; T = K-tiles): the prologue
        # branches T <= 3, the largest T that never enters the 6-way unrolled main loop, two trips of it, the segment
        # switch inside advance() and the stride-2 mask path without the parity order
        Case("adirect_T1", "igemm_adirect<4,1,1,1>/bv4", conv(1, 32, 16, 32, 64, k=1), cu=True),
        Case("adirect_T2", "igemm_adirect<4,1,1,2>", conv(1, 32, 32, 63, 64, k=1, a_pp=True), cu=True),
        Case("adirect_T3", "igemm_adirect<4,1,1,2>/bv4", conv(1, 32, 48, 64, 64, k=1), cu=True),
        Case("adirect_T8", "igemm_adirect<4,1,1,1>/bv4", conv(1, 32, 32, 32, 64, k=2), cu=True),       # 31 x 31 output, R = 961
        Case("adirect_T15", "igemm_adirect<4,1,1,1>/bv4", conv(1, 32, 16, 32, 64, k=3, kw=5), cu=True),
        Case("adirect_nseg2", "igemm_adirect<4,1,1,2>/bv4",
             conv(1, 32, 16, 64, 64, nseg=2, b_pp=True, epi={"e0": "probe", "dphi": "shared"}), cu=True),
        Case("adirect_tconv_odd", "igemm_adirect<4,1,1,1>/bv4", conv(1, 16, 16, 32, 64, s=2, mode=1, OH=31), cu=True),
        # multi-segment and transposed B
        Case("fast_nseg2", "igemm_fast<2,2,1,2>/bv4", conv(1, 8, 16, 96, 2, nseg=2, b_pp=True)),
        Case("fast_nseg3_par", "igemm_fast<2,2,1,1>/par/bv4", conv(1, 4, 16, 64, 2, s=2, mode=1, OH=8, nseg=3)),
        Case("generic_btrans", "igemm<2,2,1,1>", conv(1, 8, 16, 64, 2, b_trans=True, b_pp=True)),
        Case("generic_btrans_nseg2", "igemm<2,1,1,1>", conv(1, 8, 32, 32, 2, nseg=2, b_trans=True)),
        # per-probe A with an odd probe stride (C % 4 != 0)
        Case("generic_a_odd", "igemm<2,1,1,1>", conv(1, 6, 5, 20, 3, a_pp=True, a_odd=True)),
        # every epilogue field in one launch, shared and per-probe addends, other spaces
        Case("fast_all_epi", "igemm_fast<2,2,1,1>/bv4",
             conv(1, 8, 16, 64, 3, epi={"scale": "shared:C", "e0": "probe:H", "e1": "shared", "xhat": "shared",
                                        "res": "probe:H", "dphi": "shared", "red0": "", "red1": "", "xhat2": "shared"}), det=False),
        Case("generic_all_epi", "igemm<2,2,1,2>",
             conv(1, 8, 17, 80, 2, epi={"scale": "shared", "e0": "shared", "e1": "probe", "xhat": "shared",
                                        "res": "probe", "dphi": "shared", "red0": "", "red1": "", "xhat2": "shared"}), det=False),
        # operands in WORK (offsets scaled by the chunk size), output in PRIM (no split-K, no Winograd), CONST epilogue
        Case("work_operands", "igemm_fast<2,1,1,1>/bv4", conv(1, 4, 16, 16, 2, a_pp=True, a_space="W", out_space="W")),
        Case("prim_out_no_ksplit", "igemm_fast<2,2,1,1>/bv4", conv(1, 7, 64, 64, 1, out_space="P", epi={"scale": "shared:C"})),
        Case("prim_out_no_wino", "igemm_fast<2,1,1,1>/bv4", conv(1, 8, 32, 32, 1, out_space="P")),
        # ---- first-layer kernels: C % 16 != 0, Ktot <= 64, N = 32, shared A, P >= 8
        Case("first14_C3_P8", "igemm_first<14>", conv(2, 16, 3, 32, 8, epi={"scale": "shared", "e1": "shared", "xhat": "shared", "dphi": "shared"})),
        Case("first14_C1_P256", "igemm_first<14>", conv(1, 8, 1, 32, 256, epi={"e0": "probe"})),
        Case("first32_C7_P9", "igemm_first<32>", conv(1, 12, 7, 32, 9)),
        Case("first32_C5_P64", "igemm_first<32>", conv(1, 9, 5, 32, 64, epi={"e0": "shared", "dphi": "shared"})),
        Case("first_P7_generic", "igemm<2,1,1,1>", conv(1, 8, 3, 32, 7)),
        # ---- split-K (few probes, long K): 7 x 7 maps (no Winograd), C = 64 -> 36 K-tiles, 3 shares
        Case("ks_2211_bv4", "igemm_fast<2,2,1,1>/ks/bv4", conv(1, 7, 64, 64, 2, epi={"e0": "probe", "dphi": "shared"}), cu=True),
        Case("ks_2211", "igemm_fast<2,2,1,1>/ks", conv(1, 7, 64, 63, 2, epi={"red0": "", "red1": "", "xhat2": "shared"}), cu=True, det=False),
        Case("ks_2111_bv4", "igemm_fast<2,1,1,1>/ks/bv4", conv(1, 7, 64, 32, 1, epi={"scale": "shared", "res": "probe"}), cu=True),
        Case("ks_2111", "igemm_fast<2,1,1,1>/ks", conv(1, 7, 64, 31, 2), cu=True),
        # Ktot just below (23 K-tiles: 1 share) and at (24: 2 shares) the threshold of 12 K-tiles per share
        Case("ks_below", "igemm_fast<2,2,1,1>/bv4", conv(1, 9, 368, 64, 1, k=1), cu=True),
        Case("ks_above", "igemm_fast<2,2,1,1>/ks/bv4", conv(1, 9, 384, 64, 1, k=1), cu=True),
        Case("ks_off", "igemm_fast<2,2,1,1>/bv4", conv(1, 7, 64, 64, 2), split_k=0),
        # ---- Winograd F(2x2, 3x3): C, N multiples of 32, even maps >= 8 x 8
        Case("wino_8x8", "igemm_wino/vepi", conv(1, 8, 32, 32, 2, epi={"scale": "shared", "e0": "probe"})),
        Case("wino_28x28", "igemm_wino/vepi", conv(1, 28, 32, 64, 2, epi={"dphi": "shared", "res": "probe"})),
        Case("wino_24x24_t", "igemm_wino/vepi", conv(2, 24, 64, 32, 1, mode=1, OH=24, s=1, b_pp=True)),
        Case("wino_12x12", "igemm_wino/vepi", conv(3, 12, 32, 32, 3, nseg=2, epi={"red0": "", "red1": "", "xhat2": "shared"}), det=False),
        Case("wino_misaligned_out", "igemm_wino", conv(1, 8, 32, 32, 2, out_shift=1, epi={"e1": "shared", "xhat": "shared"})),
        Case("wino_off", "igemm_fast<2,1,1,1>/bv4", conv(1, 8, 32, 32, 2), wino=0),
        Case("wino_6x6", "igemm_wino/vepi", conv(1, 6, 32, 32, 2, a_pp=True)),
        Case("wino_4x4_ineligible", "igemm_fast<2,1,1,1>/bv4", conv(1, 4, 32, 32, 2)),
    ]
    for c in cs:
        if c.route.startswith("igemm_wino"):
            c.tol = "wino"
    return cs


def _wgrad_cases() -> List[Case]:
    return [
        Case("wg_first", "wgrad_first<32>", wgrad(2, 32, 3, 32, 8), det=False),
        Case("wg_first_C1_P9", "wgrad_first<32>", wgrad(1, 48, 1, 16, 9, epi={"scale": "shared"}), det=False),
        # skinny: one output pixel per example (dense layers), R <= 16 / <= 52 / <= 64
        Case("wg_skinny8", "wgrad_skinny<2,8>", dense_wgrad(16, 40, 45, 3, epi={"scale": "shared"})),
        Case("wg_skinny8_R3", "wgrad_skinny<2,8>", dense_wgrad(3, 130, 1, 2)),
        Case("wg_skinny26", "wgrad_skinny<2,26>", dense_wgrad(52, 130, 33, 2)),
        Case("wg_skinny32", "wgrad_skinny<2,32>", dense_wgrad(64, 64, 64, 2, epi={"scale": "shared"})),
        Case("wg_skinny32_map", "wgrad_skinny<2,32>", OpSpec(nv.OP_WGRAD, [SegSpec(2, 2, 16, 2, 2, 1, 0, 0)], 53, 1, 1, 96, 1)),
        # Winograd weight gradient: one split (no atomics), several splits (atomics)
        Case("wg_wino_rowq", "wgrad_wino/rowq", wgrad(1, 8, 32, 32, 2), tol="wino"),
        Case("wg_wino_24", "wgrad_wino/rowq", wgrad(1, 24, 32, 64, 1, epi={"scale": "shared"}), tol="wino"),
        Case("wg_wino_12", "wgrad_wino", wgrad(2, 12, 32, 32, 2), tol="wino"),
        Case("wg_wino_14", "wgrad_wino", wgrad(1, 28, 32, 32, 2), tol="wino"),
        Case("wg_wino_split", "wgrad_wino/rowq", wgrad(4, 32, 32, 32, 2), tol="wino", det=False),
        # probe-batched tiles (N <= 64, M >= 96; N = 16 keeps the 3 x 3 layers off the Winograd route)
        Case("wg_pb96_288", "wgrad_pb<1,4,3,1>", wgrad(1, 8, 32, 16, 4), det=False),
        Case("wg_pb96_576", "wgrad_pb<1,4,3,1>", wgrad(2, 6, 64, 16, 9, epi={"scale": "shared"}), det=False),
        # N = 64, M = 576 (the 64-channel 3 x 3 layers of the CIFAR net): the only shape that takes the 96-row tile through
        # the clause "M % 96 == 0 && M % 128 != 0" of launch_wgrad (N <= 32 takes the probe-batched branch without it);
        # the 7 x 7 map keeps it off the Winograd route
        Case("wg_pb96_N64_M576", "wgrad_pb<1,4,3,1>", wgrad(1, 7, 64, 64, 4), det=False),
        Case("wg_pb96_x3", "wgrad_pb<3,1,1,4>/x3", wgrad(1, 8, 32, 16, 4), prec=1, tol="x3", det=False),
        Case("wg_pb128", "wgrad_pb<2,2,2,2>", wgrad(1, 8, 16, 32, 4), det=False),
        Case("wg_pb128_P7N12", "wgrad_pb<2,2,2,2>", wgrad(1, 8, 16, 12, 7), det=False),
        Case("wg_pb128_P64", "wgrad_pb<2,2,2,2>", wgrad(2, 8, 16, 20, 64), det=False),
        Case("wg_pb128_x3", "wgrad_pb<2,2,2,2>/x3", wgrad(1, 8, 16, 32, 4), prec=1, tol="x3", det=False),
        # per-probe tiles
        Case("wg_2212_v4", "wgrad_fast<2,2,1,2>/v4", wgrad(1, 8, 4, 128, 2), det=False),
        Case("wg_2212", "wgrad_fast<2,2,1,2>", wgrad(1, 8, 4, 127, 2), det=False),
        Case("wg_2212_generic", "wgrad<2,2,1,2>", wgrad(1, 8, 3, 129, 2), det=False),
        Case("wg_2222_v4", "wgrad_fast<2,2,2,2>/v4", wgrad(1, 8, 16, 128, 2, epi={"scale": "shared"}), det=False),
        Case("wg_2222", "wgrad_fast<2,2,2,2>", wgrad(1, 8, 16, 127, 1), det=False),
        Case("wg_2222_x3", "wgrad_fast<2,2,2,2>/x3", wgrad(1, 8, 16, 128, 2), prec=1, tol="x3", det=False),
        Case("wg_2222_generic", "wgrad<2,2,2,2>", wgrad(1, 8, 17, 65, 2), det=False),
        Case("wg_2211_v4", "wgrad_fast<2,2,1,1>/v4", wgrad(1, 8, 4, 64, 2), det=False),
        Case("wg_2211", "wgrad_fast<2,2,1,1>", wgrad(1, 8, 4, 63, 2), det=False),
        Case("wg_2211_generic", "wgrad<2,2,1,1>", wgrad(1, 8, 3, 33, 2), det=False),
        Case("wg_4112_v4", "wgrad_fast<4,1,1,2>/v4", wgrad(1, 8, 16, 64, 1), det=False),
        Case("wg_4112_v4_ks3", "wgrad_fast<4,1,1,2>/v4", wgrad(1, 8, 16, 64, 1, ksplit=3), det=False),
        Case("wg_4112", "wgrad_fast<4,1,1,2>", wgrad(1, 8, 16, 63, 2), det=False),
        Case("wg_4112_x3", "wgrad_fast<4,1,1,2>/x3", wgrad(1, 8, 16, 64, 1), prec=1, tol="x3", det=False),
        Case("wg_4112_generic", "wgrad<4,1,1,2>", wgrad(1, 8, 17, 64, 2), det=False),
        Case("wg_2111", "wgrad_fast<2,1,1,1>", wgrad(1, 8, 4, 32, 2), det=False),
        Case("wg_2111_x3", "wgrad_fast<2,1,1,1>/x3", wgrad(1, 8, 4, 32, 2), prec=1, tol="x3", det=False),
        Case("wg_2111_generic", "wgrad<2,1,1,1>", wgrad(1, 8, 3, 31, 2), det=False),
        Case("wg_4111", "wgrad_fast<4,1,1,1>", wgrad(1, 8, 16, 32, 1), det=False),
        Case("wg_4111_s2", "wgrad_fast<4,1,1,1>", wgrad(1, 9, 16, 3, 1, s=2, ksplit=2), det=False),
        Case("wg_4111_x3", "wgrad_fast<4,1,1,1>/x3", wgrad(1, 8, 16, 32, 1), prec=1, tol="x3", det=False),
        Case("wg_4111_generic", "wgrad<4,1,1,1>", wgrad(1, 8, 17, 32, 1), det=False),
    ]


# ---------------------------------------------------------------------------------------------- anisotropic cases
# Every case above has a square map, a square window and one padding, so a kernel that reads OW for OH, pad_h for pad_w,
# KW for KH or IW for IH gives the same bits on it as a correct one.  The rows below ("an_...") have IH != IW and
# n_img >= 2 (a wrong per-image stride IH * IW * C shows); tests/test_kernel_routes_cpu.py asserts for each of them that
# exchanging the two axes in the op descriptor changes the float64 result by more than the bound of the route, and that
# every route of the table has at least one such row.
def _an_tile_cases() -> List[Case]:
    """the tile loop of _igemm_cases on 2 images of 4 x 8 / 8 x 4 (R = 64) and 16 x 32 / 32 x 16 (R = 1024)"""
    cs = []
    for i, t in enumerate(T6):
        g = IG[t]
        N, P, cu = g["N"], g["P"], g["cu"]
        H, W = (16, 32) if g["H"] == 32 else (4, 8)
        if i % 2:
            H, W = W, H
        adirect = t.startswith("4,1")
        if not adirect:
            cs.append(Case(f"an_fast{t}", f"igemm_fast<{t}>", conv(2, H, 16, N - 1, P, W=W, a_pp=True), cu=cu))
            cs.append(Case(f"an_fast{t}_bv4", f"igemm_fast<{t}>/bv4", conv(2, W, 16, N, P, W=H, b_pp=True, epi={"scale": "shared"}), cu=cu))
        else:
            cs.append(Case(f"an_adirect{t}", f"igemm_adirect<{t}>", conv(2, H, 16, N - 1, P, W=W, a_pp=True, epi={"e0": "probe"}), cu=cu))
            cs.append(Case(f"an_adirect{t}_bv4", f"igemm_adirect<{t}>/bv4",
                           conv(2, W, 16, N, P, W=H, b_pp=True, epi={"scale": "shared", "e1": "probe", "xhat": "shared", "dphi": "shared"}), cu=cu))
        cs.append(Case(f"an_fast{t}_par", f"igemm_fast<{t}>/par",
                       conv(2, H // 2, 16, N - 1, P, W=W // 2, s=2, mode=1, OH=H, OW=W, a_pp=True), cu=cu))
        cs.append(Case(f"an_fast{t}_par_bv4", f"igemm_fast<{t}>/par/bv4",
                       conv(2, W // 2, 16, N, P, W=H // 2, s=2, mode=1, OH=W, OW=H, b_pp=True, epi={"res": "probe", "dphi": "shared"}), cu=cu))
        cs.append(Case(f"an_fast{t}_x3", f"igemm_fast<{t}>/x3", conv(2, H, 16, N, P, W=W, a_pp=True, epi={"e0": "shared"}),
                       prec=1, tol="x3", cu=cu))
        cs.append(Case(f"an_fast{t}_x3_par", f"igemm_fast<{t}>/x3/par",
                       conv(2, W // 2, 16, N - 1, P, W=H // 2, s=2, mode=1, OH=W, OW=H, b_pp=True), prec=1, tol="x3", cu=cu))
        cs.append(Case(f"an_generic{t}", f"igemm<{t}>", conv(2, H, 17, N, P, W=W, a_pp=True), cu=cu))
    return cs


def _an_igemm_cases() -> List[Case]:
    cs = _an_tile_cases() + [
        # ---- direct kernels: wide and tall maps, KH != KW with the padding to match, 3 x 3 with padding on one axis
        # only, stride 2 on an (even, odd) map (Flax SAME: pad_h = 0, pad_w = 1)
        Case("an_generic_tall_k5x3", "igemm<2,2,1,1>", conv(2, 20, 17, 48, 2, W=6, k=5, kw=3)),
        Case("an_generic_s2_10x7", "igemm<2,1,1,1>", conv(2, 10, 5, 20, 3, W=7, s=2, pad=0, pad_w=1, epi={"scale": "shared", "e0": "shared"})),
        Case("an_fast_wide", "igemm_fast<2,2,1,1>", conv(2, 6, 16, 63, 2, W=20, a_pp=True)),
        Case("an_fast_tall_k1x3_bv4", "igemm_fast<2,2,1,1>/bv4", conv(2, 20, 16, 64, 2, W=6, k=1, kw=3, b_pp=True, epi={"scale": "shared"})),
        Case("an_fast_k3x1", "igemm_fast<2,1,1,1>", conv(3, 5, 32, 31, 2, W=9, k=3, kw=1)),
        Case("an_fast_pad01_bv4", "igemm_fast<2,2,1,2>/bv4", conv(2, 8, 16, 128, 3, W=5, pad=0, pad_w=1)),
        Case("an_fast_pad10", "igemm_fast<2,2,1,2>", conv(2, 5, 16, 127, 3, W=8, pad=1, pad_w=0, epi={"red0": "", "red1": "", "xhat2": "shared"}), det=False),
        Case("an_fast_s2_10x7_bv4", "igemm_fast<2,1,1,1>/bv4", conv(2, 10, 16, 32, 2, W=7, s=2, pad=0, pad_w=1)),
        Case("an_adirect_tall_k2x3_bv4", "igemm_adirect<4,1,1,1>/bv4", conv(2, 32, 16, 32, 64, W=16, k=2, kw=3, b_pp=True), cu=True),
        Case("an_btrans_nseg2", "igemm<2,1,1,1>", conv(2, 4, 32, 32, 2, W=8, nseg=2, b_trans=True)),
        Case("an_fast_nseg3_par", "igemm_fast<2,2,1,1>/par/bv4", conv(2, 2, 16, 64, 2, W=4, s=2, mode=1, OH=4, OW=8, nseg=3)),
        # ---- first-layer kernels
        Case("an_first14_wide", "igemm_first<14>", conv(2, 6, 3, 32, 8, W=20, epi={"scale": "shared", "e1": "shared", "xhat": "shared", "dphi": "shared"})),
        Case("an_first32_tall_k5x3", "igemm_first<32>", conv(2, 20, 3, 32, 9, W=6, k=5, kw=3, epi={"e0": "probe"})),
        Case("an_first32_s2_10x7", "igemm_first<32>", conv(2, 10, 7, 32, 9, W=7, s=2, pad=0, pad_w=1)),
        # ---- split-K: odd sides keep the 3 x 3 layers off the Winograd route; C = 64 -> 36 K-tiles, 3 shares
        Case("an_ks_2211_bv4", "igemm_fast<2,2,1,1>/ks/bv4", conv(2, 5, 64, 64, 2, W=9, epi={"e0": "probe", "dphi": "shared"}), cu=True),
        Case("an_ks_2211", "igemm_fast<2,2,1,1>/ks", conv(2, 9, 64, 63, 2, W=5, pad=1, pad_w=0, epi={"red0": "", "red1": "", "xhat2": "shared"}), cu=True, det=False),
        Case("an_ks_2111_bv4", "igemm_fast<2,1,1,1>/ks/bv4", conv(2, 3, 64, 32, 1, W=7, epi={"scale": "shared", "res": "probe"}), cu=True),
        Case("an_ks_2111", "igemm_fast<2,1,1,1>/ks", conv(2, 7, 64, 31, 2, W=5, pad=0, pad_w=1), cu=True),
        # ---- transposed stride 2: (even, even), (even, odd), (odd, even) outputs and pad_h != pad_w.  Only the
        # (even, even) outputs take the parity-class order
        Case("an_tconv_ee", "igemm_fast<2,2,1,1>/par/bv4", conv(2, 4, 16, 64, 2, W=6, s=2, mode=1, OH=8, OW=12)),
        Case("an_tconv_eo", "igemm_fast<2,2,1,1>", conv(2, 4, 16, 63, 2, W=6, s=2, mode=1, OH=8, OW=11, a_pp=True)),
        Case("an_tconv_oe", "igemm_fast<2,2,1,1>/bv4", conv(2, 4, 16, 64, 2, W=6, s=2, mode=1, OH=7, OW=12, epi={"res": "probe", "dphi": "shared"})),
        Case("an_tconv_oe_generic", "igemm<2,2,1,1>", conv(2, 4, 17, 48, 2, W=6, s=2, mode=1, OH=7, OW=12)),
        Case("an_tconv_par_pad01", "igemm_fast<2,2,1,1>/par", conv(2, 5, 16, 63, 2, W=4, s=2, mode=1, OH=12, OW=8, pad=0, pad_w=1, a_pp=True)),
        Case("an_tconv_eo_pad01", "igemm_fast<2,2,1,1>/bv4", conv(2, 4, 16, 64, 2, W=5, s=2, mode=1, OH=10, OW=9, pad=0, pad_w=1)),
        Case("an_tconv_eo_x3", "igemm_fast<2,2,1,1>/x3", conv(2, 4, 16, 64, 2, W=6, s=2, mode=1, OH=8, OW=11), prec=1, tol="x3"),
        # ---- Winograd F(2x2, 3x3): block rectangles 2^BHs x 2^BWs of 2 x 16 (8 x 24, 6 x 28, 12 x 20), 8 x 4 (24 x 8,
        # 28 x 6, 14 x 6) and 2 x 8 with two images per block (4 x 12: three images, the last block half empty); ragged
        # blocks in H only (24 x 8), in both (6 x 28, 28 x 6)
        Case("an_wino_8x24", "igemm_wino/vepi", conv(2, 8, 32, 32, 2, W=24, epi={"scale": "shared", "e0": "probe"})),
        Case("an_wino_24x8_t", "igemm_wino/vepi", conv(2, 24, 64, 32, 1, W=8, mode=1, OH=24, OW=8, s=1, b_pp=True)),
        Case("an_wino_6x28_nseg2", "igemm_wino/vepi", conv(3, 6, 32, 32, 3, W=28, nseg=2, epi={"red0": "", "red1": "", "xhat2": "shared"}), det=False),
        Case("an_wino_28x6_misaligned_out", "igemm_wino", conv(2, 28, 32, 32, 2, W=6, out_shift=1, epi={"e1": "shared", "xhat": "shared"})),
        Case("an_wino_12x20", "igemm_wino/vepi", conv(2, 12, 32, 64, 2, W=20, epi={"dphi": "shared", "res": "probe"})),
        Case("an_wino_14x6", "igemm_wino/vepi", conv(2, 14, 32, 32, 2, W=6, a_pp=True)),
        Case("an_wino_4x12", "igemm_wino/vepi", conv(3, 4, 32, 32, 2, W=12)),
        Case("an_wino_8x7_ineligible", "igemm_fast<2,1,1,1>/bv4", conv(2, 8, 32, 32, 2, W=7)),
        Case("an_wino_2x28_ineligible", "igemm_fast<2,1,1,1>/bv4", conv(2, 2, 32, 32, 2, W=28)),
    ]
    for c in cs:
        if c.route.startswith("igemm_wino"):
            c.tol = "wino"
    return cs


def _an_clone(c: Case, i: int) -> Case:
    """a weight-gradient case of one 8 x 8 map on two maps of 4 x 8 / 8 x 4: the same R, M and N, so the same route"""
    sg, sp = c.spec.segs[0], c.spec
    H, W = (4, 8) if i % 2 else (8, 4)
    spec = wgrad(2, H, sg.C, sp.N, sp.P, W=W, epi=sp.epi, ksplit=sp.ksplit)
    return Case("an_" + c.name, c.route, spec, prec=c.prec, tol=c.tol, det=c.det)


def _an_wgrad_cases() -> List[Case]:
    base = [c for c in _wgrad_cases() if c.spec.n_img == 1 and c.spec.segs[0].IH == 8 and "wino" not in c.route]
    return [_an_clone(c, i) for i, c in enumerate(base)] + [
        Case("an_wg_first", "wgrad_first<32>", wgrad(2, 24, 3, 32, 8, W=48, pad=0, pad_w=1), det=False),
        # skinny: the flattened non-square map of a dense layer (KH = IH != KW = IW, one output pixel).  Its im2col is
        # the identity, so exchanging the axes cannot change its result (test_kernel_routes_cpu.AXIS_FREE)
        Case("an_wg_skinny8_2x3", "wgrad_skinny<2,8>", OpSpec(nv.OP_WGRAD, [SegSpec(2, 3, 16, 2, 3, 1, 0, 0)], 13, 1, 1, 40, 2)),
        Case("an_wg_skinny26_3x2", "wgrad_skinny<2,26>", OpSpec(nv.OP_WGRAD, [SegSpec(3, 2, 16, 3, 2, 1, 0, 0)], 20, 1, 1, 33, 2, epi={"scale": "shared"})),
        Case("an_wg_skinny32_4x5", "wgrad_skinny<2,32>", OpSpec(nv.OP_WGRAD, [SegSpec(4, 5, 16, 4, 5, 1, 0, 0)], 53, 1, 1, 96, 1)),
        # Winograd weight gradient: /rowq follows TW & 3 alone: 8 x 12 (TH & 3 = 0, TW & 3 = 2) and 24 x 6 without, 12 x 8
        # and 6 x 24 (TH & 3 != 0, TW & 3 = 0) with; 24 x 12 on four images splits (float atomics)
        Case("an_wg_wino_8x12", "wgrad_wino", wgrad(2, 8, 32, 32, 2, W=12), tol="wino"),
        Case("an_wg_wino_12x8", "wgrad_wino/rowq", wgrad(2, 12, 32, 32, 2, W=8), tol="wino"),
        Case("an_wg_wino_24x6", "wgrad_wino", wgrad(2, 24, 32, 64, 2, W=6, epi={"scale": "shared"}), tol="wino"),
        Case("an_wg_wino_6x24", "wgrad_wino/rowq", wgrad(3, 6, 32, 64, 1, W=24), tol="wino"),
        Case("an_wg_wino_split_24x12", "wgrad_wino", wgrad(4, 24, 32, 32, 2, W=12), tol="wino", det=False),
        Case("an_wg_wino_split_16x24", "wgrad_wino/rowq", wgrad(4, 16, 32, 32, 2, W=24), tol="wino", det=False),
        # probe-batched tiles; stride 2 on an (even, odd) map
        Case("an_wg_pb96_pad10", "wgrad_pb<1,4,3,1>", wgrad(2, 6, 32, 16, 4, W=10, pad=1, pad_w=0), det=False),
        Case("an_wg_pb96_k2x3", "wgrad_pb<1,4,3,1>", wgrad(2, 9, 16, 32, 3, W=5, k=2, kw=3), det=False),
        Case("an_wg_pb96_N64_M576", "wgrad_pb<1,4,3,1>", wgrad(2, 5, 64, 64, 4, W=9), det=False),
        Case("an_wg_pb128_s2_10x7", "wgrad_pb<2,2,2,2>", wgrad(2, 10, 16, 32, 4, W=7, s=2, pad=0, pad_w=1), det=False),
        # per-probe tiles: wide and tall maps, anisotropic windows with unequal padding
        Case("an_wg_fast_wide_v4", "wgrad_fast<2,2,1,2>/v4", wgrad(2, 6, 4, 128, 2, W=20), det=False),
        Case("an_wg_fast_tall_k1x3", "wgrad_fast<2,2,1,2>", wgrad(2, 20, 4, 127, 2, W=6, k=1, kw=3), det=False),
        Case("an_wg_fast_k3x1_v4", "wgrad_fast<4,1,1,2>/v4", wgrad(2, 6, 32, 64, 1, W=20, k=3, kw=1), det=False),
        Case("an_wg_generic_k2x3", "wgrad<2,2,1,1>", wgrad(2, 9, 3, 33, 2, W=5, k=2, kw=3), det=False),
        Case("an_wg_generic_k5x3", "wgrad<4,1,1,2>", wgrad(2, 7, 17, 64, 2, W=12, k=5, kw=3), det=False),
        Case("an_wg_4111_s2_10x7", "wgrad_fast<4,1,1,1>", wgrad(2, 10, 16, 3, 1, W=7, s=2, pad=0, pad_w=1, ksplit=2), det=False),
    ]


AN_CASES: List[Case] = _an_igemm_cases() + _an_wgrad_cases()
CASES: List[Case] = _igemm_cases() + _wgrad_cases() + AN_CASES
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
