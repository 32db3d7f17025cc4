"""One row per code path and edge of the Krylov primitives — TEST INFRASTRUCTURE (a plain helper module).

A ``Case`` names the primitive, its shape dictionary (read by the builders of tests/krylov_harness.py: sizes, the float
offset ``off*`` of each operand base from a 16-byte aligned address, extra row strides ``ld*_extra``), the census label
the call must produce and the path it is there for.  Beside the table: pure-Python mirrors of ``split_row`` /
``row_apply`` and of the launch arithmetic of ``lip_dot_nt_f64``, ``lip_gemm_nt`` and ``lip_rows_combine``, which
tests/test_krylov_ops_cpu.py uses to assert what the table covers.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

KT = 256
# row-streaming kernels: (elements per block that size the grid, block cap) as in the extern "C" wrappers
ROW_LAUNCH = {"bdot": (8192, 256), "axpby": (2048, 2048), "cg_update": (4096, 1024), "cg_direction": (2048, 2048)}

KRYLOV_ROUTES = {"dot_nt/quad/part", "dot_nt/quad/atomic", "dot_nt/tile/part", "dot_nt/tile/atomic", "dot_nt/valu/part",
                 "dot_nt/valu/atomic", "rows_combine<4>", "rows_combine<12>", "gemm_nt/ks1", "gemm_nt/ks", "gemm_nn_axpy",
                 "fill_normal", "fill_rademacher"}
VALU_ONLY = {"dot_nt/valu/part", "dot_nt/valu/atomic"}      # LIP_DOT_NT_VALU, read once per process: tests/test_ab_switches.py


@dataclass
class Case:
    name: str
    prim: str
    d: Dict
    route: Optional[str] = None      # census label of the call (None: the primitive has a single launch site, no label)
    why: str = ""
    exact: bool = True               # run with exact inputs too (every case runs with random inputs)


# ------------------------------------------------------------------------------------------------ mirrors
def split_row(mis, N):
    """(head, quads, tail) of a row that starts ``mis`` floats past a 16-byte boundary"""
    h = min((4 - mis % 4) & 3, N)
    G = (N - h) >> 2
    return h, G, N - h - 4 * G


def row_plan(prim, P, N, off):
    """per row p: (head, quads, tail); and (blocks, trips of the grid-stride loop over the quads)"""
    per, cap = ROW_LAUNCH[prim]
    blocks = max(1, min(cap, (N + per - 1) // per))
    rows = [split_row((off + p * N) % 4, N) for p in range(P)]
    G = max(r[1] for r in rows)
    trips = (G + blocks * KT - 1) // (blocks * KT)
    return rows, blocks, trips, blocks == cap and (N + per - 1) // per > cap


def dot_nt_plan(m, n, K):
    """label of lip_dot_nt_f64 (scratch buffer available), and (tiles_m, tiles_n, K-ranges, kper)"""
    tm, tn = (m + 31) // 32, (n + 31) // 32
    tiles = tm * tn
    chunks = (K + 31) // 32
    ks = min((768 + tiles - 1) // tiles, chunks // 8)
    ks = max(1, min(ks, 65535))
    kper = (chunks + ks - 1) // ks * 32
    ks = (K + kper - 1) // kper
    part = ks > 1 and tiles * ks <= 4096
    if tm >= 2 and tn >= 2 and (not part or tiles * ks * 4 <= 4096) and chunks // (ks * 4) >= 4:
        ks4 = ks * 4
        kper4 = (chunks + ks4 - 1) // ks4 * 32
        ks4 = (K + kper4 - 1) // kper4
        return "dot_nt/quad/" + ("part" if part else "atomic"), (tm, tn, ks4, kper4)
    return "dot_nt/tile/" + ("part" if part else "atomic"), (tm, tn, ks, kper)


def gemm_nt_plan(m, n, K):
    tiles = ((m + 127) // 128) * ((n + 127) // 128)
    ktl = (K + 15) // 16
    ks = max(1, min((1024 + tiles - 1) // tiles, ktl // 64, 65535))
    kper = (ktl + ks - 1) // ks * 16
    ks = (K + kper - 1) // kper
    return ("gemm_nt/ks1" if ks == 1 else "gemm_nt/ks"), (tiles, ks, kper)


def rows_combine_plan(r, s):
    """(label, row tile, blocks along r, bytes of dynamic LDS)"""
    rt = 4 if (r <= 4 or s > 1365) else 12
    return f"rows_combine<{rt}>", rt, (r + rt - 1) // rt, 4 * rt * s


def nn_blocks(m, N):
    return ((m + 127) // 128) * ((N + 127) // 128)


# ------------------------------------------------------------------------------------------------ the table
def _row_cases():
    out = []
    for prim in ROW_LAUNCH:
        # four rows of odd / even length from each base offset: every head x tail; N = 1, 2, 3: no quad at all
        for N in (1, 2, 3, 41, 42, 43, 44):
            for off in range(4):
                out.append(Case(f"{prim}/N{N}/off{off}", prim, dict(P=4, N=N, off=off), why="head x tail, G == 0 for N < 4"))
        out.append(Case(f"{prim}/blocks", prim, dict(P=3, N=3 * ROW_LAUNCH[prim][0] + 5, off=1), why="several blocks, odd N"))
        out.append(Case(f"{prim}/trips", prim, dict(P=2, N=1084586, off=3), why="more than one trip of the grid-stride loop"))
    out.append(Case("bdot/cap", "bdot", dict(P=1, N=256 * 8192 + 4099, off=2), why="block cap of 256"))
    out.append(Case("bdot/same", "bdot", dict(P=3, N=1031, off=1, same=True), why="X and Y the same block (a squared norm)"))
    # axpby: the coefficient forms
    for a in (None, "vec"):
        for b in (None, "vec"):
            out.append(Case(f"axpby/a_{a}/b_{b}", "axpby", dict(P=3, N=1031, off=1, a=a, b=b), why="a / b null or per probe"))
    out.append(Case("axpby/b_s0_nan", "axpby", dict(P=3, N=2051, off=2, a="vec", b="vec", b_s=0.0), why="b_s == 0: Y holds NaN"))
    out.append(Case("axpby/b_s0_bnull_nan", "axpby", dict(P=2, N=45, off=3, a=None, b=None, b_s=0.0), why="b_s == 0, b null"))
    out.append(Case("axpby/bp0_nan_row", "axpby", dict(P=3, N=2051, off=1, a=None, b="vec", zero_b=(1,)),
                    why="b[1] == 0: only row 1 of Y holds NaN"))
    out.append(Case("axpby/same", "axpby", dict(P=3, N=1031, off=3, a="vec", b="vec", same=True), why="X and Y the same buffer"))
    # CG: the active mask
    for prim in ("cg_update", "cg_direction"):
        for tag, act in (("ones", [1, 1, 1, 1]), ("mixed", [1, 0, 0, 1]), ("zero", [0, 0, 0, 0]), ("mixed2", [0, 1, 0, 0])):
            out.append(Case(f"{prim}/active_{tag}", prim, dict(P=4, N=4099, off=1, active=act), why="active mask"))
    return out


def _lanczos_cases():
    out = []
    for prim in ("multi_dot", "multi_axpy_norm"):
        for N in (1, 2, 3, 4, 5, 2047, 2048, 2049, 4095, 4097):
            out.append(Case(f"{prim}/N{N}", prim, dict(P=2, N=N, k=3, off=N % 4, ldq_extra=0 if N % 2 else 8),
                            why="chunk edges, partial last quad over NaN padding"))
        for k in (1, 255, 256, 257, 600):
            out.append(Case(f"{prim}/k{k}", prim, dict(P=3 if k != 600 else 1, N=1030 + k % 4, k=k, kmax=k + 3, off=(k + 1) % 4),
                            why="k around the block size (the j += KT loops), kmax > k"))
        for off in range(4):
            out.append(Case(f"{prim}/off{off}", prim, dict(P=3, N=4097 + off, k=5, off=off, off_c=off), why="w at every offset, P = 3"))
        out.append(Case(f"{prim}/long", prim, dict(P=1, N=50001, k=4, off=3, ldq_extra=8), why="many blocks"))
    for N in (1, 2, 3, 4, 5, 2047, 2048, 2049, 4095, 4097):
        out.append(Case(f"scale_store/N{N}", "scale_store", dict(P=2, N=N, j=1, kmax=3, off=N % 4, ldq_extra=0 if N % 2 else 8),
                        why="chunk edges; padding zeroed up to ldq"))
    out.append(Case("scale_store/j0", "scale_store", dict(P=3, N=1031, j=0, kmax=4, off=1), why="j = 0"))
    out.append(Case("scale_store/jlast", "scale_store", dict(P=3, N=1030, j=3, kmax=4, off=2), why="j = kmax - 1"))
    out.append(Case("scale_store/P1", "scale_store", dict(P=1, N=1029, j=2, kmax=4, off=3), why="P = 1"))
    out.append(Case("scale_store/inf", "scale_store", dict(P=3, N=1031, j=1, kmax=2, off=1, inf_rows=(1,)),
                    why="nrm2 = +inf on one probe (a dead probe of lanczos_tridiag): a row of zeros"))
    out.append(Case("scale_store/long", "scale_store", dict(P=2, N=100003, j=0, kmax=1, off=3),
                    why="several trips of the grid-stride loop"))
    return out


def _dot_nt_cases():
    out = []

    def add(name, m, n, K, why, **kw):
        d = dict(m=m, n=n, K=K, **kw)
        out.append(Case("dot_nt_f64/" + name, "dot_nt_f64", d, route=dot_nt_plan(m, n, K)[0], why=why))
    add("quad_atomic", 900, 900, 600, "quad + atomics, four K-ranges per tile", off_a=1, off_b=2, lda_extra=3, ldb_extra=5)
    add("fallback_tile_part", 850, 850, 2000, "quad refused for scratch size: tile + scratch", off_a=3, off_b=1)
    add("quad_part_odd", 70, 70, 100003, "quad + scratch, 3 x 3 tiles", off_a=1, off_b=3, lda_extra=1, ldb_extra=2)
    add("tile_atomic", 3, 5, 241, "tile + atomics", off_a=2, off_b=1, lda_extra=7)
    add("tile_part", 8, 33, 4099, "tile + scratch", off_a=3, off_b=2, ldb_extra=9)
    add("gram", 65, 65, 4099, "A and B the same matrix (the Gram of gram_orthonormalize)", off_a=1, lda_extra=2, same=True)
    add("long", 33, 31, 1084586, "K = D, kper not dividing K", off_a=1, off_b=3, lda_extra=2, ldb_extra=6)
    add("quad_long", 64, 63, 100003, "quad, 2 x 2 tiles with a partial one", off_a=2, off_b=2, lda_extra=1)
    for K in (1, 15, 16, 17, 31, 32, 33, 511, 512):
        add(f"K{K}", 33, 65, K, "partial first / last 16-chunk", off_a=K % 4, off_b=(K + 1) % 4, lda_extra=K % 3, ldb_extra=4)
    for mn in (1, 31, 32, 63, 64):
        add(f"m{mn}", mn, 65 - mn if mn < 64 else 1, 4099, "tile edges", off_a=1, off_b=2, ldb_extra=1)
    add("small_tiles", 65, 33, 600, "3 x 2 tiles, two K-ranges", off_a=3, off_b=3, lda_extra=2)
    return out


def _gemm_cases():
    out = []

    def nt(name, m, n, K, why, **kw):
        out.append(Case("gemm_nt/" + name, "gemm_nt", dict(m=m, n=n, K=K, **kw), route=gemm_nt_plan(m, n, K)[0], why=why))
    for K in (1, 3, 4, 15, 16, 17, 1023):
        nt(f"K{K}", 5, 7, K, "K around the K-tile", off_a=K % 4, off_b=(K + 2) % 4, lda_extra=1, ldb_extra=2, off_c=K % 4)
    nt("K16383", 127, 129, 1024 * 16 - 1, "K-ranges, partial last tile", off_a=1, off_b=2, lda_extra=3)
    nt("K16385", 128, 1, 1024 * 16 + 1, "K-ranges with a one-element tail", off_a=3, off_b=1, ldb_extra=3)
    nt("long", 129, 1, 1084586, "K = D", off_a=1, off_b=3, lda_extra=2)
    nt("m257", 257, 128, 2051, "three row tiles", off_a=2, off_b=1, ldb_extra=1)
    nt("gram", 127, 127, 4099, "A and B the same matrix", off_a=3, lda_extra=1, same=True)

    def nn(name, m, k, N, why, **kw):
        out.append(Case("gemm_nn_axpy/" + name, "gemm_nn_axpy", dict(m=m, k=k, N=N, **kw), route="gemm_nn_axpy", why=why))
    for i, k in enumerate((4, 5, 6, 7, 15, 16, 17, 33)):
        nn(f"k{k}", (1, 127, 128, 129)[i % 4], k, (4, 5, 127, 128, 129, 1300, 131, 260)[i], "k around the K-tile, tail shift",
           v=(None, "distinct", "out")[i % 3], off_t=i % 4, off_b=(i + 1) % 4, off_o=(i + 2) % 4, off_v=(i + 3) % 4,
           ldt_extra=1 + i % 3, ldb_extra=5, ldo_extra=6, ldv_extra=7)
    nn("k450", 256, 450, 1300, "the sampler's shape, in place", v="out", off_t=1, off_b=2, off_o=3, ldt_extra=1, ldb_extra=3, ldo_extra=2)
    nn("long", 1, 5, 100003, "N long, one row", v="distinct", off_t=3, off_b=1, off_o=2, off_v=1)
    for blocks in (1, 7, 8, 9, 16, 17):
        nn(f"blocks{blocks}", 129 if blocks % 2 == 0 else 3, 6, 128 * (blocks // 2 if blocks % 2 == 0 else blocks) - 3,
           "XCD swizzle g8", v=None if blocks % 2 else "distinct", off_t=2, off_b=3, off_o=1, off_v=2, ldt_extra=2, ldb_extra=1,
           ldo_extra=3, ldv_extra=9)
    return out


def _rows_combine_cases():
    out = []

    def rc(name, r, s, N, why, **kw):
        out.append(Case("rows_combine/" + name, "rows_combine", dict(r=r, s=s, N=N, **kw), route=rows_combine_plan(r, s)[0], why=why))
    for i, (r, s) in enumerate(((1, 7), (4, 30), (5, 30), (12, 7), (13, 30), (25, 9))):
        rc(f"r{r}", r, s, (1023, 1024, 1025, 4099, 5, 3)[i], "row tiles", z=i % 2 == 1, zscale=(0.0, 1.0, -0.5)[i % 3],
           off_y=i % 4, off_o=(i + 1) % 4, off_z=(i + 2) % 4, ldy_extra=1, ldz_extra=2, ldo_extra=3)
    rc("r9_s1366", 9, 1366, 1025, "<4> because s > 1365", z=True, zscale=-0.5, off_y=1, off_o=2, off_z=3, ldy_extra=2, ldo_extra=1)
    rc("lds12", 5, 1365, 1030, "<12> at its LDS limit", off_y=3, off_o=1, ldy_extra=1, ldo_extra=5)
    rc("lds4", 5, 4096, 1027, "<4> at its LDS limit (64 KiB)", z=True, zscale=1.0, off_y=2, off_o=3, off_z=1, ldz_extra=4)
    for N in (1, 2, 3, 4, 5):
        rc(f"N{N}", 6, 5, N, "short rows", z=True, zscale=0.0 if N == 2 else -0.5, off_y=N % 4, off_o=(N + 1) % 4, off_z=(N + 2) % 4,
           ldy_extra=3, ldz_extra=1, ldo_extra=2)
    return out


CASES: List[Case] = _row_cases() + _lanczos_cases() + _dot_nt_cases() + _gemm_cases() + _rows_combine_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ------------------------------------------------------------------------------------------------ refusals
# (name, primitive, shape, what to break): the builders lay the call out, `breakage` then edits the argument list
REFUSALS = [
    ("bdot/mixed_alignment", "bdot", dict(P=2, N=40, off=0, off_y=1), None),
    ("axpby/mixed_alignment", "axpby", dict(P=2, N=40, off=2, off_x=3), None),
    ("cg_update/mixed_alignment", "cg_update", dict(P=2, N=40, off=0), ("shift", 2, 4)),          # p moved by one float
    ("cg_direction/mixed_alignment", "cg_direction", dict(P=2, N=40, off=1), ("shift", 1, 8)),
    ("multi_dot/ldq_mod4", "multi_dot", dict(P=2, N=40, k=2), ("set", 7, 42)),
    ("multi_dot/ldq_lt_N", "multi_dot", dict(P=2, N=40, k=2), ("set", 7, 36)),
    ("multi_dot/unaligned_Q", "multi_dot", dict(P=2, N=40, k=2), ("shift", 0, 4)),
    ("multi_dot/k_gt_kmax", "multi_dot", dict(P=2, N=40, k=2), ("set", 4, 5)),
    ("multi_dot/k_gt_8192", "multi_dot", dict(P=1, N=8, k=2), ("set2", (4, 8193), (5, 8200))),
    ("multi_axpy_norm/ldq_mod4", "multi_axpy_norm", dict(P=2, N=40, k=2), ("set", 8, 42)),
    ("multi_axpy_norm/unaligned_Q", "multi_axpy_norm", dict(P=2, N=40, k=2), ("shift", 0, 8)),
    ("scale_store/ldq_lt_N", "scale_store", dict(P=2, N=40, j=0), ("set", 7, 36)),
    ("scale_store/j_eq_kmax", "scale_store", dict(P=2, N=40, j=0, kmax=2), ("set", 3, 2)),
    ("dot_nt_f64/lda_lt_K", "dot_nt_f64", dict(m=3, n=3, K=40), ("set", 1, 39)),
    ("gemm_nt/ldb_lt_K", "gemm_nt", dict(m=3, n=3, K=40), ("set", 4, 39)),
    ("rows_combine/out_is_Y", "rows_combine", dict(r=3, s=3, N=40), ("copy", 7, 1)),
    ("rows_combine/out_is_Z", "rows_combine", dict(r=3, s=3, N=40, z=True), ("copy", 7, 4)),
    ("rows_combine/s_gt_4096", "rows_combine", dict(r=1, s=3, N=8), ("set", 3, 4097)),
    ("gemm_nn_axpy/k_lt_4", "gemm_nn_axpy", dict(m=3, k=4, N=40), ("set", 3, 3)),
    ("gemm_nn_axpy/out_is_B", "gemm_nn_axpy", dict(m=4, k=4, N=40), ("copy", 10, 4)),
    ("gemm_nn_axpy/V_overlaps_out", "gemm_nn_axpy", dict(m=3, k=4, N=40, v="out"), ("shift", 7, 4)),
    ("bdot/null", "bdot", dict(P=2, N=40), ("set", 1, 0)),
    ("bdot/N0", "bdot", dict(P=2, N=40), ("set", 4, 0)),
    ("axpby/P0", "axpby", dict(P=2, N=40), ("set", 6, 0)),
    ("cg_update/null_rr_new", "cg_update", dict(P=2, N=40), ("set", 7, 0)),
    ("rows_combine/null_Cm", "rows_combine", dict(r=3, s=3, N=40), ("set", 0, 0)),
    ("dot_nt_f64/m0", "dot_nt_f64", dict(m=3, n=3, K=40), ("set", 2, 0)),
    ("gemm_nn_axpy/null_T", "gemm_nn_axpy", dict(m=3, k=4, N=40), ("set", 0, 0)),
    ("fill_normal/null", "fill_normal", None, None),
    ("fill_rademacher/N0", "fill_rademacher", None, None),
]


def break_args(args, how):
    """apply a REFUSALS edit to an argument list: set index, shift a pointer by bytes, copy one argument over another"""
    args = list(args)
    if how is None:
        return args
    if how[0] == "set":
        args[how[1]] = how[2]
    elif how[0] == "set2":
        for i, v in how[1:]:
            args[i] = v
    elif how[0] == "shift":
        args[how[1]] += how[2]
    elif how[0] == "copy":
        args[how[1]] = args[how[2]]
    return args


# fills: total elements, float offset of the base, seed
FILL_TOTALS = [1, 3, 4, 5, 1023, 1024, 1025, 32 * 256 * 4 - 1, 32 * 256 * 4, 32 * 256 * 4 + 1, 3 * 32 * 256 * 4 + 777]
FILL_SEEDS = [0, 1, 2 ** 32, 2 ** 64 - 1]
FILL_CASES = [(t, i % 4, FILL_SEEDS[i % 4]) for i, t in enumerate(FILL_TOTALS)] + \
             [(1025, off, 2 ** 32 + 5) for off in range(4)] + [(4 * 8192 + 2, 0, s) for s in FILL_SEEDS]
# the grid-stride loop of fill_kernel: more than 8192 blocks x 4096 elements (134 MB); the Rademacher kernel would need
# 16384 blocks x 32768 elements (2 GiB) for a second trip and is not taken there
FILL_NORMAL_STRIDE = (8192 * 4096 + 4099, 1, 7)
