"""The kernels behind the A/B environment switches — TEST INFRASTRUCTURE (a plain helper module).

The library reads each ``LIP_...`` switch once per process (``struct Switches`` of csrc/lip_internal.h, filled on the
first call of ``switches()`` in csrc/lip_mfma.hip), so a switch can only be tested in a fresh process: tests/test_ab_switches.py starts
tests/ab_child.py once per entry below, with the entry's environment, and asserts for every row that the census is
exactly the expected route and that the op passes the same float64 check as in tests/test_kernel_routes.py /
tests/test_krylov_ops.py.  tests/test_ab_switches_cpu.py checks the table itself.

An ``Entry`` holds the environment, ``rows`` = (row name, expected route) pairs whose expected route DIFFERS from the
row's default route (the switch demonstrably did something), ``unchanged`` = rows that must keep their default route
because a rule of the dispatcher precedes the switch, and one line saying why the routes follow from the dispatcher
(launch_igemm / run_igemm / launch_wgrad / run_wgrad* of lip_mfma.hip, lip_dot_nt_f64 of lip_krylov.hip).  Row names are
those of kernel_route_cases.BY_NAME and krylov_cases.BY_NAME; the few geometries no existing row has are NEW_CASES below.
Expected routes assume the 256 CUs of an MI355X wherever the row's default does (``cu``).

Left out, on purpose:
  LIP_DBG             synchronises the stream after every launch and prints timing stamps to stderr: a diagnostic, never
                      part of an A/B comparison; it selects no kernel of its own (the stamps are a run-time pointer)
  LIP_SMALLP_FACTOR   numeric threshold of the few-probe rule: both sides of it are LIP_NOSMALLP on / off below
  LIP_WGW_MINBLOCKS   numeric threshold between the Winograd and the direct weight gradient: both are default routes
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import krylov_cases as kc
from kernel_route_cases import BY_NAME as ROUTE_ROWS, T6, Case, conv

EXCLUDED = {"LIP_DBG", "LIP_SMALLP_FACTOR", "LIP_WGW_MINBLOCKS"}


@dataclass
class Entry:
    name: str
    env: Dict[str, str]
    why: str
    rows: List[Tuple[str, str]] = field(default_factory=list)
    unchanged: List[str] = field(default_factory=list)
    # start-up defaults: expected lip_get_precision() / lip_get_winograd() of a process that called no setter, the census
    # of one split-K-eligible launch (ks_2211_bv4) before any setter, and rows run in the precision, Winograd and split-K
    # modes the process started with (run_case then calls no setter; they run before every other row)
    precision: Optional[int] = None
    winograd: Optional[int] = None
    first_launch: Optional[str] = None
    startup_rows: List[Tuple[str, str]] = field(default_factory=list)


# ------------------------------------------------------------------------------------------------ new geometries
# Default routes (checked by the "defaults" entry, in a child without any switch):
#   few probes with N > 64: R > 64 and fewer than 2 x 256 blocks of 128 rows -> the 64-row tile <2,2,1,1>
#   256-row tiles (LIP_TILE=1): R >= 4096, and 32 row tiles x 16 probes = 2 x 256 blocks, the smallest launch that the
#   few-probe rule lets through on 256 CUs -> the 128-row tiles <4,1,1,*>, A operand direct
NEW_CASES: List[Case] = [
    Case("ab_fewp_N128_bv4", "igemm_fast<2,2,1,1>/bv4", conv(1, 12, 16, 128, 2, b_pp=True, epi={"scale": "shared"})),
    Case("an_ab_fewp_N127", "igemm_fast<2,2,1,1>", conv(2, 6, 16, 127, 2, W=20, a_pp=True)),
    Case("ab_r4096_N64_bv4", "igemm_adirect<4,1,1,2>/bv4", conv(4, 32, 16, 64, 16, b_pp=True, epi={"scale": "shared"}), cu=True),
    Case("ab_r4096_N32_bv4", "igemm_adirect<4,1,1,1>/bv4", conv(4, 32, 16, 32, 16, epi={"e0": "probe", "dphi": "shared"}), cu=True),
    Case("an_ab_r4096_N63", "igemm_adirect<4,1,1,2>", conv(4, 16, 16, 63, 16, W=64, a_pp=True), cu=True),
    Case("an_ab_r4096_N31", "igemm_adirect<4,1,1,1>", conv(4, 64, 16, 31, 16, W=16, a_pp=True, epi={"e0": "probe"}), cu=True),
]
NEW_BY_NAME = {c.name: c for c in NEW_CASES}
assert not (set(NEW_BY_NAME) & set(ROUTE_ROWS))
CONV_ROWS: Dict[str, Case] = {**ROUTE_ROWS, **NEW_BY_NAME}
DOT_ROWS = [c.name for c in kc.CASES if c.prim == "dot_nt_f64"]


def default_route(row):
    return CONV_ROWS[row].route if row in CONV_ROWS else kc.BY_NAME[row].route


def tol_of_route(route):
    """the tolerance class follows the kernel a row lands on (constants of tests/test_kernel_routes.py)"""
    return "wino" if "_wino" in route else ("x3" if "/x3" in route else "exact")


def _both(rows):
    """the rows and their anisotropic twins"""
    return list(rows) + [("an_" + r, route) for r, route in rows]


A41 = ("4,1,1,2", "4,1,1,1")           # the tiles of igemm_adirect
DIRECT = [t for t in T6 if t not in A41]

# ------------------------------------------------------------------------------------------------ LIP_NOADIRECT
_noadirect = _both([(f"adirect{t}{b}", f"igemm_fast<{t}>{'/bv4' if b else ''}") for t in A41 for b in ("", "_bv4")]) + \
    [("an_adirect_tall_k2x3_bv4", "igemm_fast<4,1,1,1>/bv4")]

# ------------------------------------------------------------------------------------------------ LIP_GENERIC
# igemm: run_igemm takes igemm_kernel<t> for the tile launch_igemm chose; the tile rule itself is unchanged
_generic_igemm = _both([(f"fast{t}{b}", f"igemm<{t}>") for t in DIRECT for b in ("", "_bv4")] +
                       [(f"adirect{t}{b}", f"igemm<{t}>") for t in A41 for b in ("", "_bv4")] +
                       [(f"fast{t}_par", f"igemm<{t}>") for t in ("2,2,1,2", "4,1,1,2")] +
                       [(f"fast{t}_par_bv4", f"igemm<{t}>") for t in ("2,1,1,1", "2,2,2,2")]) + \
    [("fast_all_epi", "igemm<2,2,1,1>"), ("fast_nseg3_par", "igemm<2,2,1,1>"), ("an_fast_nseg3_par", "igemm<2,2,1,1>"),
     ("work_operands", "igemm<2,1,1,1>"), ("an_tconv_ee", "igemm<2,2,1,1>"), ("an_tconv_par_pad01", "igemm<2,2,1,1>"),
     # the switch is part of igemm_first_ok: the first-layer shapes (R > 64, few blocks) take the 64-row generic tile
     ("first14_C3_P8", "igemm<2,1,1,1>"), ("first14_C1_P256", "igemm<2,1,1,1>"), ("first32_C7_P9", "igemm<2,1,1,1>"),
     ("first32_C5_P64", "igemm<2,1,1,1>"), ("an_first14_wide", "igemm<2,1,1,1>"), ("an_first32_tall_k5x3", "igemm<2,1,1,1>"),
     ("an_first32_s2_10x7", "igemm<2,1,1,1>")]
# igemm_wino_ok precedes run_igemm and does not read the switch
_generic_wino = ["wino_8x8", "wino_12x12", "wino_misaligned_out", "an_wino_8x24", "an_wino_28x6_misaligned_out", "wg_wino_rowq",
                 "wg_wino_12", "an_wg_wino_8x12", "an_wg_wino_12x8"]
# wgrad: the switch is part of wgrad_first_ok, wgrad_skinny_ok and of nopb; run_wgrad takes wgrad_kernel<t> for the tile
# of the rule N > 64: M <= 64 ? <2,2,1,2> : <2,2,2,2>; N > 32: <2,2,1,1> : <4,1,1,2>; else <2,1,1,1> : <4,1,1,1>
_generic_wgrad = [("wg_first", "wgrad<2,1,1,1>"), ("wg_first_C1_P9", "wgrad<2,1,1,1>"), ("an_wg_first", "wgrad<2,1,1,1>"),
                  ("wg_skinny8", "wgrad<2,2,1,1>"), ("wg_skinny8_R3", "wgrad<4,1,1,1>"), ("wg_skinny26", "wgrad<4,1,1,2>"),
                  ("wg_skinny32", "wgrad<2,2,1,1>"), ("wg_skinny32_map", "wgrad<2,2,1,2>"), ("an_wg_skinny8_2x3", "wgrad<4,1,1,2>"),
                  ("an_wg_skinny26_3x2", "wgrad<4,1,1,2>"), ("an_wg_skinny32_4x5", "wgrad<2,2,2,2>"),
                  ("wg_pb96_288", "wgrad<4,1,1,1>"), ("wg_pb96_576", "wgrad<4,1,1,1>"), ("wg_pb96_N64_M576", "wgrad<4,1,1,2>"),
                  ("an_wg_pb96_N64_M576", "wgrad<4,1,1,2>"), ("wg_pb128", "wgrad<4,1,1,1>"), ("wg_pb128_P7N12", "wgrad<4,1,1,1>"),
                  ("wg_pb128_P64", "wgrad<4,1,1,1>"), ("an_wg_pb96_pad10", "wgrad<4,1,1,1>"), ("an_wg_pb96_k2x3", "wgrad<4,1,1,1>"),
                  ("an_wg_pb128_s2_10x7", "wgrad<4,1,1,1>")] + \
    _both([(f"wg_{t.replace(',', '')}_v4", f"wgrad<{t}>") for t in ("2,2,1,2", "2,2,2,2", "2,2,1,1", "4,1,1,2")] +
          [("wg_2111", "wgrad<2,1,1,1>"), ("wg_4111", "wgrad<4,1,1,1>")])

# ------------------------------------------------------------------------------------------------ LIP_NOFIRST / NOSKINNY / NOPB
# igemm: C % 16 != 0, so igemm_fast_ok fails -> igemm<t>; R > 64 with few blocks: the few-probe rule, N = 32 -> <2,1,1,1>.
# wgrad: M <= 32 (<= 64), N <= 32 -> <2,1,1,1>; C % 4 != 0 -> wgrad_kernel
_nofirst = [(r, "igemm<2,1,1,1>") for r in ("first14_C3_P8", "first14_C1_P256", "first32_C7_P9", "first32_C5_P64", "an_first14_wide",
                                            "an_first32_tall_k5x3", "an_first32_s2_10x7")] + \
           [(r, "wgrad<2,1,1,1>") for r in ("wg_first", "wg_first_C1_P9", "an_wg_first")]
# the tile rule on (M, N); C % 4 == 0 and a 16-byte aligned a -> wgrad_fast, /v4 on the 64+ column tiles when N % 4 == 0;
# an_wg_skinny8_2x3 (M = 96, N = 40, P = 2) is a probe-batched shape: wgrad_pb<1,4,3,1>
_noskinny = [("wg_skinny8", "wgrad_fast<2,2,1,1>"), ("wg_skinny8_R3", "wgrad<4,1,1,1>"), ("wg_skinny26", "wgrad<4,1,1,2>"),
             ("wg_skinny32", "wgrad_fast<2,2,1,1>/v4"), ("wg_skinny32_map", "wgrad_fast<2,2,1,2>/v4"),
             ("an_wg_skinny8_2x3", "wgrad_pb<1,4,3,1>"), ("an_wg_skinny26_3x2", "wgrad_fast<4,1,1,2>"),
             ("an_wg_skinny32_4x5", "wgrad_fast<2,2,2,2>/v4")]
# M >= 96 and N <= 32 -> <4,1,1,1> (32 columns: no /v4); N = 64 -> <4,1,1,2>/v4
_nopb = [(r, "wgrad_fast<4,1,1,1>") for r in ("wg_pb96_288", "wg_pb96_576", "wg_pb128", "wg_pb128_P7N12", "wg_pb128_P64", "an_wg_pb96_288",
                                              "an_wg_pb128", "an_wg_pb128_P7N12", "an_wg_pb96_pad10", "an_wg_pb96_k2x3",
                                              "an_wg_pb128_s2_10x7")] + \
        [("wg_pb96_x3", "wgrad_fast<4,1,1,1>/x3"), ("wg_pb128_x3", "wgrad_fast<4,1,1,1>/x3"), ("an_wg_pb96_x3", "wgrad_fast<4,1,1,1>/x3"),
         ("an_wg_pb128_x3", "wgrad_fast<4,1,1,1>/x3"), ("wg_pb96_N64_M576", "wgrad_fast<4,1,1,2>/v4"),
         ("an_wg_pb96_N64_M576", "wgrad_fast<4,1,1,2>/v4")]

# ------------------------------------------------------------------------------------------------ LIP_NOPAR
# par = false in run_igemm: the <2,...> tiles take igemm_fast<t>[/bv4] in the plain row order, the <4,1,...> tiles the
# A-direct kernel (its only launches in mode 1 at stride 2), split precision /x3 without /par
_nopar = _both([(f"fast{t}_par", f"igemm_fast<{t}>") for t in DIRECT] + [(f"fast{t}_par_bv4", f"igemm_fast<{t}>/bv4") for t in DIRECT] +
               [(f"fast{t}_par", f"igemm_adirect<{t}>") for t in A41] + [(f"fast{t}_par_bv4", f"igemm_adirect<{t}>/bv4") for t in A41] +
               [(f"fast{t}_x3_par", f"igemm_fast<{t}>/x3") for t in T6]) + \
    [("an_tconv_ee", "igemm_fast<2,2,1,1>/bv4"), ("an_tconv_par_pad01", "igemm_fast<2,2,1,1>")]

# ------------------------------------------------------------------------------------------------ LIP_NOBV4
_nobv4 = _both([(f"fast{t}_bv4", f"igemm_fast<{t}>") for t in DIRECT] + [(f"adirect{t}_bv4", f"igemm_adirect<{t}>") for t in A41] +
               [(f"fast{t}_par_bv4", f"igemm_fast<{t}>/par") for t in ("2,2,1,2", "4,1,1,1")] +
               [("ks_2211_bv4", "igemm_fast<2,2,1,1>/ks"), ("ks_2111_bv4", "igemm_fast<2,1,1,1>/ks")] +
               [(f"wg_{t.replace(',', '')}_v4", f"wgrad_fast<{t}>") for t in ("2,2,1,2", "2,2,2,2", "2,2,1,1", "4,1,1,2")])

# ------------------------------------------------------------------------------------------------ LIP_WINO_NOVEPI
_novepi = [(r, "igemm_wino") for r, c in ROUTE_ROWS.items() if c.route == "igemm_wino/vepi"]

# ------------------------------------------------------------------------------------------------ LIP_NOSMALLP
# without the few-probe rule R > 64 takes the 128-row tiles: N > 64 <2,2,2,2>, 33..64 <4,1,1,2>, <= 32 <4,1,1,1> (the
# <4,1,...> tiles A-direct unless /par or /x3; C % 16 != 0 generic)
_nosmallp = [("ab_fewp_N128_bv4", "igemm_fast<2,2,2,2>/bv4"), ("an_ab_fewp_N127", "igemm_fast<2,2,2,2>"),
             ("ks_below", "igemm_adirect<4,1,1,2>/bv4"), ("an_fast_wide", "igemm_adirect<4,1,1,2>"),
             ("an_fast_tall_k1x3_bv4", "igemm_adirect<4,1,1,2>/bv4"), ("an_fast_k3x1", "igemm_adirect<4,1,1,1>"),
             ("an_wino_8x7_ineligible", "igemm_adirect<4,1,1,1>/bv4"), ("an_generic_tall_k5x3", "igemm<4,1,1,2>"),
             ("an_tconv_ee", "igemm_fast<4,1,1,2>/par/bv4"), ("an_tconv_par_pad01", "igemm_fast<4,1,1,2>/par"),
             ("an_tconv_eo_x3", "igemm_fast<4,1,1,2>/x3")]

# ------------------------------------------------------------------------------------------------ LIP_TILE
# 2: one-wave blocks, N <= 32 <1,1,1,1>, 33..64 <1,1,1,2>; 3: <1,1,2,1> (N <= 32).  The override follows the few-probe
# rule, so the rows have R <= 64.  4 sends N <= 32 to <2,1,1,1>, which R <= 64 takes anyway: its rows have R = 1024 and
# enough probes to pass the few-probe rule (default <4,1,1,1>, A-direct).  1: 256-row tiles <4,1,2,*> for R >= 4096
_tile2 = _both([("fast2,1,1,1", "igemm_fast<1,1,1,1>"), ("fast2,1,1,1_bv4", "igemm_fast<1,1,1,1>/bv4"),
                ("fast2,2,1,1", "igemm_fast<1,1,1,2>"), ("fast2,2,1,1_bv4", "igemm_fast<1,1,1,2>/bv4"),
                ("fast2,1,1,1_par", "igemm_fast<1,1,1,1>/par"), ("fast2,2,1,1_par_bv4", "igemm_fast<1,1,1,2>/par/bv4"),
                ("generic2,1,1,1", "igemm<1,1,1,1>"), ("generic2,2,1,1", "igemm<1,1,1,2>")])
_tile3 = _both([("fast2,1,1,1", "igemm_fast<1,1,2,1>"), ("fast2,1,1,1_bv4", "igemm_fast<1,1,2,1>/bv4"),
                ("fast2,1,1,1_par_bv4", "igemm_fast<1,1,2,1>/par/bv4"), ("generic2,1,1,1", "igemm<1,1,2,1>")])
_tile4 = _both([("adirect4,1,1,1", "igemm_fast<2,1,1,1>"), ("adirect4,1,1,1_bv4", "igemm_fast<2,1,1,1>/bv4"),
                ("fast4,1,1,1_par", "igemm_fast<2,1,1,1>/par")])
_tile1 = [("ab_r4096_N64_bv4", "igemm_adirect<4,1,2,2>/bv4"), ("ab_r4096_N32_bv4", "igemm_adirect<4,1,2,1>/bv4"),
          ("an_ab_r4096_N63", "igemm_adirect<4,1,2,2>"), ("an_ab_r4096_N31", "igemm_adirect<4,1,2,1>")]
_tile1_noad = [(r, route.replace("igemm_adirect", "igemm_fast")) for r, route in _tile1]

# ------------------------------------------------------------------------------------------------ lip_dot_nt_f64
# part against atomic as dot_nt_plan decides it (the K-ranges and the scratch test precede the switches)
_valu = [(r, "dot_nt/valu/" + default_route(r).rsplit("/", 1)[1]) for r in DOT_ROWS]
_noquad = [(r, "dot_nt/tile/" + default_route(r).rsplit("/", 1)[1]) for r in DOT_ROWS if default_route(r).startswith("dot_nt/quad/")]
_noquad_same = [r for r in DOT_ROWS if default_route(r).startswith("dot_nt/tile/")]

KS_ROW, KS_ROUTE = "ks_2211_bv4", "igemm_fast<2,2,1,1>/ks/bv4"      # the split-K-eligible launch every child starts with

ENTRIES: List[Entry] = [
    Entry("defaults", {}, "no switch: the new geometries take the default routes their Case states; start-up modes f32, Winograd on, "
          "split-K on", rows=[], unchanged=[c.name for c in NEW_CASES], precision=0, winograd=1, first_launch=KS_ROUTE),
    Entry("noadirect", {"LIP_NOADIRECT": "1"}, "run_igemm<4,1,..>: noad skips the igemm_adirect launch, the LIP_LAUNCH_IGEMM ladder follows",
          rows=_noadirect),
    Entry("wgrad3", {"LIP_WGRAD3": "1"}, "launch_wgrad: M % 96 == 0 && M % 128 != 0 with w3 -> run_wgrad_pb<3,1,1,4> in f32 mode",
          rows=[(r, "wgrad_pb<3,1,1,4>") for r in ("wg_pb96_288", "wg_pb96_576", "wg_pb96_N64_M576", "an_wg_pb96_288", "an_wg_pb96_pad10",
                                                   "an_wg_pb96_k2x3", "an_wg_pb96_N64_M576")]),
    Entry("generic_igemm", {"LIP_GENERIC": "1"}, "run_igemm: force_generic -> igemm_kernel<t>, t by the unchanged tile rule; igemm_first_ok is "
          "off; igemm_wino_ok precedes run_igemm and does not read the switch", rows=_generic_igemm, unchanged=_generic_wino[:5]),
    Entry("generic_wgrad", {"LIP_GENERIC": "1"}, "launch_wgrad: first, skinny and probe-batched off; run_wgrad: force_generic -> wgrad_kernel<t>; "
          "wgrad_wino_ok precedes and does not read the switch", rows=_generic_wgrad, unchanged=_generic_wino[5:]),
    Entry("nofirst", {"LIP_NOFIRST": "1"}, "igemm_first_ok / wgrad_first_ok off: C % 16 != 0 (C % 4 != 0) -> the generic kernel on the 64-row tile",
          rows=_nofirst),
    Entry("noskinny", {"LIP_NOSKINNY": "1"}, "wgrad_skinny_ok off: the per-probe tile rule on (M, N), or the probe-batched tile where pb_ok holds",
          rows=_noskinny),
    Entry("nopb", {"LIP_NOPB": "1"}, "launch_wgrad: pb_ok false -> run_wgrad<4,1,1,1> (N <= 32) / <4,1,1,2> (N = 64)", rows=_nopb),
    Entry("nopb96", {"LIP_NOPB96": "1"}, "launch_wgrad: N = 64, M = 576 fails N <= 32 and 5 * waste128 >= M, so without pb96 it leaves the "
          "probe-batched branch: run_wgrad<4,1,1,2>, N % 4 == 0 -> /v4",
          rows=[("wg_pb96_N64_M576", "wgrad_fast<4,1,1,2>/v4"), ("an_wg_pb96_N64_M576", "wgrad_fast<4,1,1,2>/v4")],
          unchanged=["wg_pb96_576", "an_wg_pb96_pad10"]),
    Entry("nopar", {"LIP_NOPAR": "1"}, "run_igemm: par false -> plain row order; WM == 4 && WN == 1 && !par -> igemm_adirect (mode 1, stride 2)",
          rows=_nopar),
    Entry("nobv4", {"LIP_NOBV4": "1"}, "run_igemm: bv4 false on every ladder (ks, adirect, par, plain); run_wgrad: the /v4 launch is skipped",
          rows=_nobv4),
    Entry("wino_novepi", {"LIP_WINO_NOVEPI": "1"}, "run_igemm_wino: vepi false -> igemm_wino_kernel<false>", rows=_novepi,
          unchanged=["wino_misaligned_out", "an_wino_28x6_misaligned_out"]),
    Entry("nosmallp", {"LIP_NOSMALLP": "1"}, "launch_igemm: the few-probe clause is skipped, R > 64 -> the 128-row tile of the column count",
          rows=_nosmallp),
    Entry("tile2", {"LIP_TILE": "2"}, "launch_igemm: tile_override() == 2 && N <= 64 -> <1,1,1,2> (N > 32) / <1,1,1,1>, after the few-probe rule",
          rows=_tile2),
    Entry("tile3", {"LIP_TILE": "3"}, "launch_igemm: tile_override() == 3 && N <= 32 -> <1,1,2,1>", rows=_tile3),
    Entry("tile4", {"LIP_TILE": "4"}, "launch_igemm: tile_override() == 4 && N <= 32 -> <2,1,1,1> whatever R (R <= 64 takes it by default, so "
          "the rows have R = 1024 and pass the few-probe rule)", rows=_tile4),
    Entry("tile1", {"LIP_TILE": "1"}, "launch_igemm: big_m (R >= 4096) -> <4,1,2,2> (N > 32) / <4,1,2,1>; run_igemm: A-direct", rows=_tile1),
    Entry("tile1_noadirect", {"LIP_TILE": "1", "LIP_NOADIRECT": "1"}, "as tile1, noad -> igemm_fast<4,1,2,*>", rows=_tile1_noad),
    Entry("dot_nt_valu", {"LIP_DOT_NT_VALU": "1"}, "lip_dot_nt_f64: valu -> dot_nt_f64_kernel, part / atomic by the scratch test", rows=_valu),
    Entry("dot_nt_noquad", {"LIP_DOT_NT_NOQUAD": "1"}, "lip_dot_nt_f64: noquad -> dot_nt_f64_mfma_kernel<false>; the rows that take it by default "
          "stay", rows=_noquad, unchanged=_noquad_same),
    Entry("precision_bf16x3", {"LIP_PRECISION": "bf16x3"}, "precision_mode(): first read of the environment -> 1; run_igemm: split -> /x3, no "
          "A-direct, no split-K (the first launch is unsplit, dword B loads)", precision=1, winograd=1, first_launch="igemm_fast<2,2,1,1>/x3",
          startup_rows=[("fast2,2,1,1", "igemm_fast<2,2,1,1>/x3"), ("an_fast2,2,1,2_bv4", "igemm_fast<2,2,1,2>/x3"),
                        ("wino_8x8", "igemm_fast<2,1,1,1>/x3")]),
    Entry("nowino", {"LIP_NOWINO": "1"}, "wino_mode(): first read -> 0; igemm_wino_ok / wgrad_wino_ok false -> the direct kernels", precision=0,
          winograd=0, first_launch=KS_ROUTE,
          startup_rows=[("wino_8x8", "igemm_fast<2,1,1,1>/bv4"), ("an_wino_8x24", "igemm_fast<2,1,1,1>/bv4"),
                        ("wg_wino_rowq", "wgrad_pb<1,4,3,1>")]),
    Entry("wino_f", {"LIP_WINO": "f"}, "wino_mode(): first read -> 2 (the same launches as 1)", precision=0, winograd=2, first_launch=KS_ROUTE,
          unchanged=["wino_8x8", "an_wino_8x24"]),
    Entry("noksplit", {"LIP_NOKSPLIT": "1"}, "split_k_enabled(): first read -> off; run_igemm<2,2,1,1>: noks -> the plain ladder", precision=0,
          winograd=1, first_launch="igemm_fast<2,2,1,1>/bv4",
          startup_rows=[("ks_2211_bv4", "igemm_fast<2,2,1,1>/bv4"), ("ks_2111", "igemm_fast<2,1,1,1>"),
                        ("an_ks_2211_bv4", "igemm_fast<2,2,1,1>/bv4"), ("an_ks_2211", "igemm_fast<2,2,1,1>")]),
]
BY_ENTRY = {e.name: e for e in ENTRIES}
assert len(BY_ENTRY) == len(ENTRIES)
