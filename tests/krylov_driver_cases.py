"""One row per path and edge of the Krylov drivers (krylov.py) — TEST INFRASTRUCTURE (a plain helper module).

A ``Case`` names the driver, the operator and the start block it is run on (built by :func:`problem`: float32 tensors on
the CPU, which tests/test_krylov_drivers.py moves to the device and tests/krylov_driver_ref.py runs in float64 and
float32), the group of assertions it belongs to and the edge it is there for.  ``covers`` lists the public drivers of
krylov.py and the keywords of ``cg`` the row exercises; tests/test_krylov_drivers_cpu.py asserts that together they
reach all of them, and that every row is what its ``why`` says (breakdown step, conditioning, iteration counts).

Bit-for-bit rows: ``lip_multi_dot`` adds the partial sums of its four waves with LDS atomics, in whatever order they
arrive, so a Lanczos / Golub-Kahan run repeats bit for bit only where a single wave holds data — N <= 256; ``lip_bdot``
splits a row by its 16-byte alignment, so a row is compared with a run in which it sits at the same offset of its block
(a slice of the block, or the block with ANOTHER row exchanged).  The CG kernels run one block up to N = 2048 and add in
a fixed order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

import krylov_driver_ref as R

PUBLIC_DRIVERS = {"lanczos_tridiag", "funm_lanczos_sym", "funm_lanczos_dense", "dense_funm_sym_eigh", "tridiag_dense", "cg",
                  "cg_dense", "bidiag", "slq_logdet_product", "RangeDeflation", "cg_deflated", "gram_orthonormalize"}
CG_KEYWORDS = {"x0", "tol", "atol", "maxiter", "check_every", "stall", "keep_best"}
SIZES = {1, 2, 3, 24, 37, 1027, 1030, 1031, 4099}
LONG = 100003


@dataclass
class Case:
    name: str
    driver: str                      # lanczos | funm | funm_dense | cg | cg_dense | bidiag | deflation | gram
    group: str                       # which assertions of the test files apply
    d: Dict
    why: str
    covers: Tuple[str, ...] = ()
    allow: int = 2                   # iteration-count allowance of a CG row (float32 against float64)


def _g(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_g(seed), dtype=torch.float64).float()


def operator(d: Dict) -> R.Operator:
    kind, N = d["op"], d["N"]
    if kind == "diag_lin":
        return R.op_diag(torch.linspace(d.get("lo", 1.0), d.get("hi", 2.0), N, dtype=torch.float64), noisy=d.get("noisy", False))
    if kind == "diag_log":
        return R.op_diag(torch.logspace(0.0, d.get("decades", 2.0), N, dtype=torch.float64), noisy=d.get("noisy", False))
    if kind == "diag_five":                          # five distinct eigenvalues with multiplicities 1, 2, 3, ... (cyclic)
        vals = torch.tensor([0.5, 1.0, 1.5, 2.0, 2.5], dtype=torch.float64)
        return R.op_diag(vals[torch.arange(N) % 5])
    if kind == "outliers":
        return R.op_outliers(N)
    if kind == "dense":
        return R.op_dense_sym(N, d.get("seed", 1))
    if kind == "lowrank":
        return R.op_lowrank(N, 2, d.get("seed", 2))
    if kind == "rect":
        return R.op_rect(d["n_out"], N, d.get("seed", 3))
    if kind == "defl":
        return R.op_deflation(N, d["r"], d.get("seed", 4))
    raise KeyError(kind)


def problem(case: "Case"):
    """(operator, start block / right-hand sides (P, N) float32 on the CPU)"""
    d = case.d
    op = operator(d)
    N, P = d["N"], d["P"]
    V = _randn(P, N, seed=d.get("vseed", 11))
    for p, what in d.get("rows", {}).items():
        if what == "zero":
            V[p] = 0.0
        elif what == "eigvec" and d["op"] == "lowrank":      # B^T v = 0 exactly: an eigenvector of the eigenvalue 0.5
            V[p] = 0.0
            V[p, 3], V[p, 4], V[p, 5] = 1.5, -1.5, 0.75
        elif what == "eigvec" and d["op"] == "dense":
            V[p] = (1.5 * torch.linalg.eigh(op.dense())[1][:, -1]).float()
        elif what == "eigvec":                       # a unit vector of a diagonal map: every sum has one term, exact
            V[p] = 0.0
            V[p, 17 % N] = 2.5
        elif what == "inv2":                         # in the invariant subspace range(B) of 0.5 I + B B^T, exactly
            V[p] = (op.t["B"].double() @ torch.tensor([0.75, -1.25], dtype=torch.float64)).float()
    return op, V.contiguous()


def cg_kwargs(case: "Case", B: torch.Tensor) -> Dict:
    """the keywords of ``cg`` a row sets (atol relative to the smallest right-hand side)"""
    d = case.d
    kw = dict(tol=d.get("tol", 1e-5))
    if "atol_rel" in d:
        kw["atol"] = d["atol_rel"] * float(B.double().norm(dim=1).min())
    if "maxiter" in d:
        kw["maxiter"] = d["maxiter"]
    return kw


def _lanczos_rows():
    L = ("lanczos_tridiag",)
    out = [
        Case("lz/well", "lanczos", "elementwise", dict(op="diag_lin", N=1031, P=3, k=12),
             "far from convergence: T and Q well conditioned; N % 4 == 3 (padded ldq)", L),
        Case("lz/well_1030", "lanczos", "elementwise", dict(op="diag_lin", N=1030, P=2, k=7), "N % 4 == 2", L),
        Case("lz/dense37", "lanczos", "elementwise", dict(op="dense", N=37, P=2, k=8), "dense operator, N % 4 == 1, one wave", L),
        Case("lz/dense24", "lanczos", "elementwise", dict(op="dense", N=24, P=4, k=6), "N % 4 == 0: no padding", L),
        Case("lz/blocks", "lanczos", "elementwise", dict(op="diag_lin", N=4099, P=2, k=6), "three blocks per row: atomics between blocks", L),
        Case("lz/long", "lanczos", "elementwise", dict(op="diag_lin", N=LONG, P=1, k=4), "long row, P = 1", L),
        Case("lz/full24", "lanczos", "full", dict(op="dense", N=24, P=2, k=24), "k = N: eig(T) = eig(A), Q square orthogonal", L),
        Case("lz/full1", "lanczos", "full", dict(op="dense", N=1, P=1, k=1), "N = k = 1, P = 1, empty off", L),
        Case("lz/full2", "lanczos", "full", dict(op="dense", N=2, P=2, k=2), "N = k = 2", L),
        Case("lz/full3", "lanczos", "full", dict(op="dense", N=3, P=1, k=3), "N = k = 3", L),
        Case("lz/k1", "lanczos", "elementwise", dict(op="diag_lin", N=1030, P=3, k=1), "k = 1: empty off", L),
        Case("lz/breakdown", "lanczos", "breakdown",
             dict(op="lowrank", N=37, P=4, k=8, rows={1: "inv2", 2: "eigvec"}, steps=[2, 1, 0, 2]),
             "0.5 I + B B^T, B (37, 2): generic probes span 3 dimensions (off[2:] == 0, diag[3:] == 1), probe 1 starts in "
             "range(B) (off[1:] == 0), probe 2 on an eigenvector (off[0] == 0, diag[0] == lam); each equals its own P = 1 run",
             L + ("funm_lanczos_sym", "dense_funm_sym_eigh", "tridiag_dense")),
        Case("lz/zero_mid", "lanczos", "zero_row", dict(op="dense", N=37, P=4, k=6, rows={1: "zero"}, zero=1),
             "a zero start row among non-zero ones: zero basis rows, diag 1, off 0; the others as in the block with ANOTHER "
             "row 1", L + ("funm_lanczos_sym",)),
        Case("lz/zero_last", "lanczos", "zero_row", dict(op="dense", N=37, P=4, k=6, rows={3: "zero"}, zero=3),
             "a zero last row: the others as in the block without it (a slice)", L + ("funm_lanczos_sym",)),
        Case("lz/scale", "lanczos", "scaling", dict(op="dense", N=37, P=2, k=8), "operator x 2^-20, 2^+20: T scales, Q identical", L),
        Case("lz/scale_breakdown", "lanczos", "scaling",
             dict(op="lowrank", N=37, P=3, k=6, rows={1: "inv2"}, steps=[2, 1, 2]),
             "the breakdown threshold is scale-free: same dead steps under 2^-20, 2^+20", L),
    ]
    F = ("funm_lanczos_sym", "dense_funm_sym_eigh", "tridiag_dense", "lanczos_tridiag")
    out += [
        Case("fn/one", "funm", "funm", dict(op="dense", N=37, P=3, k=5, f="one"), "f = 1 returns b", F),
        Case("fn/ident_k2", "funm", "funm", dict(op="diag_lin", N=1031, P=3, k=2, f="ident"), "f(x) = x returns A b at k = 2", F),
        Case("fn/ident_k7", "funm", "funm", dict(op="dense", N=24, P=2, k=7, f="ident"), "f(x) = x returns A b at any k >= 2", F),
        Case("fn/five_k5", "funm", "funm", dict(op="diag_five", N=1030, P=3, k=5, f="invsqrt"), "five eigenvalues: exact at k = 5", F),
        Case("fn/five_k5_inv", "funm", "funm", dict(op="diag_five", N=1030, P=3, k=5, f="inv"), "x^-1, exact at k = 5", F),
        Case("fn/five_k8", "funm", "funm", dict(op="diag_five", N=1030, P=3, k=8, f="invsqrt", steps=[4, 4, 4]),
             "k = 8 > 5: through the breakdown guard", F),
        Case("fn/five_k8_inv", "funm", "funm", dict(op="diag_five", N=1030, P=3, k=8, f="inv", steps=[4, 4, 4]), "x^-1 through the guard", F),
        Case("fn/floor", "funm", "funm", dict(op="diag_five", N=1030, P=2, k=5, f="invsqrt", floor=0.75),
             "floor = 0.75 raises the Ritz value 0.5", F),
        Case("fn/clip", "funm", "funm", dict(op="diag_five", N=1030, P=2, k=5, f="invsqrt", clip_min=1.25),
             "clip_min = 1.25 raises 0.5 and 1.0 (the reference's monkey-patch clips at 1)", F),
        Case("fn/floor_clip", "funm", "funm", dict(op="diag_five", N=1030, P=2, k=5, f="inv", floor=0.75, clip_min=1.25), "both clamps", F),
    ]
    D = ("funm_lanczos_dense", "dense_funm_sym_eigh", "tridiag_dense")
    out += [
        Case("fd/dense24", "funm_dense", "funm_dense", dict(op="dense", N=24, P=3, k=24, f="invsqrt", exact=True), "full depth in float64: exact", D),
        Case("fd/breakdown", "funm_dense", "funm_dense", dict(op="lowrank", N=37, P=4, k=8, f="invsqrt", rows={1: "inv2", 2: "eigvec"}, exact=True),
             "the float64 twin's breakdown guard: exact", D),
        Case("fd/zero_row", "funm_dense", "funm_dense", dict(op="dense", N=37, P=3, k=6, f="inv", rows={1: "zero"}, zero=1),
             "alive = length > 0: a zero row returns zero; k = 6 of 37: not converged, held to the float64 recurrence of the same k", D),
        Case("fd/k_gt_d", "funm_dense", "funm_dense", dict(op="dense", N=3, P=2, k=8, f="inv", exact=True), "k > d is cut to d: exact", D),
    ]
    return out


def _cg_rows():
    base = dict(op="diag_log", N=1027, P=4)
    return [
        Case("cg/spd", "cg", "cg", dict(base), "SPD diagonal, cond 1e2: X, iterations, residual_norm", ("cg", "tol")),
        Case("cg/small", "cg", "cg", dict(op="dense", N=3, P=2), "N = 3", ("cg",)),
        Case("cg/N1", "cg", "cg", dict(op="dense", N=1, P=1), "N = 1, P = 1: one step", ("cg",)),
        Case("cg/blocks", "cg", "cg", dict(op="diag_log", N=4099, P=3, decades=1.0), "two blocks per row in cg_update", ("cg",)),
        Case("cg/long", "cg", "cg", dict(op="diag_log", N=LONG, P=2, decades=1.0), "long rows", ("cg",)),
        Case("cg/frozen", "cg", "cg_frozen", dict(op="diag_lin", hi=10.0, N=1027, P=4, rows={3: "eigvec"}, special=3),
             "row 3 is a unit vector (one step, every sum exact): frozen while the others run ~20 steps; bit-identical to "
             "its P = 1 run, the others to their P = 3 run", ("cg",)),
        Case("cg/zero_row", "cg", "cg_frozen", dict(op="diag_lin", hi=10.0, N=1027, P=4, rows={3: "zero"}, special=3),
             "a zero right-hand side: x = 0, nothing NaN, the others as without it", ("cg",)),
        Case("cg/x0_exact", "cg", "cg_x0", dict(base, x0="exact"), "x0 = the rounded exact solution: 0 iterations, x0 returned", ("cg", "x0")),
        Case("cg/x0_random", "cg", "cg_x0", dict(base, x0="random"), "a random x0: the same solution", ("cg", "x0")),
        Case("cg/atol", "cg", "cg", dict(base, atol_rel=1e-2), "atol = 1e-2 ||b||_min > tol ||b||: atol decides the stop", ("cg", "atol")),
        Case("cg/maxiter", "cg", "cg_maxiter", dict(base, maxiter=4), "maxiter = 4 reached: the 4th iterate", ("cg", "maxiter")),
        Case("cg/check_every", "cg", "cg_check", dict(base, check_every=3), "check_every = 3: same X, iterations a multiple of 3",
             ("cg", "check_every")),
        Case("cg/stall", "cg", "cg_noise", dict(op="outliers", N=1027, P=2, tol=1e-6, maxiter=20, stall=3, stops=[13, 5]),
             "bfloat16-rounded product, oscillating residual: plain CG runs to maxiter, stall = 3 stops after the first "
             "three steps in a row without improvement (steps 13 and 5)", ("cg", "stall", "maxiter", "tol")),
        Case("cg/keep_best", "cg", "cg_noise", dict(op="outliers", N=1027, P=2, tol=1e-6, maxiter=20, stall=3, keep_best=True),
             "keep_best returns the iterate of smallest true residual, which is NOT the last one", ("cg", "keep_best")),
        Case("cgd/mixed", "cg_dense", "cg_dense", dict(op="dense", N=37, P=4, rows={1: "zero", 2: "eigvec"}),
             "explicit matrix in float64: mixed difficulty and a zero row", ("cg_dense",)),
    ]


def _bidiag_rows():
    Bd = ("bidiag",)
    return [
        Case("bd/tall", "bidiag", "bidiag", dict(op="rect", N=23, n_out=45, P=3, k=6), "N = 23 -> 45: both paddings", Bd),
        Case("bd/wide", "bidiag", "bidiag", dict(op="rect", N=1031, n_out=37, P=3, k=6), "N = 1031 -> 37", Bd),
        Case("bd/full", "bidiag", "slq", dict(op="rect", N=23, n_out=45, P=2, k=23), "k = N, full rank: the quadrature is exact",
             Bd + ("slq_logdet_product",)),
        Case("bd/k1", "bidiag", "slq", dict(op="rect", N=3, n_out=24, P=2, k=1), "k = 1: empty betas", Bd + ("slq_logdet_product",)),
        Case("bd/zero_mid", "bidiag", "bd_zero", dict(op="rect", N=23, n_out=45, P=4, k=5, rows={1: "zero"}, zero=1),
             "a zero start row: finite output, log-det term 0, the others as in the block with ANOTHER row 1",
             Bd + ("slq_logdet_product",)),
        Case("bd/zero_last", "bidiag", "bd_zero", dict(op="rect", N=23, n_out=45, P=4, k=5, rows={3: "zero"}, zero=3),
             "a zero last row: the others as in the block without it", Bd + ("slq_logdet_product",)),
    ]


def _deflation_rows():
    d = dict(op="defl", N=1030, r=5)
    Df = ("RangeDeflation",)
    return [
        Case("df/coeffs_S3", "deflation", "df_coeffs", dict(d, P=3), "S = 3 < 32: dot_nt", Df),
        Case("df/coeffs_S33", "deflation", "df_coeffs", dict(d, P=33), "S = 33 >= 32: gemm_nt", Df),
        Case("df/closed_form", "deflation", "df_closed", dict(d, P=3), "range_part, closed_form for x^-1/2 and x^-1", Df),
        Case("df/project", "deflation", "df_project", dict(d, P=3), "project_out with passes = 1, 2 and C=", Df),
        Case("df/relres", "deflation", "df_relres", dict(d, P=3), "relative_residual of the exact solution and of known perturbations", Df),
        Case("df/cg_deflated", "deflation", "df_cg", dict(d, P=3), "forward error and result orthogonality; keep_best by default",
             Df + ("cg_deflated", "cg", "keep_best")),
        Case("df/wrap", "deflation", "df_wrap", dict(d, P=2), "the Winograd route is off inside the product and restored after, also on a raise", Df),
    ]


def _gram_rows():
    G = ("gram_orthonormalize",)
    return [
        Case("go/chol", "gram", "gram", dict(s=36, N=1031, branch="chol"), "s <= 64: CholeskyQR, with the transform", G),
        Case("go/eigh_s65", "gram", "gram", dict(s=65, N=1030, branch="eigh"), "64 < s: the eigendecomposition from the start", G),
        Case("go/eigh_s384", "gram", "gram", dict(s=384, N=4099, branch="eigh"), "s = 384, the largest on this path", G),
        Case("go/qr", "gram", "gram", dict(s=24, N=37, branch="qr"), "N < 4 s: Householder QR in float64", G),
        Case("go/zero", "gram", "gram_zero", dict(s=5, N=1031, branch="zero"), "all-zero Y: empty Q, a (0, s) transform", G),
    ]


CASES: List[Case] = _lanczos_rows() + _cg_rows() + _bidiag_rows() + _deflation_rows() + _gram_rows()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def group(name: str) -> List[Case]:
    return [c for c in CASES if c.group == name]


FUNS = {
    "one": lambda x: torch.ones_like(x),
    "ident": lambda x: x,
    "invsqrt": lambda x: x ** -0.5,
    "inv": lambda x: 1.0 / x,
}


def gram_branch(s: int, N: int) -> str:
    """mirror of the branch choice of ``gram_orthonormalize`` for a full-rank, well-conditioned Y"""
    if s > 384 or N < 4 * s:
        return "qr"
    return "chol" if s <= 64 else "eigh"
