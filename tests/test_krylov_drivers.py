"""GPU: the drivers of krylov.py — Lanczos, f(A) b, CG, Golub-Kahan, the deflation, gram_orthonormalize — against the
float64 recurrences, case by case.

Each row of tests/krylov_driver_cases.py is one run of a driver on an operator that float64 and float32 see alike
(float32 tensors on the device, their exact images on the CPU; no network, no engine).  The reference is
oracle/matfree.py where it has the function and tests/krylov_driver_ref.py otherwise, in float64; the same recurrence run
in float32 on the CPU gives ``D32``, and every floating-point quantity is bounded by ``max(8 D32, 4 * 2^-24 * scale)``
(``R.bound``; 8 for the kernels' wave and block trees against a sequential sum).  Bit-for-bit claims have no tolerance,
iteration counts the allowance of their row.  Every figure is printed (``STAT``) before it is asserted; the largest
ratios to D32 measured on an MI355X are listed in DESIGN.md section 5.
"""
import functools

import pytest
import torch

from lip_amd import _native as nv
from lip_amd import krylov as K
import krylov_driver_ref as R
from krylov_driver_cases import BY_NAME, CASES, FUNS, cg_kwargs, group, problem
from oracle import matfree as om

pytestmark = pytest.mark.gpu

# Measured on an MI355X: every figure is printed as a STAT line, and one run's figures stand, quantity by quantity, in
# MEASURED at the end of this file (`bound` is max(8 D32, 4 * 2^-24 * scale)).  Per driver, the quantity that used most of
# its bound, and the largest ratio to D32 among the quantities whose bound D32 sets:
#   driver            quantity (row)                      measured    D32         bound       measured / D32 (largest)
#   Lanczos           diag (lz/zero_last)                 2.398e-07   1.179e-07   9.430e-07   2.03
#                     Q (lz/dense37)                      1.441e-06   9.382e-07   7.505e-06   1.54
#   funm_lanczos_sym  f(A) b (fn/one)                     2.384e-07   1.192e-07   9.537e-07   2.00
#                     f(A) b (fn/ident_k7)                6.998e-07   3.806e-07   3.044e-06   1.84
#   cg                residual_norm[0] (cg/small)         2.189e-07   2.103e-08   5.234e-07   (floor 4 * 2^-24 ||b||)
#                     X[0] - exact (cg/small)             1.435e-07   3.678e-08   4.206e-07   (floor 4 * 2^-24 ||x||)
#                     X[1] at step 5 (cg/stall)           1.042e-03   5.233e-04   4.186e-03   1.99
#   bidiag            alphas (bd/wide)                    2.519e-07   1.633e-07   1.306e-06   1.54
#   RangeDeflation    coeffs, gemm_nt (df/coeffs_S33)     3.508e-06   1.268e-06   1.015e-05   2.77
#                     relative_residual (df/relres)       3.360e-08   3.931e-08   3.145e-07   0.86
#   gram_orthon.      T Y - Q (go/eigh_s384)              6.866e-08   4.221e-08   3.376e-07   1.63
#   float64 twins     against the CPU float64 recurrence of the same depth: funm_lanczos_dense 2.8e-15 (fd/dense24),
#                     2.0e-15 (fd/zero_row, k = 6 of 37); cg_dense 6.7e-16
# Iteration counts equal the float64 counts in every row (allowance 2); cg/stall stops at step 13 (rows at 13 and 5 as in
# the reference), cg/keep_best keeps iterates 10 and 2 of 13.
# Against the parent commit the four zero-start-row tests failed (NaN basis, diag / alphas of that probe) and nothing else.

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ids = lambda cs: [c.name for c in cs]


def dev(t):
    return t.to(DEV).contiguous()


def host(t):
    return t.detach().double().cpu()


def check(case, what, measured, d32, scale):
    b = R.bound(d32, scale)
    print(f"STAT {case.name} {what}: measured {measured:.3e}, D32 {d32:.3e}, bound {b:.3e}, measured / D32 {measured / max(d32, 1e-300):.3g}")
    assert measured <= b, f"{case.name}: {what} is {measured:.3e} from the float64 reference, bound {b:.3e} (D32 {d32:.3e})"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def prob(name):
    return problem(BY_NAME[name])


# ================================================================================================ Lanczos
@functools.lru_cache(maxsize=None)
def lanczos_refs(name):
    """(Q, diag, off) of the float64 reference — oracle/matfree.py on the rows without breakdown — and of the float32 run"""
    case = BY_NAME[name]
    op, V0 = prob(name)
    k = case.d["k"]
    Q64, d64, o64, steps = R.lanczos_block(op, V0, k, F64)
    if steps == [k] * len(V0):
        mv, _ = op.on(F64)
        outs = [om.tridiag_sym(k)(lambda q: mv(q[None, :])[0], v.double()) for v in V0]
        Q64 = torch.stack([o[0] for o in outs])
        d64 = torch.stack([torch.diagonal(o[1]) for o in outs])
        o64 = torch.stack([torch.diagonal(o[1], 1) for o in outs])
    return (Q64, d64, o64), R.lanczos_block(op, V0, k, F32)[:3], steps


def run_lanczos(op, V0, k):
    mv, _ = op.on(F32, DEV)
    Q, dg, off = K.lanczos_tridiag(mv, dev(V0), k)
    torch.cuda.synchronize() if DEV == "cuda" else None
    return Q, dg, off


def structure(op, Q, dg, off, steps=None):
    """||Q Q^T - I||_max, ||Q A Q^T - T||_max / ||A||, and the worst three-term residual / ||A||, in float64, over the
    live part of every probe: all k rows, or rows 0 .. j of a probe that broke down at step j (-1: a zero start row,
    nothing live); at the step of a breakdown the three-term residual is what the guard judged negligible"""
    mv, _ = op.on(F64)
    nA = op.norm()
    Q, dg, off = host(Q), host(dg), host(off)
    k = Q.shape[1]
    orth = coup = res = 0.0
    for p in range(Q.shape[0]):
        L = k if steps is None else min(steps[p] + 1, k)
        if L == 0:
            continue
        Qp, dp, op_ = Q[p, :L], dg[p, :L], off[p, :L - 1]
        AQ = mv(Qp)
        orth = max(orth, R.maxabs(Qp @ Qp.T, torch.eye(L, dtype=F64)))
        coup = max(coup, R.maxabs(Qp @ AQ.T, R.tridiag(dp, op_)) / nA)
        for j in range(L if L < k else L - 1):
            r = AQ[j] - dp[j] * Qp[j] - (op_[j] * Qp[j + 1] if j + 1 < L else 0.0) - (op_[j - 1] * Qp[j - 1] if j else 0.0)
            res = max(res, float(r.norm()) / nA)
    return dict(orthogonality=orth, projection=coup, three_term=res)


def check_structure(case, op, got, ref32, steps=None):
    s, s32 = structure(op, *got, steps=steps), structure(op, *ref32, steps=steps)
    for key in s:
        check(case, key, s[key], s32[key], 1.0)


@pytest.mark.parametrize("case", group("elementwise"), ids=ids(group("elementwise")))
def test_lanczos_elementwise(case):
    op, V0 = prob(case.name)
    k, N = case.d["k"], case.d["N"]
    (Q64, d64, o64), (Q32, d32, o32), _ = lanczos_refs(case.name)
    Q, dg, off = run_lanczos(op, V0, k)
    assert Q.shape == (len(V0), k, N) and dg.shape == (len(V0), k) and off.shape == (len(V0), max(k - 1, 0))
    assert bool((off >= 0).all())                    # the sign convention that fixes the rows of Q
    nA = op.norm()
    check(case, "diag", R.maxabs(host(dg), d64), R.maxabs(d32, d64), nA)
    check(case, "off", R.maxabs(host(off), o64), R.maxabs(o32, o64), nA)
    check(case, "Q", R.maxabs(host(Q), Q64), R.maxabs(Q32, Q64), 1.0)
    assert Q.ldq == (N + 3) // 4 * 4 and Q.basis_buffer.shape == (len(V0), k, Q.ldq)
    assert not Q.basis_buffer[:, :, N:].any(), "padding columns of the basis beyond N are not zero"
    check_structure(case, op, (Q, dg, off), (Q32, d32, o32))


@pytest.mark.parametrize("case", group("full"), ids=ids(group("full")))
def test_lanczos_full_depth(case):
    op, V0 = prob(case.name)
    k = case.d["k"]
    _, (Q32, d32, o32), _ = lanczos_refs(case.name)
    Q, dg, off = run_lanczos(op, V0, k)
    ev = torch.linalg.eigvalsh(op.dense())
    eigs = lambda d, o: torch.linalg.eigvalsh(R.tridiag(host(d), host(o)))
    check(case, "eig(T) - eig(A)", R.maxabs(eigs(dg, off), ev[None, :].expand(len(V0), -1)),
          R.maxabs(eigs(d32, o32), ev[None, :].expand(len(V0), -1)), op.norm())
    check_structure(case, op, (Q, dg, off), (Q32, d32, o32))      # Q is square: orthogonality is Q Q^T = I


@pytest.mark.parametrize("case", group("breakdown"), ids=ids(group("breakdown")))
def test_lanczos_breakdown(case):
    op, V0 = prob(case.name)
    k, steps = case.d["k"], case.d["steps"]
    (Q64, d64, o64), (Q32, d32, o32), steps64 = lanczos_refs(case.name)
    assert steps64 == steps
    Q, dg, off = run_lanczos(op, V0, k)
    nA = op.norm()
    for p, j in enumerate(steps):
        assert not off[p, j:].any(), f"probe {p}: off[{j}:] = {off[p, j:].tolist()}"
        assert bool((off[p, :j] > 0).all())
        assert bool((dg[p, j + 1:] == 1).all()), f"probe {p}: diag[{j + 1}:] = {dg[p, j + 1:].tolist()}"
        assert not Q[p, j + 1:].any(), f"probe {p}: basis rows from {j + 1} on are not zero"
        # the live part against the float64 recurrence
        check(case, f"diag[{p}]", R.maxabs(host(dg[p, :j + 1]), d64[p, :j + 1]), R.maxabs(d32[p, :j + 1], d64[p, :j + 1]), nA)
        check(case, f"off[{p}]", R.maxabs(host(off[p, :j]), o64[p, :j]), R.maxabs(o32[p, :j], o64[p, :j]), nA)
        check(case, f"Q[{p}]", R.maxabs(host(Q[p, :j + 1]), Q64[p, :j + 1]), R.maxabs(Q32[p, :j + 1], Q64[p, :j + 1]), 1.0)
    check(case, "diag[2, 0] - lam", abs(float(dg[2, 0]) - 0.5), abs(float(d32[2, 0]) - 0.5), nA)
    check_structure(case, op, (Q, dg, off), (Q32, d32, o32), steps)
    # every probe is its own P = 1 run (a slice of the block: the same alignment)
    mv, _ = op.on(F32, DEV)
    Vd = dev(V0)
    for p in range(len(V0)):
        Q1, d1, o1 = K.lanczos_tridiag(mv, Vd[p:p + 1], k)
        assert same_bits(d1[0], dg[p]) and same_bits(o1[0], off[p]) and same_bits(Q1[0], Q[p]), f"probe {p} differs from its P = 1 run"
    # f(A) b is exact through the guard
    f = FUNS["invsqrt"]
    got = K.funm_lanczos_sym(K.dense_funm_sym_eigh(f), k)(mv, Vd)
    want = R.funm_exact(op, V0, f)
    f32 = R.funm_from_lanczos(Q32, d32, o32, V0.norm(dim=1), f)
    check(case, "f(A) b", R.maxabs(host(got), want), R.maxabs(f32, want), float(want.abs().max()))


@pytest.mark.parametrize("case", group("zero_row"), ids=ids(group("zero_row")))
def test_lanczos_zero_start_row(case):
    op, V0 = prob(case.name)
    k, z = case.d["k"], case.d["zero"]
    assert not V0[z].any()
    Q, dg, off = run_lanczos(op, V0, k)
    assert bool(torch.isfinite(Q).all()) and bool(torch.isfinite(dg).all()) and bool(torch.isfinite(off).all())
    assert not Q[z].any() and bool((dg[z] == 1).all()) and not off[z].any()
    mv, _ = op.on(F32, DEV)
    f = FUNS["invsqrt"]
    est = K.funm_lanczos_sym(K.dense_funm_sym_eigh(f), k)
    out = est(mv, dev(V0))
    assert bool(torch.isfinite(out).all()) and not out[z].any()
    others = [p for p in range(len(V0)) if p != z]
    if z == len(V0) - 1:                             # the block without it
        Vw, rows = V0[:z], others
    else:                                            # the block with another, non-zero row in its place
        Vw, rows = V0.clone(), others
        Vw[z] = V0[others[0]].flip(0)
    Qw, dw, ow = run_lanczos(op, Vw, k)
    outw = est(mv, dev(Vw))
    for p in rows:
        assert same_bits(Qw[p], Q[p]) and same_bits(dw[p], dg[p]) and same_bits(ow[p], off[p]), f"probe {p} changed with the zero row"
        assert same_bits(outw[p], out[p])
    (Q64, d64, o64), (Q32, d32, o32), _ = lanczos_refs(case.name)
    check(case, "diag", R.maxabs(host(dg), d64), R.maxabs(d32, d64), op.norm())
    check(case, "Q", R.maxabs(host(Q), Q64), R.maxabs(Q32, Q64), 1.0)
    check_structure(case, op, (Q, dg, off), (Q32, d32, o32), [-1 if p == z else k for p in range(len(V0))])
    want = R.funm_exact(op, V0, f)
    check(case, "f(A) b", R.maxabs(host(out), R.funm_from_lanczos(Q64, d64, o64, V0.double().norm(dim=1), f)),
          R.maxabs(R.funm_from_lanczos(Q32, d32, o32, V0.norm(dim=1), f), R.funm_from_lanczos(Q64, d64, o64, V0.double().norm(dim=1), f)),
          float(want.abs().max()))


@pytest.mark.parametrize("case", group("scaling"), ids=ids(group("scaling")))
def test_lanczos_power_of_two_scaling(case):
    op, V0 = prob(case.name)
    k = case.d["k"]
    steps = case.d.get("steps", [k] * len(V0))
    Q, dg, off = run_lanczos(op, V0, k)
    check_structure(case, op, (Q, dg, off), lanczos_refs(case.name)[1], steps)
    for s in (2.0 ** -20, 2.0 ** 20):
        Qs, ds, os_ = run_lanczos(op.scaled(s), V0, k)
        assert same_bits(Qs, Q), f"scale {s}: the basis changed"
        for p, j in enumerate(steps):
            assert torch.equal(ds[p, :j + 1], dg[p, :j + 1] * s) and torch.equal(os_[p], off[p] * s), f"scale {s}, probe {p}"
            assert bool((ds[p, j + 1:] == 1).all())


@pytest.mark.parametrize("case", group("funm"), ids=ids(group("funm")))
def test_funm_lanczos_sym(case):
    op, V0 = prob(case.name)
    d = case.d
    f = FUNS[d["f"]]
    mv, _ = op.on(F32, DEV)
    got = K.funm_lanczos_sym(K.dense_funm_sym_eigh(f, clip_min=d.get("clip_min"), floor=d.get("floor")), d["k"])(mv, dev(V0))
    want = R.funm_exact(op, V0, f, d.get("floor"), d.get("clip_min"))
    (_, _, _), (Q32, d32, o32), steps = lanczos_refs(case.name)
    assert steps == d.get("steps", [d["k"]] * len(V0))
    f32 = R.funm_from_lanczos(Q32, d32, o32, V0.norm(dim=1), f, d.get("floor"), d.get("clip_min"))
    check(case, "f(A) b", R.maxabs(host(got), want), R.maxabs(f32, want), float(want.abs().max()))


@pytest.mark.parametrize("case", group("funm_dense"), ids=ids(group("funm_dense")))
def test_funm_lanczos_dense(case):
    """the float64 twin on the device against the float64 recurrence of the same depth on the CPU, on every row, within
    4 N 2^-53 scale (N 2^-53: the ceiling of a length-N float64 sum); rows whose recurrence is exact (full depth, or
    through the breakdown guard) also against f(A) b from eigh, within max(8 D64, 4 N 2^-53 scale) with D64 the distance
    of the CPU recurrence from that answer"""
    op, V0 = prob(case.name)
    d = case.d
    f = FUNS[d["f"]]
    A = op.dense()
    got = K.funm_lanczos_dense(K.dense_funm_sym_eigh(f), d["k"])(A.to(DEV), V0.double().to(DEV))
    assert got.dtype == F64 and bool(torch.isfinite(got).all())
    want = R.funm_exact(op, V0, f)
    Q64, d64, o64, _ = R.lanczos_block(op, V0, min(d["k"], d["N"]), F64)
    rec = R.funm_from_lanczos(Q64, d64, o64, V0.double().norm(dim=1), f)
    scale = float(want.abs().max())
    floor = 4 * d["N"] * 2.0 ** -53 * scale
    m = R.maxabs(host(got), rec)
    print(f"STAT {case.name} f(A) b - float64 recurrence: measured {m:.3e}, bound {floor:.3e}")
    assert m <= floor
    if d.get("exact"):
        D64, m = R.maxabs(rec, want), R.maxabs(host(got), want)
        print(f"STAT {case.name} f(A) b - exact (float64): measured {m:.3e}, D64 {D64:.3e}, bound {max(8 * D64, floor):.3e}")
        assert m <= max(8 * D64, floor)
    if "zero" in d:
        assert not got[d["zero"]].any()


# ================================================================================================ CG
@functools.lru_cache(maxsize=None)
def cg_refs(name):
    case = BY_NAME[name]
    op, B = prob(name)
    kw = cg_kwargs(case, B)
    mv, _ = op.on(F64)
    X64 = torch.stack([om.cg(lambda v: mv(v[None, :])[0], b.double(), **kw)[0] for b in B])     # the oracle's loop
    _, it64, infos64 = R.cg_block(op, B, F64, **kw)
    X32, it32, infos32 = R.cg_block(op, B, F32, **kw)
    # rows whose stop is no close call: the float32 residual parts from the float64 one by delta (relative) over the last
    # two steps, and the threshold lies more than 8 delta from either — the margin of the D32 rule, on the decision
    thr = [max(kw["tol"] * float(b.double().norm()), kw.get("atol", 0.0)) for b in B]
    clear = []
    for h64, h32, n64, n32, t in zip((i["hist"] for i in infos64), (i["hist"] for i in infos32), it64, it32, thr):
        if n64 != n32 or n64 in (0, kw.get("maxiter")) or h64[-1] == 0.0:
            clear.append(n64 == n32)
            continue
        delta = max(abs(a - b) / b for a, b in zip(h32[-2:], h64[-2:]))
        clear.append(h64[-1] * (1 + 8 * delta) < t < h64[-2] * (1 - 8 * delta))
    print(f"STAT {name}: rows whose stop is clear of the threshold {clear}")
    return kw, X64, (it64, clear), X32, (it32, [i["hist"][-1] for i in infos32])


def true_residual(op, X, B):
    """||b - A x|| per row, the product through the float32 operator on the device, the rest in float64"""
    mv, _ = op.on(F32, DEV)
    return (host(B) - host(mv(dev(X)))).norm(dim=1)


def check_cg_solution(case, op, B, X, info, X64, X32, stops, stops32):
    (it64, clear), (it32, rec32) = stops, stops32
    ex = R.solve_exact(op, B)
    for p in range(len(B)):
        check(case, f"X[{p}] - exact", R.maxabs(host(X[p]), ex[p]), R.maxabs(X32[p], ex[p]), float(ex[p].norm()))
        # the iterate itself against the oracle's loop in float64, at the float32 run's distance from it, where both
        # precisions stop at the same step and the stop is not a close call (a step more or less moves x by the
        # truncation error, far above rounding)
        if clear[p]:
            check(case, f"X[{p}] - float64 iterate", R.maxabs(host(X[p]), X64[p]), R.maxabs(X32[p], X64[p]), float(ex[p].norm()))
        else:
            print(f"STAT {case.name} X[{p}]: the stop is a close call, not compared with the float64 iterate")
    assert abs(info["iterations"] - max(it64)) <= case.allow, f"{info['iterations']} iterations, float64 {max(it64)}"
    print(f"STAT {case.name} iterations: {info['iterations']}, float64 {it64}")
    # the recurrence residual the driver reports against b - A x recomputed in float64: the two drift apart by the
    # rounding of the updates, and the float32 run on the CPU shows by how much
    mv64, _ = op.on(F64)
    tr = true_residual(op, X, B)
    rn = host(info["residual_norm"])
    for p in range(len(B)):
        d32 = abs(rec32[p] - float((B[p].double() - mv64(X32[p].double()[None, :])[0]).norm()))
        check(case, f"residual_norm[{p}]", abs(float(rn[p]) - float(tr[p])), d32, float(B[p].norm()))


@pytest.mark.parametrize("case", group("cg"), ids=ids(group("cg")))
def test_cg(case):
    op, B = prob(case.name)
    kw, X64, stops, X32, stops32 = cg_refs(case.name)
    mv, _ = op.on(F32, DEV)
    X, info = K.cg(mv, dev(B), **kw)
    assert bool(torch.isfinite(X).all())
    check_cg_solution(case, op, B, X, info, X64, X32, stops, stops32)
    if "atol" in kw:
        assert bool((info["residual_norm"] <= kw["atol"]).all()) and kw["atol"] > kw["tol"] * float(B.norm(dim=1).max())


@pytest.mark.parametrize("case", group("cg_frozen"), ids=ids(group("cg_frozen")))
def test_cg_frozen_row(case):
    op, B = prob(case.name)
    kw, X64, stops, X32, stops32 = cg_refs(case.name)
    sp = case.d["special"]
    assert sp == len(B) - 1
    mv, _ = op.on(F32, DEV)
    Bd = dev(B)
    X, info = K.cg(mv, Bd, **kw)
    assert bool(torch.isfinite(X).all()) and bool(torch.isfinite(info["residual_norm"]).all())
    check_cg_solution(case, op, B, X, info, X64, X32, stops, stops32)
    X1, info1 = K.cg(mv, Bd[sp:sp + 1], **kw)
    assert info1["iterations"] == stops[0][sp] <= 1
    assert same_bits(X1[0], X[sp]), "the frozen row drifted while the others ran on"
    if not B[sp].any():
        assert not X[sp].any() and float(info["residual_norm"][sp]) == 0.0
    Xo, infoo = K.cg(mv, Bd[:sp], **kw)
    assert same_bits(Xo, X[:sp]) and infoo["iterations"] == info["iterations"], "the other rows changed with the special one"


@pytest.mark.parametrize("case", group("cg_x0"), ids=ids(group("cg_x0")))
def test_cg_x0(case):
    op, B = prob(case.name)
    kw, X64, stops, X32, stops32 = cg_refs(case.name)
    mv, _ = op.on(F32, DEV)
    ex = R.solve_exact(op, B)
    if case.d["x0"] == "exact":
        x0 = dev(ex.float())
        X, info = K.cg(mv, dev(B), x0=x0, **kw)
        assert info["iterations"] == 0 and same_bits(X, x0) and X.data_ptr() != x0.data_ptr()
        return
    x0 = torch.randn(B.shape, generator=torch.Generator().manual_seed(5), dtype=F64).float()
    X, info = K.cg(mv, dev(B), x0=dev(x0), **kw)
    X32r, it32r, _ = R.cg_block(op, B, F32, X0=x0, **kw)
    _, it64r, _ = R.cg_block(op, B, F64, X0=x0, **kw)
    assert all(abs(a - b) <= case.allow for a, b in zip(it32r, it64r))
    assert abs(info["iterations"] - max(it64r)) <= case.allow
    Xn, _ = K.cg(mv, dev(B), **kw)
    for p in range(len(B)):
        check(case, f"X[{p}] - exact", R.maxabs(host(X[p]), ex[p]), R.maxabs(X32r[p], ex[p]), float(ex[p].norm()))
        check(case, f"X[{p}] - X without x0", R.maxabs(host(X[p]), host(Xn[p])), R.maxabs(X32r[p], X32[p]), float(ex[p].norm()))


@pytest.mark.parametrize("case", group("cg_maxiter"), ids=ids(group("cg_maxiter")))
def test_cg_maxiter(case):
    op, B = prob(case.name)
    kw, X64, stops, X32, stops32 = cg_refs(case.name)
    mv, _ = op.on(F32, DEV)
    X, info = K.cg(mv, dev(B), **kw)
    assert info["iterations"] == kw["maxiter"] <= 5
    for p in range(len(B)):
        check(case, f"X[{p}] after {kw['maxiter']} steps", R.maxabs(host(X[p]), X64[p]), R.maxabs(X32[p], X64[p]), float(X64[p].norm()))


@pytest.mark.parametrize("case", group("cg_check"), ids=ids(group("cg_check")))
def test_cg_check_every(case):
    op, B = prob(case.name)
    kw, *_ = cg_refs(case.name)
    mv, _ = op.on(F32, DEV)
    X1, info1 = K.cg(mv, dev(B), **kw)
    ce = case.d["check_every"]
    Xc, infoc = K.cg(mv, dev(B), check_every=ce, **kw)
    assert same_bits(Xc, X1), "check_every changed the answer"
    assert same_bits(infoc["residual_norm"], info1["residual_norm"])
    assert infoc["iterations"] == -(-info1["iterations"] // ce) * ce
    print(f"STAT {case.name}: iterations {info1['iterations']} -> {infoc['iterations']}")


def test_cg_stall():
    """the reference run is that on the same rounded operator; its plateau steps are asserted in the CPU file"""
    case = BY_NAME["cg/stall"]
    op, B = prob(case.name)
    d = case.d
    mv, _ = op.on(F32, DEV)
    X, info = K.cg(mv, dev(B), tol=d["tol"], maxiter=d["maxiter"])
    assert info["iterations"] == d["maxiter"]
    _, _, infos = R.cg_block(op, B, F32, tol=d["tol"], maxiter=d["maxiter"], keep=True)
    plateaus = [R.plateau_step(i["hist"], d["stall"]) for i in infos]
    Xs, info_s = K.cg(mv, dev(B), tol=d["tol"], maxiter=d["maxiter"], stall=d["stall"])
    print(f"STAT {case.name}: stall={d['stall']} stops at {info_s['iterations']}, the reference stops improving at {plateaus}")
    assert abs(info_s["iterations"] - max(plateaus)) <= d["stall"]
    # every row is frozen where it stalled: the iterate of the reference run on the same operator at its stop
    _, _, infos64 = R.cg_block(op, B, F64, tol=d["tol"], maxiter=d["maxiter"], keep=True)
    for p, t in enumerate(d["stops"]):
        x64, x32 = infos64[p]["xs"][t], infos[p]["xs"][t]
        check(case, f"X[{p}] at step {t}", R.maxabs(host(Xs[p]), x64), R.maxabs(x32, x64), float(x64.norm()))


def test_cg_keep_best():
    case = BY_NAME["cg/keep_best"]
    op, B = prob(case.name)
    d = case.d
    mv, _ = op.on(F32, DEV)
    Xb, info = K.cg(mv, dev(B), tol=d["tol"], maxiter=d["maxiter"], stall=d["stall"], keep_best=True)
    it = info["iterations"]
    assert it < d["maxiter"]
    tb = true_residual(op, Xb, B)
    rn = host(info["residual_norm"])
    plain = [true_residual(op, K.cg(mv, dev(B), tol=d["tol"], maxiter=t)[0], B) for t in range(it + 1)]
    _, _, infos = R.cg_block(op, B, F32, tol=d["tol"], maxiter=d["maxiter"], keep=True)
    for p in range(len(B)):
        stop, kept = R.keep_best_walk(infos[p]["true"], d["stall"])
        print(f"STAT {case.name} row {p}: stopped by {it}, residual {float(rn[p]):.4e} (recomputed {float(tb[p]):.4e}); the plain "
              f"run's {[round(float(t[p]), 4) for t in plain]}; the reference keeps iterate {kept} and stops at {stop}")
        # the residual reported is that of the iterate returned (one float32 bdot apart: 4 x 2^-24 relative)
        assert abs(float(rn[p]) - float(tb[p])) <= 4 * R.U24 * float(tb[p])
        # ... and no iterate of the plain run up to the row's stop has a smaller one (the choice is made on float32 sums)
        assert all(float(tb[p]) <= float(t[p]) * (1 + 8 * R.U24) for t in plain[: min(stop, it) + 1])
        # ... while the last one is clearly worse: the best iterate is not the last
        assert float(tb[p]) < 0.9 * float(plain[min(stop, it)][p])
    assert abs(it - max(R.keep_best_walk(i["true"], d["stall"])[0] for i in infos)) <= d["stall"]


def test_cg_dense():
    case = BY_NAME["cgd/mixed"]
    op, B = prob(case.name)
    A = op.dense()
    X, info = K.cg_dense(A.to(DEV), B.double().to(DEV))
    assert X.dtype == F64 and bool(torch.isfinite(X).all())
    ex = R.solve_exact(op, B)
    X64, it64, _ = R.cg_block(op, B, F64)
    assert not X[1].any() and float(info["residual_norm"][1]) == 0.0
    assert abs(info["iterations"] - max(it64)) <= case.allow and it64[2] <= 2 < min(it64[0], it64[3])
    for p in range(len(B)):
        D64 = R.maxabs(X64[p], ex[p])
        m = R.maxabs(host(X[p]), ex[p])
        print(f"STAT {case.name} X[{p}] - exact (float64): measured {m:.3e}, D64 {D64:.3e}")
        assert m <= max(8 * D64, 4 * case.d["N"] * 2.0 ** -53 * float(ex[p].norm()))
        # D64 is the truncation error of the stopping rule: the iterate itself against the CPU float64 loop, one
        # length-N float64 sum's ceiling per step
        mi, bi = R.maxabs(host(X[p]), X64[p]), 4 * max(it64) * case.d["N"] * 2.0 ** -53 * float(ex[p].norm())
        print(f"STAT {case.name} X[{p}] - float64 iterate (float64): measured {mi:.3e}, bound {bi:.3e}")
        assert mi <= bi
    # the recurrence residual against b - A x: apart by the rounding of the updates, 2^-53 ||A|| ||x|| per step
    tr = (B.double() - host(X) @ A).norm(dim=1)
    assert R.maxabs(host(info["residual_norm"]), tr) <= 4 * info["iterations"] * 2.0 ** -53 * op.norm() * float(ex.norm())


# ================================================================================================ Golub-Kahan
@functools.lru_cache(maxsize=None)
def bidiag_refs(name):
    case = BY_NAME[name]
    op, V0 = prob(name)
    k = case.d["k"]
    mv, vm = op.on(F64)
    outs = [om.bidiag(k)(lambda q: mv(q[None, :])[0], lambda q: vm(q[None, :])[0], v.double()) for v in V0]
    U64, V64 = torch.stack([o[0] for o in outs]), torch.stack([o[2] for o in outs])
    a64 = torch.stack([torch.diagonal(o[1]) for o in outs])
    b64 = torch.stack([torch.diagonal(o[1], 1) for o in outs])
    return (a64, b64, V64, U64), R.bidiag_block(op, V0, k, F32)


def run_bidiag(op, V0, k, n_out, bases=True):
    mv, vm = op.on(F32, DEV)
    return K.bidiag(mv, vm, dev(V0), k, n_out, return_bases=bases)


def bidiag_structure(op, al, be, V, U, co):
    """orthogonality of both bases, the two recurrences, and the coefficient arrays against the projections they are"""
    A = op.dense()
    nA = op.norm()
    al, be, V, U = host(al), host(be), host(V), host(U)
    cu, cv = host(co[0]) + host(co[1]), host(co[2]) + host(co[3])
    out = dict(orth_U=0.0, orth_V=0.0, rec_Av=0.0, rec_Atu=0.0, cu=0.0, cv=0.0, second_pass=0.0)
    for p in range(V.shape[0]):
        k = V.shape[1]
        eye = torch.eye(k, dtype=F64)
        out["orth_U"] = max(out["orth_U"], R.maxabs(U[p] @ U[p].T, eye))
        out["orth_V"] = max(out["orth_V"], R.maxabs(V[p] @ V[p].T, eye))
        AV, AtU = V[p] @ A.T, U[p] @ A
        for j in range(k):
            r = AV[j] - al[p, j] * U[p, j] - (be[p, j - 1] * U[p, j - 1] if j else 0.0)
            out["rec_Av"] = max(out["rec_Av"], float(r.norm()) / nA)
            out["cu"] = max(out["cu"], R.maxabs(cu[p, j, :j], U[p, :j] @ AV[j]) / nA)
            if j + 1 < k:
                r = AtU[j] - al[p, j] * V[p, j] - be[p, j] * V[p, j + 1]
                out["rec_Atu"] = max(out["rec_Atu"], float(r.norm()) / nA)
                out["cv"] = max(out["cv"], R.maxabs(cv[p, j, :j + 1], V[p, :j + 1] @ AtU[j]) / nA)
    out["second_pass"] = max(float(host(co[1]).abs().max()), float(host(co[3]).abs().max())) / nA
    return out


@pytest.mark.parametrize("case", group("bidiag"), ids=ids(group("bidiag")))
def test_bidiag(case):
    op, V0 = prob(case.name)
    k, N, n_out = case.d["k"], case.d["N"], case.d["n_out"]
    (a64, b64, V64, U64), (a32, b32, V32, U32, co32) = bidiag_refs(case.name)
    al, be, V, U, co = run_bidiag(op, V0, k, n_out)
    assert V.shape == (len(V0), k, N) and U.shape == (len(V0), k, n_out) and all(c.shape == (len(V0), k, k) for c in co)
    nA = op.norm()
    check(case, "alphas", R.maxabs(host(al), a64), R.maxabs(a32, a64), nA)
    check(case, "betas", R.maxabs(host(be), b64), R.maxabs(b32, b64), nA)
    check(case, "V", R.maxabs(host(V), V64), R.maxabs(V32, V64), 1.0)
    check(case, "U", R.maxabs(host(U), U64), R.maxabs(U32, U64), 1.0)
    al2, be2 = run_bidiag(op, V0, k, n_out, bases=False)
    check(case, "alphas without bases", R.maxabs(host(al2), a64), R.maxabs(a32, a64), nA)
    check(case, "betas without bases", R.maxabs(host(be2), b64), R.maxabs(b32, b64), nA)
    s, s32 = bidiag_structure(op, al, be, V, U, co), bidiag_structure(op, a32, b32, V32, U32, co32)
    for key in s:
        check(case, key, s[key], s32[key], 1.0)
    for j in range(k):                               # strict triangular support
        assert not co[0][:, j, j:].any() and not co[1][:, j, j:].any()
        assert not co[2][:, j, j + 1:].any() and not co[3][:, j, j + 1:].any()


@pytest.mark.parametrize("case", group("slq"), ids=ids(group("slq")))
def test_slq_logdet_product(case):
    op, V0 = prob(case.name)
    k, n_out = case.d["k"], case.d["n_out"]
    mv, vm = op.on(F32, DEV)
    got = K.slq_logdet_product(mv, vm, dev(V0), k, n_out)
    assert got.dtype == F64 and got.shape == (len(V0),)
    (a64, b64, _, _), (a32, b32, *_) = bidiag_refs(case.name)
    l2 = (V0.double() ** 2).sum(1)
    ref = R.slq_exact(op, V0) if k == case.d["N"] else R.slq_from_bidiag(a64, b64, l2)
    check(case, "quadrature", R.maxabs(host(got), ref), R.maxabs(R.slq_from_bidiag(a32, b32, l2), ref), float(ref.abs().max()))
    al, be = run_bidiag(op, V0, k, n_out, bases=False)
    assert be.shape == (len(V0), max(k - 1, 0))
    check(case, "alphas", R.maxabs(host(al), a64), R.maxabs(a32, a64), op.norm())


@pytest.mark.parametrize("case", group("bd_zero"), ids=ids(group("bd_zero")))
def test_bidiag_zero_start_row(case):
    op, V0 = prob(case.name)
    k, n_out, z = case.d["k"], case.d["n_out"], case.d["zero"]
    al, be, V, U, co = run_bidiag(op, V0, k, n_out)
    for t in (al, be, V, U) + tuple(co):
        assert bool(torch.isfinite(t).all()), "a zero start row made the output non-finite"
    assert not V[z].any() and not U[z].any()
    mv, vm = op.on(F32, DEV)
    q = K.slq_logdet_product(mv, vm, dev(V0), k, n_out)
    assert bool(torch.isfinite(q).all()) and float(q[z]) == 0.0
    others = [p for p in range(len(V0)) if p != z]
    if z == len(V0) - 1:
        Vw = V0[:z]
    else:
        Vw = V0.clone()
        Vw[z] = V0[others[0]].flip(0)
    alw, bew, Vv, Uw, cow = run_bidiag(op, Vw, k, n_out)
    qw = K.slq_logdet_product(mv, vm, dev(Vw), k, n_out)
    for p in others:
        assert same_bits(alw[p], al[p]) and same_bits(bew[p], be[p]) and same_bits(Vv[p], V[p]) and same_bits(Uw[p], U[p]), \
            f"probe {p} changed with the zero row"
        assert all(same_bits(a[p], b[p]) for a, b in zip(cow, co)) and float(qw[p]) == float(q[p])


# ================================================================================================ the deflation
@functools.lru_cache(maxsize=None)
def deflation(name):
    op, B = prob(name)
    return op, B, K.RangeDeflation(dev(op.t["Qt"]), dev(op.t["lam"]))


def rows_norm(t):
    return host(t).norm(dim=1)


@pytest.mark.parametrize("case", group("df_coeffs"), ids=ids(group("df_coeffs")))
def test_deflation_coeffs(case):
    op, B, defl = deflation(case.name)
    C = defl.coeffs(dev(B))
    assert C.dtype == F64 and C.shape == (len(B), case.d["r"])
    want = B.double() @ op.t["Qt"].double().T
    d32 = R.maxabs(B @ op.t["Qt"].T, want)
    check(case, "coeffs", R.maxabs(host(C), want), d32, float(B.double().norm(dim=1).max()))


def test_deflation_closed_form():
    case = BY_NAME["df/closed_form"]
    op, B, defl = deflation(case.name)
    Qt, lam, al = op.t["Qt"], op.t["lam"], float(op.t["alpha"])
    C64 = B.double() @ Qt.double().T
    for fname in ("invsqrt", "inv"):
        f = FUNS[fname]
        want = R.funm_exact(op, B, f)
        scale = float(want.norm(dim=1).max())
        # the float32 run of the same formula on the CPU
        C32 = B @ Qt.T
        rp32 = (C32 * f(lam)[None, :]) @ Qt
        cf32 = rp32 + float(f(torch.tensor(al, dtype=F64))) * (B - C32 @ Qt)
        rp = defl.range_part(defl.coeffs(dev(B)), f)
        check(case, f"range_part {fname}", R.maxabs(host(rp), (C64 * f(lam.double())[None, :]) @ Qt.double()),
              R.maxabs(rp32, (C64 * f(lam.double())[None, :]) @ Qt.double()), float(B.norm(dim=1).max()))
        got = defl.closed_form(dev(B), f, al)
        check(case, f"closed_form {fname}", R.maxabs(host(got), want), R.maxabs(cf32, want), scale)


def test_deflation_project_out():
    case = BY_NAME["df/project"]
    op, B, defl = deflation(case.name)
    Qt = op.t["Qt"]
    # a block with a range component 200 x its complement, as the products of the deflated operator have
    g = torch.Generator().manual_seed(9)
    V = (B + 200.0 * torch.randn(len(B), case.d["r"], generator=g, dtype=F64).float() @ Qt).contiguous()
    Vd = dev(V)
    o1, o2 = defl.project_out(Vd, passes=1), defl.project_out(Vd, passes=2)
    l1, l2 = (host(o1) @ Qt.double().T).norm(dim=1), (host(o2) @ Qt.double().T).norm(dim=1)
    print(f"STAT {case.name}: ||Q out|| after one pass {l1.tolist()}, after two {l2.tolist()}")
    assert bool((l2 <= l1).all()), "the second projection pass left more of range(Q) than the first"
    p32 = V - (V @ Qt.T) @ Qt
    p64 = V.double() - (V.double() @ Qt.double().T) @ Qt.double()
    scale = float(V.norm(dim=1).max())
    check(case, "project_out", R.maxabs(host(o1), p64), R.maxabs(p32, p64), scale)
    check(case, "project_out passes=2", R.maxabs(host(o2), p64), R.maxabs(p32, p64), scale)
    check(case, "||Q out|| passes=2", float(l2.max()), float((p32.double() @ Qt.double().T).norm(dim=1).max()), scale)
    back = host(o1) + (V.double() @ Qt.double().T) @ Qt.double()
    check(case, "out + Q^T (Q V) - V", R.maxabs(back, V), R.maxabs(p32.double() + (V.double() @ Qt.double().T) @ Qt.double(), V), scale)
    C = defl.coeffs(Vd)
    assert same_bits(defl.project_out(Vd, C=C), o1), "C= differs from the computed coefficients"


def _relres_formula(op, X, B, dtype):
    """the definition of ``relative_residual`` on the CPU: coefficients in float64, the product and the two projected
    blocks in ``dtype``"""
    Qt, lam = op.t["Qt"], op.t["lam"].double()
    mv, _ = op.on(dtype)
    co = lambda V: V.double() @ Qt.double().T
    proj = lambda V: V - (co(V).to(dtype) @ Qt.to(dtype))
    rr = co(X) * lam[None, :] - co(B)
    rp = proj(proj(mv(X.to(dtype)))) - proj(B.to(dtype))
    return torch.sqrt((rr * rr).sum(1) + (rp.double() ** 2).sum(1)) / B.double().norm(dim=1)


def test_deflation_relative_residual():
    case = BY_NAME["df/relres"]
    op, B, defl = deflation(case.name)
    Qt, lam, al = op.t["Qt"].double(), op.t["lam"].double(), float(op.t["alpha"])
    mv, _ = op.on(F32, DEV)
    X = R.solve_exact(op, B)
    bn = B.double().norm(dim=1)
    # a known perturbation in the complement and one in the range, on top of the exact solution
    g = torch.Generator().manual_seed(3)
    Ep = torch.randn(B.shape, generator=g, dtype=F64)
    Ep = Ep - (Ep @ Qt.T) @ Qt
    Ep = 0.5 * Ep / Ep.norm(dim=1, keepdim=True) * X.norm(dim=1, keepdim=True)
    Er = torch.zeros(len(B), len(lam), dtype=F64)
    Er[:, 3] = 0.25 * (B.double() @ Qt.T)[:, 3] / lam[3]
    # rounding x to float32 moves it by 2^-24 ||x|| in every direction, which lam_max multiplies: that IS the rounding
    # level of a residual at this condition number, and the function must report it, not hide it
    apriori = R.U24 * op.norm() * float((X.norm(dim=1) / bn).max())
    for tag, Xq in (("exact solution, rounded", X.float()), ("perturbed", (X + Ep + Er @ Qt).float())):
        want, w32 = _relres_formula(op, Xq, B, F64), _relres_formula(op, Xq, B, F32)
        got = host(defl.relative_residual(mv, dev(Xq), dev(B)))
        print(f"STAT {case.name} {tag}: {got.tolist()}, float64 {want.tolist()}, a-priori rounding level {apriori:.3e}")
        check(case, f"relative_residual ({tag})", R.maxabs(got, want), R.maxabs(w32, want), float(want.max()))
        if tag == "perturbed":
            dX = Xq.double() - X                     # ... which is the residual of the perturbation, lam_k and alpha times its parts
            known = torch.sqrt(((dX @ Qt.T) * lam[None, :]).pow(2).sum(1) + (al * (dX - (dX @ Qt.T) @ Qt)).pow(2).sum(1)) / bn
            assert R.maxabs(want, known) <= 1e-6 * float(known.max()) and float(known.min()) > 0.1
        else:
            assert float(want.max()) <= apriori


def test_cg_deflated():
    case = BY_NAME["df/cg_deflated"]
    op, B, defl = deflation(case.name)
    Qt, lam, al = op.t["Qt"].double(), op.t["lam"].double(), float(op.t["alpha"])
    mv, _ = op.on(F32, DEV)
    calls = [0]

    def counted(V):
        calls[0] += 1
        return mv(V)
    X, info = K.cg_deflated(counted, dev(B), defl, tol=1e-4, maxiter=10)
    it = info["iterations"]
    assert 1 <= it < 10 and calls[0] == 2 * it, f"{calls[0]} products for {it} iterations: keep_best is not the default"
    calls[0] = 0
    _, info_p = K.cg_deflated(counted, dev(B), defl, tol=1e-4, maxiter=10, keep_best=False)
    assert calls[0] == info_p["iterations"]
    want = R.solve_exact(op, B)
    C = B.double() @ Qt.T
    want_sub = (C / lam[None, :]) @ Qt + (B.double() - C @ Qt) / al      # the same in the two invariant subspaces
    scale = float(want.norm(dim=1).max())
    x32 = ((B @ Qt.float().T) / lam.float()[None, :]) @ Qt.float() + (B - (B @ Qt.float().T) @ Qt.float()) / al
    d32 = R.maxabs(x32, want_sub)
    err = R.maxabs(host(X), want_sub)
    print(f"STAT {case.name}: {it} iterations, forward error {err:.3e} of {scale:.3e}, exact solve - subspace form {R.maxabs(want, want_sub):.3e}")
    # the complement solve stops at tol = 1e-4 of ||b_perp||: that much of ||x|| on top of the float32 formula's own error
    assert err <= R.bound(d32, scale) + 8 * 1e-4 * scale
    # result orthogonality: the complement part of the answer has no range component left
    Xperp = host(X) - ((C / lam[None, :]) @ Qt)
    leak = float((Xperp @ Qt.T).norm(dim=1).max())
    leak32 = float(((x32.double() - ((C / lam[None, :]) @ Qt)) @ Qt.T).norm(dim=1).max())
    check(case, "range component of the complement part", leak, leak32, scale)


def test_deflation_switches_winograd_off_and_restores_it():
    case = BY_NAME["df/wrap"]
    op, B, defl = deflation(case.name)
    lib = nv.load()
    mv, _ = op.on(F32, DEV)
    before = lib.lip_get_winograd()
    seen = []

    def spy(V):
        seen.append(lib.lip_get_winograd())
        return mv(V)

    def broken(V):
        seen.append(lib.lip_get_winograd())
        raise RuntimeError("product failed")
    try:
        for mode in (1, 0, before):
            nv.check(lib.lip_set_winograd(mode), "lip_set_winograd")
            seen.clear()
            defl.wrap(spy)(dev(B))
            assert seen == [0] and lib.lip_get_winograd() == mode
            seen.clear()
            defl.relative_residual(spy, dev(B), dev(B))
            assert seen == [0] and lib.lip_get_winograd() == mode
            for call in (lambda: defl.wrap(broken)(dev(B)), lambda: defl.relative_residual(broken, dev(B), dev(B))):
                seen.clear()
                with pytest.raises(RuntimeError, match="product failed"):
                    call()
                assert seen == [0] and lib.lip_get_winograd() == mode
    finally:
        lib.lip_set_winograd(before)


# ================================================================================================ gram_orthonormalize
@pytest.mark.parametrize("case", group("gram"), ids=ids(group("gram")))
def test_gram_orthonormalize(case):
    s, N = case.d["s"], case.d["N"]
    Y = torch.randn(s, N, generator=torch.Generator().manual_seed(21), dtype=F64).float()
    Y = (Y * torch.logspace(0, 2, s, dtype=F64).float()[:, None]).contiguous()        # rows over two decades
    Q, T = K.gram_orthonormalize(dev(Y), return_transform=True)
    assert Q.dtype == F32 and T.dtype == F64 and Q.shape == (s, N) and T.shape == (s, s)
    assert K.gram_orthonormalize(dev(Y)).shape == (s, N)
    Qh, Th = host(Q), host(T)
    # the float32 run of the same map on the CPU: Q = T Y with float32 coefficients and sums
    Q32 = Th.float() @ Y
    eye = torch.eye(s, dtype=F64)
    check(case, "T Y - Q", R.maxabs(Th @ Y.double(), Qh), R.maxabs(Q32, Th @ Y.double()), float(Qh.abs().max()))
    check(case, "Q Q^T - I", R.maxabs(Qh @ Qh.T, eye), R.maxabs(Q32.double() @ Q32.double().T, eye), 1.0)
    # same span: Y projected on the rows of Q reproduces Y
    back = lambda q: (Y.double() @ q.T) @ q
    check(case, "Y Q^T Q - Y", R.maxabs(back(Qh), Y), R.maxabs(back(Q32.double()), Y), float(Y.abs().max()))


def test_gram_orthonormalize_zero():
    case = BY_NAME["go/zero"]
    s, N = case.d["s"], case.d["N"]
    Y = torch.zeros(s, N, device=DEV)
    Q, T = K.gram_orthonormalize(Y, return_transform=True)
    assert Q.shape == (0, N) and Q.dtype == F32 and T.shape == (0, s) and T.dtype == F64
    assert K.gram_orthonormalize(Y).shape == (0, N)


def test_every_row_is_run():
    """every row of the table is consumed by a test of this module: as a parameter, or by name"""
    import inspect
    import re
    import sys
    me = sys.modules[__name__]
    run = set(re.findall(r'BY_NAME\["([^"]+)"\]', inspect.getsource(me)))
    for name, fn in vars(me).items():
        if name.startswith("test_") and callable(fn):
            for mark in getattr(fn, "pytestmark", []):
                if mark.name == "parametrize" and mark.args[0] == "case":
                    run |= {c.name for c in mark.args[1]}
    assert run == {c.name for c in CASES}, sorted({c.name for c in CASES} ^ run)


# ---------------------------------------------------------------------------------------------- measured on an MI355X
# Every floating-point quantity asserted above, as one run on an MI355X printed it: row and quantity, the measured distance
# from the float64 reference, D32 (D64 for the float64 twins; '-' where the bound has no such term) and the bound it is held to.
MEASURED = """
lz/well              diag                                          1.198e-07   9.868e-08   7.894e-07
lz/well              off                                           3.409e-08   5.281e-08   4.768e-07
lz/well              Q                                             7.339e-07   7.018e-07   5.615e-06
lz/well              orthogonality                                 1.362e-07   2.783e-07   2.227e-06
lz/well              projection                                    1.288e-07   2.060e-07   1.648e-06
lz/well              three_term                                    5.501e-08   6.612e-08   5.290e-07
lz/well_1030         diag                                          6.769e-08   9.846e-08   7.877e-07
lz/well_1030         off                                           3.021e-08   2.399e-08   4.768e-07
lz/well_1030         Q                                             3.249e-07   6.378e-07   5.102e-06
lz/well_1030         orthogonality                                 1.441e-07   1.675e-07   1.340e-06
lz/well_1030         projection                                    1.104e-07   1.269e-07   1.015e-06
lz/well_1030         three_term                                    4.825e-08   4.797e-08   3.838e-07
lz/dense37           diag                                          3.570e-07   3.570e-07   2.856e-06
lz/dense37           off                                           6.224e-08   1.337e-07   1.070e-06
lz/dense37           Q                                             1.441e-06   9.382e-07   7.505e-06
lz/dense37           orthogonality                                 1.590e-07   1.047e-07   8.374e-07
lz/dense37           projection                                    8.877e-08   1.228e-07   9.825e-07
lz/dense37           three_term                                    6.627e-08   8.715e-08   6.972e-07
lz/dense24           diag                                          1.353e-07   2.109e-07   1.687e-06
lz/dense24           off                                           1.004e-07   8.988e-08   7.190e-07
lz/dense24           Q                                             5.533e-07   8.074e-07   6.459e-06
lz/dense24           orthogonality                                 1.524e-07   1.157e-07   9.257e-07
lz/dense24           projection                                    1.251e-07   1.431e-07   1.145e-06
lz/dense24           three_term                                    8.221e-08   8.455e-08   6.764e-07
lz/blocks            diag                                          6.950e-08   1.097e-07   8.778e-07
lz/blocks            off                                           2.788e-08   3.727e-08   4.768e-07
lz/blocks            Q                                             1.497e-07   2.593e-07   2.074e-06
lz/blocks            orthogonality                                 1.153e-07   3.828e-07   3.062e-06
lz/blocks            projection                                    1.067e-07   2.674e-07   2.139e-06
lz/blocks            three_term                                    4.609e-08   6.523e-08   5.219e-07
lz/long              diag                                          3.298e-08   2.372e-07   1.898e-06
lz/long              off                                           2.690e-08   1.052e-08   4.768e-07
lz/long              Q                                             3.020e-08   3.276e-08   2.621e-07
lz/long              orthogonality                                 1.484e-07   6.261e-07   5.009e-06
lz/long              projection                                    1.024e-07   4.483e-07   3.586e-06
lz/long              three_term                                    3.695e-08   9.543e-08   7.634e-07
lz/k1                diag                                          5.459e-08   6.462e-08   5.170e-07
lz/k1                off                                           0.000e+00   0.000e+00   4.768e-07
lz/k1                Q                                             7.682e-09   6.562e-09   2.384e-07
lz/k1                orthogonality                                 9.457e-08   8.015e-08   6.412e-07
lz/k1                projection                                    5.996e-08   5.498e-08   4.398e-07
lz/k1                three_term                                    0.000e+00   0.000e+00   2.384e-07
lz/full24            eig(T) - eig(A)                               1.002e-07   8.195e-08   6.556e-07
lz/full24            orthogonality                                 1.391e-07   1.656e-07   1.325e-06
lz/full24            projection                                    1.157e-07   1.461e-07   1.169e-06
lz/full24            three_term                                    9.629e-08   8.548e-08   6.839e-07
lz/full1             eig(T) - eig(A)                               0.000e+00   0.000e+00   2.384e-07
lz/full1             orthogonality                                 0.000e+00   0.000e+00   2.384e-07
lz/full1             projection                                    0.000e+00   0.000e+00   2.384e-07
lz/full1             three_term                                    0.000e+00   0.000e+00   2.384e-07
lz/full2             eig(T) - eig(A)                               1.165e-07   1.075e-07   8.600e-07
lz/full2             orthogonality                                 7.361e-08   1.364e-07   1.091e-06
lz/full2             projection                                    8.282e-08   1.050e-07   8.402e-07
lz/full2             three_term                                    4.482e-08   6.020e-08   4.816e-07
lz/full3             eig(T) - eig(A)                               7.514e-08   9.000e-08   7.200e-07
lz/full3             orthogonality                                 9.946e-08   1.198e-07   9.581e-07
lz/full3             projection                                    1.037e-07   1.014e-07   8.111e-07
lz/full3             three_term                                    3.765e-08   5.601e-08   4.481e-07
lz/breakdown         diag[0]                                       3.316e-07   3.316e-07   2.652e-06
lz/breakdown         off[0]                                        1.052e-07   1.333e-07   2.629e-06
lz/breakdown         Q[0]                                          2.750e-07   3.632e-07   2.906e-06
lz/breakdown         diag[1]                                       3.090e-07   3.090e-07   2.629e-06
lz/breakdown         off[1]                                        3.931e-08   7.990e-08   2.629e-06
lz/breakdown         Q[1]                                          1.127e-07   1.303e-07   1.042e-06
lz/breakdown         diag[2]                                       2.980e-08   2.980e-08   2.629e-06
lz/breakdown         off[2]                                        0.000e+00   0.000e+00   2.629e-06
lz/breakdown         Q[2]                                          1.987e-08   1.987e-08   2.384e-07
lz/breakdown         diag[3]                                       4.060e-07   4.060e-07   3.248e-06
lz/breakdown         off[3]                                        2.710e-07   2.710e-07   2.629e-06
lz/breakdown         Q[3]                                          2.328e-07   4.550e-07   3.640e-06
lz/breakdown         diag[2, 0] - lam                              2.980e-08   2.980e-08   2.629e-06
lz/breakdown         orthogonality                                 1.910e-07   1.783e-07   1.427e-06
lz/breakdown         projection                                    8.422e-08   1.476e-07   1.180e-06
lz/breakdown         three_term                                    4.546e-07   7.919e-07   6.335e-06
lz/breakdown         f(A) b                                        1.479e-06   1.479e-06   1.183e-05
lz/zero_mid          diag                                          2.398e-07   2.514e-07   2.011e-06
lz/zero_mid          Q                                             9.090e-07   6.744e-07   5.395e-06
lz/zero_mid          orthogonality                                 1.910e-07   1.658e-07   1.327e-06
lz/zero_mid          projection                                    1.241e-07   1.396e-07   1.117e-06
lz/zero_mid          three_term                                    6.627e-08   8.800e-08   7.040e-07
lz/zero_mid          f(A) b                                        4.586e-07   5.892e-07   4.714e-06
lz/zero_last         diag                                          2.398e-07   1.179e-07   9.430e-07
lz/zero_last         Q                                             9.090e-07   6.744e-07   5.395e-06
lz/zero_last         orthogonality                                 1.590e-07   1.658e-07   1.327e-06
lz/zero_last         projection                                    8.877e-08   1.283e-07   1.026e-06
lz/zero_last         three_term                                    6.627e-08   8.579e-08   6.863e-07
lz/zero_last         f(A) b                                        3.297e-07   1.915e-07   1.532e-06
lz/scale             orthogonality                                 1.590e-07   1.047e-07   8.374e-07
lz/scale             projection                                    8.877e-08   1.228e-07   9.825e-07
lz/scale             three_term                                    6.627e-08   8.715e-08   6.972e-07
lz/scale_breakdown   orthogonality                                 1.568e-07   1.783e-07   1.427e-06
lz/scale_breakdown   projection                                    1.272e-07   1.476e-07   1.180e-06
lz/scale_breakdown   three_term                                    4.546e-07   7.919e-07   6.335e-06
fn/one               f(A) b                                        2.384e-07   1.192e-07   9.537e-07
fn/ident_k2          f(A) b                                        6.351e-07   1.092e-06   8.734e-06
fn/ident_k7          f(A) b                                        6.998e-07   3.806e-07   3.044e-06
fn/five_k5           f(A) b                                        6.793e-07   7.501e-07   6.001e-06
fn/five_k5_inv       f(A) b                                        1.192e-06   9.537e-07   7.629e-06
fn/five_k8           f(A) b                                        6.793e-07   7.501e-07   6.001e-06
fn/five_k8_inv       f(A) b                                        1.192e-06   9.537e-07   7.629e-06
fn/floor             f(A) b                                        4.992e-07   4.992e-07   3.993e-06
fn/clip              f(A) b                                        3.378e-07   2.746e-07   2.197e-06
fn/floor_clip        f(A) b                                        2.623e-07   3.338e-07   2.670e-06
fd/dense24           f(A) b - float64 recurrence                   2.776e-15           -   1.903e-14
fd/dense24           f(A) b - exact (float64)                      3.733e-15   4.552e-15   3.642e-14
fd/breakdown         f(A) b - float64 recurrence                   1.332e-15           -   6.364e-14
fd/breakdown         f(A) b - exact (float64)                      3.553e-15   3.997e-15   6.364e-14
fd/zero_row          f(A) b - float64 recurrence                   1.998e-15           -   2.993e-14
fd/k_gt_d            f(A) b - float64 recurrence                   5.551e-16           -   1.750e-15
fd/k_gt_d            f(A) b - exact (float64)                      4.649e-16   6.661e-16   5.329e-15
cg/spd               X[0] - exact                                  2.039e-05   2.051e-05   1.641e-04
cg/spd               X[0] - float64 iterate                        5.270e-07   5.480e-07   4.384e-06
cg/spd               X[1] - exact                                  3.338e-05   3.338e-05   2.670e-04
cg/spd               X[1] - float64 iterate                        3.385e-07   5.735e-07   4.588e-06
cg/spd               X[2] - exact                                  2.127e-05   2.127e-05   1.702e-04
cg/spd               X[2] - float64 iterate                        5.813e-07   5.464e-07   4.371e-06
cg/spd               X[3] - exact                                  1.925e-05   1.937e-05   1.550e-04
cg/spd               X[3] - float64 iterate                        4.969e-07   6.585e-07   5.268e-06
cg/spd               residual_norm[0]                              2.892e-07   4.634e-07   7.724e-06
cg/spd               residual_norm[1]                              6.085e-08   1.963e-07   7.468e-06
cg/spd               residual_norm[2]                              2.380e-07   1.749e-07   8.037e-06
cg/spd               residual_norm[3]                              5.290e-07   7.513e-07   7.624e-06
cg/small             X[0] - exact                                  1.435e-07   3.678e-08   4.206e-07
cg/small             X[1] - exact                                  6.610e-08   6.610e-08   5.288e-07
cg/small             residual_norm[0]                              2.189e-07   2.103e-08   5.234e-07
cg/small             residual_norm[1]                              1.043e-07   9.862e-08   7.889e-07
cg/N1                X[0] - exact                                  0.000e+00   0.000e+00   1.759e-07
cg/N1                X[0] - float64 iterate                        0.000e+00   0.000e+00   1.759e-07
cg/N1                residual_norm[0]                              0.000e+00   0.000e+00   1.759e-07
cg/blocks            X[0] - exact                                  3.396e-05   3.372e-05   2.698e-04
cg/blocks            X[0] - float64 iterate                        7.595e-07   5.210e-07   7.128e-06
cg/blocks            X[1] - exact                                  3.190e-05   3.166e-05   2.533e-04
cg/blocks            X[1] - float64 iterate                        4.750e-07   4.931e-07   7.154e-06
cg/blocks            X[2] - exact                                  2.980e-05   3.004e-05   2.403e-04
cg/blocks            X[2] - float64 iterate                        4.212e-07   5.057e-07   6.949e-06
cg/blocks            residual_norm[0]                              2.101e-07   2.353e-08   1.543e-05
cg/blocks            residual_norm[1]                              1.098e-07   9.986e-08   1.530e-05
cg/blocks            residual_norm[2]                              4.507e-07   3.196e-07   1.509e-05
cg/long              X[0] - exact                                  3.850e-05   3.850e-05   3.080e-04
cg/long              X[0] - float64 iterate                        8.759e-07   1.203e-06   3.502e-05
cg/long              X[1] - exact                                  4.163e-05   4.139e-05   3.311e-04
cg/long              X[1] - float64 iterate                        9.442e-07   7.628e-07   3.475e-05
cg/long              residual_norm[0]                              2.638e-07   3.362e-07   7.529e-05
cg/long              residual_norm[1]                              1.698e-07   3.449e-07   7.503e-05
cg/atol              X[0] - exact                                  2.412e-02   2.412e-02   1.930e-01
cg/atol              X[0] - float64 iterate                        3.060e-07   4.276e-07   3.421e-06
cg/atol              X[1] - exact                                  2.667e-02   2.667e-02   2.134e-01
cg/atol              X[1] - float64 iterate                        3.077e-07   2.711e-07   2.472e-06
cg/atol              X[2] - exact                                  1.897e-02   1.897e-02   1.518e-01
cg/atol              X[2] - float64 iterate                        5.453e-07   5.453e-07   4.362e-06
cg/atol              X[3] - exact                                  1.808e-02   1.808e-02   1.446e-01
cg/atol              X[3] - float64 iterate                        4.310e-07   4.310e-07   3.448e-06
cg/atol              residual_norm[0]                              3.054e-07   2.452e-08   7.724e-06
cg/atol              residual_norm[1]                              1.199e-07   8.318e-07   7.468e-06
cg/atol              residual_norm[2]                              2.645e-07   4.781e-07   8.037e-06
cg/atol              residual_norm[3]                              1.546e-07   1.274e-07   7.624e-06
cg/frozen            X[0] - exact                                  3.633e-05   3.622e-05   2.897e-04
cg/frozen            X[0] - float64 iterate                        3.065e-07   4.257e-07   3.406e-06
cg/frozen            X[1] - exact                                  4.840e-05   4.828e-05   3.862e-04
cg/frozen            X[1] - float64 iterate                        2.676e-07   2.749e-07   2.370e-06
cg/frozen            X[2] - exact                                  4.029e-05   4.029e-05   3.223e-04
cg/frozen            X[2] - float64 iterate                        2.551e-07   2.365e-07   2.627e-06
cg/frozen            X[3] - exact                                  7.229e-08   7.229e-08   5.783e-07
cg/frozen            X[3] - float64 iterate                        7.229e-08   7.229e-08   5.783e-07
cg/frozen            residual_norm[0]                              2.307e-07   6.640e-08   7.724e-06
cg/frozen            residual_norm[1]                              1.029e-07   7.798e-08   7.468e-06
cg/frozen            residual_norm[2]                              1.585e-08   1.949e-09   8.037e-06
cg/frozen            residual_norm[3]                              2.051e-09   8.306e-08   6.645e-07
cg/zero_row          X[0] - exact                                  3.633e-05   3.622e-05   2.897e-04
cg/zero_row          X[0] - float64 iterate                        3.065e-07   4.257e-07   3.406e-06
cg/zero_row          X[1] - exact                                  4.840e-05   4.828e-05   3.862e-04
cg/zero_row          X[1] - float64 iterate                        2.676e-07   2.749e-07   2.370e-06
cg/zero_row          X[2] - exact                                  4.029e-05   4.029e-05   3.223e-04
cg/zero_row          X[2] - float64 iterate                        2.551e-07   2.365e-07   2.627e-06
cg/zero_row          X[3] - exact                                  0.000e+00   0.000e+00   0.000e+00
cg/zero_row          X[3] - float64 iterate                        0.000e+00   0.000e+00   0.000e+00
cg/zero_row          residual_norm[0]                              2.307e-07   6.640e-08   7.724e-06
cg/zero_row          residual_norm[1]                              1.029e-07   7.798e-08   7.468e-06
cg/zero_row          residual_norm[2]                              1.585e-08   1.949e-09   8.037e-06
cg/zero_row          residual_norm[3]                              0.000e+00   0.000e+00   0.000e+00
cg/x0_random         X[0] - exact                                  2.468e-05   2.468e-05   1.975e-04
cg/x0_random         X[0] - X without x0                           1.392e-05   1.386e-05   1.109e-04
cg/x0_random         X[1] - exact                                  2.191e-05   2.239e-05   1.791e-04
cg/x0_random         X[1] - X without x0                           2.968e-05   2.968e-05   2.375e-04
cg/x0_random         X[2] - exact                                  2.651e-05   2.639e-05   2.112e-04
cg/x0_random         X[2] - X without x0                           1.550e-05   1.621e-05   1.297e-04
cg/x0_random         X[3] - exact                                  1.997e-05   2.009e-05   1.607e-04
cg/x0_random         X[3] - X without x0                           1.574e-05   1.532e-05   1.225e-04
cg/maxiter           X[0] after 4 steps                            1.531e-07   9.551e-08   1.511e-06
cg/maxiter           X[1] after 4 steps                            7.656e-08   1.417e-07   1.472e-06
cg/maxiter           X[2] after 4 steps                            8.295e-08   1.243e-07   1.635e-06
cg/maxiter           X[3] after 4 steps                            7.099e-08   1.115e-07   1.432e-06
cg/stall             X[0] at step 13                               1.301e-02   1.819e-02   1.456e-01
cg/stall             X[1] at step 5                                1.042e-03   5.233e-04   4.186e-03
cgd/mixed            X[0] - exact (float64)                        4.833e-06   4.833e-06           -
cgd/mixed            X[0] - float64 iterate (float64)              4.441e-16           -   4.997e-13
cgd/mixed            X[1] - exact (float64)                        0.000e+00   0.000e+00           -
cgd/mixed            X[1] - float64 iterate (float64)              0.000e+00           -   0.000e+00
cgd/mixed            X[2] - exact (float64)                        3.964e-09   3.964e-09           -
cgd/mixed            X[2] - float64 iterate (float64)              0.000e+00           -   8.626e-14
cgd/mixed            X[3] - exact (float64)                        9.411e-06   9.411e-06           -
cgd/mixed            X[3] - float64 iterate (float64)              6.661e-16           -   6.284e-13
bd/tall              alphas                                        2.068e-07   3.295e-07   2.636e-06
bd/tall              betas                                         1.732e-07   6.388e-07   5.110e-06
bd/tall              V                                             3.400e-07   8.832e-07   7.066e-06
bd/tall              U                                             3.578e-07   6.619e-07   5.295e-06
bd/tall              alphas without bases                          2.068e-07   3.295e-07   2.636e-06
bd/tall              betas without bases                           1.732e-07   6.388e-07   5.110e-06
bd/tall              orth_U                                        1.814e-07   1.426e-07   1.141e-06
bd/tall              orth_V                                        1.451e-07   2.328e-07   1.863e-06
bd/tall              rec_Av                                        9.669e-08   1.701e-07   1.361e-06
bd/tall              rec_Atu                                       1.374e-07   2.109e-07   1.687e-06
bd/tall              cu                                            6.724e-08   6.478e-08   5.183e-07
bd/tall              cv                                            9.243e-08   1.127e-07   9.012e-07
bd/tall              second_pass                                   8.941e-08   1.341e-07   1.073e-06
bd/wide              alphas                                        2.519e-07   1.633e-07   1.306e-06
bd/wide              betas                                         2.830e-07   2.330e-07   1.864e-06
bd/wide              V                                             7.185e-08   5.983e-08   4.787e-07
bd/wide              U                                             4.052e-07   2.926e-07   2.341e-06
bd/wide              alphas without bases                          2.519e-07   1.633e-07   1.306e-06
bd/wide              betas without bases                           2.830e-07   2.330e-07   1.864e-06
bd/wide              orth_U                                        1.846e-07   1.951e-07   1.560e-06
bd/wide              orth_V                                        1.342e-07   2.476e-07   1.981e-06
bd/wide              rec_Av                                        1.975e-07   1.690e-07   1.352e-06
bd/wide              rec_Atu                                       9.337e-08   9.294e-08   7.435e-07
bd/wide              cu                                            1.582e-07   1.345e-07   1.076e-06
bd/wide              cv                                            4.361e-08   5.970e-08   4.776e-07
bd/wide              second_pass                                   2.036e-07   1.832e-07   1.465e-06
bd/full              quadrature                                    2.017e-06   2.622e-06   2.098e-05
bd/full              alphas                                        7.565e-07   7.423e-07   5.938e-06
bd/k1                quadrature                                    8.495e-08   1.369e-07   2.129e-06
bd/k1                alphas                                        7.532e-08   7.532e-08   7.153e-07
df/coeffs_S3         coeffs                                        8.882e-16   5.268e-07   8.076e-06
df/coeffs_S33        coeffs                                        3.508e-06   1.268e-06   1.015e-05
df/closed_form       range_part invsqrt                            7.893e-09   3.852e-08   8.076e-06
df/closed_form       closed_form invsqrt                           8.431e-06   1.052e-05   2.547e-04
df/closed_form       range_part inv                                5.298e-09   3.894e-08   8.076e-06
df/closed_form       closed_form inv                               5.317e-04   5.388e-04   8.053e-03
df/project           project_out                                   4.087e-06   5.301e-06   1.128e-04
df/project           project_out passes=2                          3.714e-06   5.301e-06   1.128e-04
df/project           ||Q out|| passes=2                            7.912e-08   4.369e-05   3.495e-04
df/project           out + Q^T (Q V) - V                           4.087e-06   5.301e-06   1.128e-04
df/relres            relative_residual (exact solution, rounded)   1.123e-08   1.475e-13   3.018e-07
df/relres            relative_residual (perturbed)                 3.360e-08   3.931e-08   3.145e-07
df/cg_deflated       range component of the complement part        1.188e-04   6.843e-04   8.053e-03
go/chol              T Y - Q                                       1.061e-08   9.121e-09   7.297e-08
go/chol              Q Q^T - I                                     1.050e-07   1.664e-07   1.331e-06
go/chol              Y Q^T Q - Y                                   2.869e-05   3.378e-05   2.703e-04
go/eigh_s65          T Y - Q                                       5.960e-08   4.923e-08   3.938e-07
go/eigh_s65          Q Q^T - I                                     6.104e-08   1.689e-07   1.351e-06
go/eigh_s65          Y Q^T Q - Y                                   6.649e-05   5.341e-05   4.272e-04
go/eigh_s384         T Y - Q                                       6.866e-08   4.221e-08   3.376e-07
go/eigh_s384         Q Q^T - I                                     5.930e-08   3.354e-07   2.683e-06
go/eigh_s384         Y Q^T Q - Y                                   1.627e-04   1.272e-04   1.017e-03
go/qr                T Y - Q                                       2.353e-08   1.042e-07   8.334e-07
go/qr                Q Q^T - I                                     3.332e-08   1.110e-07   8.883e-07
go/qr                Y Q^T Q - Y                                   1.287e-05   3.609e-05   2.887e-04
"""
