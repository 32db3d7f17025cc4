"""References of the Krylov drivers (krylov.py) — TEST INFRASTRUCTURE (a plain helper module).

Plain torch on the CPU, one probe at a time, generic in dtype: the same code runs the recurrence in float64 (the
reference; where oracle/matfree.py restates the function, the tests compare with that one and
tests/test_krylov_drivers_cpu.py asserts that the two agree) and in float32 (what an honest float32 execution of the same
algorithm costs on the same input).  The distance of the two runs, ``D32``, sets every floating-point bound of
tests/test_krylov_drivers.py: ``bound(D32, scale) = max(8 D32, 4 * 2^-24 * scale)``.

The operators are built once in float32 — the device gets those tensors, the float64 runs their exact ``.double()``
images — so both precisions see the same matrix.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch

U24 = 2.0 ** -24


def bound(d32: float, scale: float) -> float:
    return max(8.0 * float(d32), 4.0 * U24 * float(scale))


def maxabs(a: torch.Tensor, b: torch.Tensor) -> float:
    if a.numel() == 0:
        return 0.0
    return float((a.double() - b.double()).abs().max())


# ------------------------------------------------------------------------------------------------ operators
@dataclass
class Operator:
    """A linear map given by float32 tensors.  ``on(dtype, device)`` returns callables on blocks (P, N): ``matvec`` and,
    for a rectangular map, ``vecmat``; ``dense(dtype)`` the explicit matrix (n_out, N) on the CPU."""
    kind: str
    t: Dict[str, torch.Tensor]
    scale: float = 1.0               # an exact power of two applied to the map

    @property
    def N(self):
        for key in ("d", "A", "Qt"):
            if key in self.t:
                return self.t[key].shape[-1]
        raise KeyError(self.kind)

    def scaled(self, s: float) -> "Operator":
        return Operator(self.kind, self.t, self.scale * s)

    def on(self, dtype, device="cpu"):
        t = {k: v.to(device=device, dtype=dtype) for k, v in self.t.items()}
        s = self.scale

        def rows(A, V):
            # one product per probe, of a fixed shape: a row's result does not depend on its neighbours in the block
            return torch.stack([(A * v[None, :]).sum(1) for v in V]) if V.shape[0] else V.new_zeros(0, A.shape[0])
        if self.kind == "diag":
            return (lambda V: V * (t["d"] * s)), None
        if self.kind == "diag_bf16":                 # a deterministic noise floor of 2^-9 relative per element
            return (lambda V: (V * (t["d"] * s)).bfloat16().to(dtype)), None
        if self.kind == "dense":
            A = t["A"] * s
            return (lambda V: rows(A, V)), None
        if self.kind == "rect":
            A = t["A"] * s
            At = A.T.contiguous()
            return (lambda V: rows(A, V)), (lambda U: rows(At, U))
        if self.kind == "defl":
            Qt, w, al = t["Qt"], t["w"], float(self.t["alpha"])
            return (lambda V: s * (al * V + ((V @ Qt.T) * w[None, :]) @ Qt)), None
        raise KeyError(self.kind)

    def norm(self) -> float:
        """||A||_2 of the float64 image"""
        if self.kind in ("diag", "diag_bf16"):
            return float(self.t["d"].double().abs().max()) * self.scale
        if self.kind == "defl":
            return float(self.t["lam"].double().max()) * self.scale
        return float(torch.linalg.matrix_norm(self.dense(), 2))

    def cond(self) -> float:
        if self.kind in ("diag", "diag_bf16"):
            d = self.t["d"].double().abs()
            return float(d.max() / d.min())
        return float(torch.linalg.cond(self.dense()))

    def dense(self, dtype=torch.float64) -> torch.Tensor:
        t = {k: v.to(dtype) for k, v in self.t.items()}
        if self.kind in ("diag", "diag_bf16"):
            return torch.diag(t["d"]) * self.scale
        if self.kind in ("dense", "rect"):
            return t["A"] * self.scale
        if self.kind == "defl":
            n = t["Qt"].shape[1]
            return self.scale * (float(self.t["alpha"]) * torch.eye(n, dtype=dtype) + (t["Qt"].T * t["w"][None, :]) @ t["Qt"])
        raise KeyError(self.kind)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def op_diag(d: torch.Tensor, noisy=False) -> Operator:
    return Operator("diag_bf16" if noisy else "diag", dict(d=d.float()))


def op_outliers(N: int, small=0.01, noisy=True) -> Operator:
    """diagonal: a cluster linspace(1, 2) and three small outliers — the CG residual oscillates while the outliers are
    resolved (plateaus that last several steps) — through a bfloat16-rounded product"""
    d = torch.linspace(1.0, 2.0, N, dtype=torch.float64)
    d[:3] = torch.tensor([1.0, 2.0, 3.5], dtype=torch.float64) * small
    return op_diag(d, noisy)


def op_dense_sym(N: int, seed: int, lo=1.0, hi=2.0) -> Operator:
    """a dense symmetric matrix with spectrum linspace(lo, hi, N) (up to the float32 rounding of its entries)"""
    Qm, _ = torch.linalg.qr(torch.randn(N, N, generator=_gen(seed), dtype=torch.float64))
    A = (Qm * torch.linspace(lo, hi, N, dtype=torch.float64)[None, :]) @ Qm.T
    A = A.float()
    return Operator("dense", dict(A=0.5 * (A + A.T)))                # (x + y) / 2 is symmetric in float32 too


def op_lowrank(N: int, r: int, seed: int, shift=0.5) -> Operator:
    """shift I + B B^T with B (N, r) of small dyadic entries, so that the float32 matrix IS of that form and every
    Krylov space has dimension <= r + 1 exactly; rows 3 and 4 of B are equal and row 5 is zero, which makes
    e_3 - e_4 and e_5 eigenvectors of the eigenvalue ``shift``.  ``.t["B"]`` keeps B (exact in float32)."""
    B = torch.randint(-3, 4, (N, r), generator=_gen(seed)).double() / 4.0
    if N > 5:
        B[4] = B[3]
        B[5] = 0.0
    A = shift * torch.eye(N, dtype=torch.float64) + B @ B.T
    assert torch.equal(A.float().double(), A)
    return Operator("dense", dict(A=A.float(), B=B.float()))


def op_rect(n_out: int, N: int, seed: int) -> Operator:
    """a full-rank rectangular map with singular values between 1 and 3"""
    m = min(n_out, N)
    Uo, _ = torch.linalg.qr(torch.randn(n_out, m, generator=_gen(seed), dtype=torch.float64))
    Vo, _ = torch.linalg.qr(torch.randn(N, m, generator=_gen(seed + 1), dtype=torch.float64))
    A = (Uo * torch.linspace(1.0, 3.0, m, dtype=torch.float64)[None, :]) @ Vo.T
    return Operator("rect", dict(A=A.float().contiguous()))


def op_deflation(N: int, r: int, seed: int, lam_lo=1.0, lam_hi=1e6, alpha=1e-3) -> Operator:
    """alpha I + Qt^T diag(lam - alpha) Qt with Qt orthonormalised in float64, then rounded to float32"""
    Qm, _ = torch.linalg.qr(torch.randn(N, r, generator=_gen(seed), dtype=torch.float64))
    lam = torch.logspace(math.log10(lam_lo), math.log10(lam_hi), r, dtype=torch.float64).float()
    return Operator("defl", dict(Qt=Qm.T.float().contiguous(), w=(lam.double() - alpha).float(), lam=lam,
                                 alpha=torch.tensor(alpha, dtype=torch.float64)))


# ------------------------------------------------------------------------------------------------ Lanczos
def lanczos(matvec: Callable, v0: torch.Tensor, k: int, brk_rtol2: float):
    """The recurrence of ``krylov.lanczos_tridiag`` for one probe: start v0 / ||v0||, per step two passes of classical
    Gram-Schmidt against the whole basis, diag[j] = the sum of the two coefficients on q_j, breakdown when
    ||w||^2 <= brk_rtol2 ||A q_j||^2 (the remaining block is diag 1, off 0, zero basis rows); a zero start is broken
    down from the beginning.  Returns Q (k, N), diag (k,), off (k-1,), and the step at which it broke down (k: never;
    j: off[j] is the first zero; -1: zero start)."""
    dt = v0.dtype
    n = v0.numel()
    Q = torch.zeros(k, n, dtype=dt)
    diag = torch.ones(k, dtype=dt)
    off = torch.zeros(max(k - 1, 0), dtype=dt)
    nrm2 = torch.dot(v0, v0)
    if float(nrm2) == 0.0:
        return Q, diag, off, -1
    q = v0 / torch.sqrt(nrm2)
    for j in range(k):
        Q[j] = q
        w = matvec(q[None, :])[0]
        wn2 = torch.dot(w, w)
        c1 = Q[: j + 1] @ w
        w = w - Q[: j + 1].T @ c1
        c2 = Q[: j + 1] @ w
        w = w - Q[: j + 1].T @ c2
        diag[j] = c1[j] + c2[j]
        if j + 1 < k:
            nrm2 = torch.dot(w, w)
            if not float(nrm2) > brk_rtol2 * float(wn2):
                return Q, diag, off, j
            off[j] = torch.sqrt(nrm2)
            q = w / off[j]
    return Q, diag, off, k


BRK = {torch.float32: 1e-10, torch.float64: 1e-26}      # float32: the driver's own; float64: (1e-13)^2 as in the oracle


def lanczos_block(op: Operator, V0: torch.Tensor, k: int, dtype):
    """:func:`lanczos` for every row of V0 (float32 data, run in ``dtype``): Q (P, k, N), diag, off, breakdown steps"""
    mv, _ = op.on(dtype)
    outs = [lanczos(mv, v.to(dtype), k, BRK[dtype]) for v in V0]
    return (torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs]),
            [o[3] for o in outs])


def tridiag(diag, off):
    T = torch.diag_embed(diag)
    if off.shape[-1] > 0:
        T = T + torch.diag_embed(off, 1) + torch.diag_embed(off, -1)
    return T


def funm_from_lanczos(Q, diag, off, length, f, floor=None, clip_min=None):
    """||b|| Q^T f(T) e1 per probe, the small algebra in float64 as in the driver; the result in the dtype of Q"""
    ev, U = torch.linalg.eigh(tridiag(diag.double(), off.double()))
    if floor is not None:
        ev = ev.clamp(min=floor)
    if clip_min is not None:
        ev = ev.clamp(min=clip_min)
    fT0 = ((U * f(ev).unsqueeze(-2)) @ U.transpose(-1, -2))[:, :, 0]
    coef = (fT0 * length.double()[:, None]).to(Q.dtype)
    return torch.einsum("pk,pkn->pn", coef, Q)


def funm_exact(op: Operator, B: torch.Tensor, f, floor=None, clip_min=None) -> torch.Tensor:
    """f(A) b for the rows of B through eigh of the dense float64 matrix, with the same clamps on the exact spectrum"""
    if op.kind == "diag":
        ev, U = op.t["d"].double() * op.scale, None
    else:
        ev, U = torch.linalg.eigh(op.dense())
    if floor is not None:
        ev = ev.clamp(min=floor)
    if clip_min is not None:
        ev = ev.clamp(min=clip_min)
    if U is None:
        return B.double() * f(ev)[None, :]
    return ((B.double() @ U) * f(ev)[None, :]) @ U.T


# ------------------------------------------------------------------------------------------------ Golub-Kahan
def bidiag(matvec: Callable, vecmat: Callable, v0: torch.Tensor, k: int):
    """The recurrence of ``krylov.bidiag`` for one probe (two passes of classical Gram-Schmidt against the whole basis on
    either side, no breakdown guard): alphas (k,), betas (k-1,), V (k, N), U (k, n_out) and the coefficient arrays
    (cu1, cu2, cv1, cv2), each (k, k)."""
    dt = v0.dtype
    v = v0 / torch.linalg.vector_norm(v0)
    Vs, Us = [], []
    alphas, betas = torch.zeros(k, dtype=dt), torch.zeros(max(k - 1, 0), dtype=dt)
    co = [torch.zeros(k, k, dtype=dt) for _ in range(4)]
    for j in range(k):
        Vs.append(v)
        u = matvec(v[None, :])[0]
        if j > 0:
            Um = torch.stack(Us)
            for c in (co[0], co[1]):
                c[j, :j] = Um @ u
                u = u - Um.T @ c[j, :j]
        alphas[j] = torch.linalg.vector_norm(u)
        u = u / alphas[j]
        Us.append(u)
        if j + 1 < k:
            w = vecmat(u[None, :])[0]
            Vm = torch.stack(Vs)
            for c in (co[2], co[3]):
                c[j, :j + 1] = Vm @ w
                w = w - Vm.T @ c[j, :j + 1]
            betas[j] = torch.linalg.vector_norm(w)
            v = w / betas[j]
    return alphas, betas, torch.stack(Vs), torch.stack(Us), tuple(co)


def bidiag_block(op: Operator, V0: torch.Tensor, k: int, dtype):
    mv, vm = op.on(dtype)
    outs = [bidiag(mv, vm, v.to(dtype), k) for v in V0]
    st = lambda i: torch.stack([o[i] for o in outs])
    return st(0), st(1), st(2), st(3), tuple(torch.stack([o[4][c] for o in outs]) for c in range(4))


def slq_from_bidiag(alphas, betas, length2):
    """||v||^2 e1^T log(B^T B) e1 per probe, the small algebra in float64 as in the driver"""
    B = torch.diag_embed(alphas.double())
    if betas.shape[-1] > 0:
        B = B + torch.diag_embed(betas.double(), 1)
    _, S, Vt = torch.linalg.svd(B)
    return length2.double() * (Vt[:, :, 0] ** 2 * torch.log(S ** 2)).sum(-1)


def slq_exact(op: Operator, V0: torch.Tensor) -> torch.Tensor:
    """v^T log(A^T A) v per probe from eigh in float64"""
    A = op.dense()
    ev, W = torch.linalg.eigh(A.T @ A)
    C = V0.double() @ W
    return (C * C * torch.log(ev)[None, :]).sum(1)


# ------------------------------------------------------------------------------------------------ CG
def cg(A: Callable, b: torch.Tensor, x0: Optional[torch.Tensor] = None, tol=1e-5, atol=0.0, maxiter=None,
       stall: Optional[int] = None, keep=False):
    """``jax.scipy.sparse.linalg.cg`` for one right-hand side (the loop of oracle/matfree.py ``cg``), with the iteration
    count, the recurrence residual ||r|| after every step and, with ``keep``, every iterate; ``stall`` is the driver's
    rule (stop once ||r||^2 has not fallen below 0.81 x its best for ``stall`` steps in a row)."""
    n = b.numel()
    maxiter = 10 * n if maxiter is None else maxiter
    Af = lambda v: A(v[None, :])[0]
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    atol2 = max(float(tol) ** 2 * float(torch.dot(b, b)), float(atol) ** 2)
    r = b - Af(x) if x0 is not None else b.clone()
    p = r.clone()
    gamma = torch.dot(r, r)
    hist, xs = [float(gamma) ** 0.5], [x.clone()]
    true = [float(torch.linalg.vector_norm(b - Af(x)))] if keep else []
    best, since, k = float(gamma), 0, 0
    while float(gamma) > atol2 and k < maxiter and (stall is None or since < stall):
        Ap = Af(p)
        alpha = gamma / torch.dot(p, Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        gamma_new = torch.dot(r, r)
        p = r + (gamma_new / gamma) * p
        gamma = gamma_new
        k += 1
        since = 0 if float(gamma) < 0.81 * best else since + 1
        best = min(best, float(gamma))
        hist.append(float(gamma) ** 0.5)
        if keep:
            xs.append(x.clone())
            true.append(float(torch.linalg.vector_norm(b - Af(x))))
    return x, dict(iterations=k, hist=hist, xs=xs, true=true)


def cg_block(op: Operator, B: torch.Tensor, dtype, X0: Optional[torch.Tensor] = None, **kw):
    """:func:`cg` for every row of B: X (P, N), the per-row iteration counts, the per-row infos"""
    mv, _ = op.on(dtype)
    outs = [cg(mv, b.to(dtype), None if X0 is None else X0[i].to(dtype), **kw) for i, b in enumerate(B)]
    return torch.stack([o[0] for o in outs]), [o[1]["iterations"] for o in outs], [o[1] for o in outs]


def plateau_step(hist, stall: int) -> int:
    """first iteration t after which ``stall`` residuals in a row fail to fall 10 % below the best so far (0.81 on the
    square, the driver's rule): the step at which the run stops improving; len(hist) if it never does"""
    r2 = [h * h for h in hist]
    for t in range(len(r2) - stall):
        best = min(r2[: t + 1])
        run = best
        ok = True
        for v in r2[t + 1: t + 1 + stall]:
            if v < 0.81 * run:
                ok = False
                break
            run = min(run, v)
        if ok:
            return t
    return len(hist)


def keep_best_walk(true, patience: int):
    """(stop step, index of the iterate kept) of the driver's ``keep_best`` rule on a history of TRUE residual norms"""
    tb, idle, kept = true[0] ** 2, 0, 0
    for t in range(1, len(true)):
        tt = true[t] ** 2
        idle = 0 if tt < 0.81 * tb else idle + 1
        if tt < tb:
            tb, kept = tt, t
        if idle >= patience:
            return t, kept
    return len(true) - 1, kept


def solve_exact(op: Operator, B: torch.Tensor) -> torch.Tensor:
    if op.kind == "diag":
        return B.double() / (op.t["d"].double() * op.scale)[None, :]
    return torch.linalg.solve(op.dense(), B.double().T).T
