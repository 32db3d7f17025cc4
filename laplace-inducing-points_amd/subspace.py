"""The eigen-solver of the low-rank Laplace posterior and the streaming primitive its marginal variance needs, built on
the drivers of ``krylov.py`` and re-exported there as ``krylov.top_eigenpairs`` and ``krylov.cols_wsqsum``.

``top_eigenpairs`` is a randomized block subspace iteration whose every dense step is a HIP primitive that already
exists (CholeskyQR2 on ``lip_dot_nt_f64``, ``lip_rows_combine``); ``cols_wsqsum`` wraps ``lip_cols_wsqsum``
(``csrc/lip_krylov.hip``).  All blocks are (P, N) float32 on the GPU, as in ``krylov.py``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import _native as nv
from . import krylov as _k


def cols_wsqsum(U: torch.Tensor, w: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[d] += sum_j w[j] U[j, d]^2 for float32 rows U (k, N) (any row stride): float64 column sums in one read of U and
    without a (k, N) temporary, bitwise reproducible (``lip_cols_wsqsum``).  ``w`` (k,) is taken in float64 (None: ones);
    ``out`` (N,) float64 is added into (a zero vector when not given)."""
    lib = nv.load()
    U, ldu = _k._rows_f32(U)
    k, N = U.shape
    if out is None:
        out = torch.zeros(N, device=U.device, dtype=torch.float64)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == N):
        raise ValueError(f"cols_wsqsum: out must be a contiguous float64 device vector of {N} doubles")
    if k == 0 or N == 0:
        return out
    wp = 0
    if w is not None:
        w = w.to(device=U.device, dtype=torch.float64).contiguous()
        if w.numel() != k:
            raise ValueError(f"cols_wsqsum: w must hold {k} weights, got {tuple(w.shape)}")
        wp = w.data_ptr()
    nv.check(lib.lip_cols_wsqsum(U.data_ptr(), ldu, k, N, wp, out.data_ptr(), nv.stream_ptr()), "lip_cols_wsqsum")
    return out


def top_eigenpairs(matvec: Callable[[torch.Tensor], torch.Tensor], N: int, rank: int, oversample: int = 8,
                   power_iters: int = 1, seed: int = 0, probes: Optional[torch.Tensor] = None, rtol: float = 1e-10,
                   device="cuda"):
    """The leading eigenpairs of a symmetric positive semi-definite block operator ``matvec`` ((P, N) float32 device rows
    -> (P, N)) by randomized block subspace iteration (Halko, Martinsson & Tropp 2011, algorithms 4.4 + 5.3) with
    P = rank + oversample probes:

        Omega (P, N) = ``fill_normal(seed)`` or ``probes``;  Y = A Omega;
        ``power_iters`` times:  Q = orth(Y) (:func:`gram_orthonormalize`, ``rtol``),  Y = A Q;
        Q = orth(Y);  B = A Q;  T = sym(B Q^T) in float64 (``dot_nt``) = S diag(ev) S^T;
        the min(rank, rows of Q) largest ev, clamped at 0, are ``lam``;  U = S_k^T Q (``rows_combine``).

    Returns ``(lam (r,) float64 descending, U (r, N) float32 with orthonormal rows, info)``; ``info`` holds ``passes``
    (operator applications, power_iters + 2), ``rows`` (of the final Q), ``dropped`` (rows the orthonormalisations took
    out, P - rows: a rank-deficient Y yields fewer rows) and ``residual`` (r,) = ||S_k^T B - lam_j u_j|| / max(lam), the
    Ritz residuals from the block already at hand.  A zero operator returns zero pairs.  The Ritz values never exceed
    the eigenvalues they approximate (Cauchy interlacing)."""
    rank, P = int(rank), int(rank) + int(oversample)
    if rank < 1 or oversample < 0 or power_iters < 0:
        raise ValueError(f"top_eigenpairs: rank >= 1, oversample >= 0 and power_iters >= 0 are needed (got {rank}, "
                         f"{oversample}, {power_iters})")
    if probes is None:
        Omega = _k.fill_normal(P, N, seed, device=device)
    else:
        Omega = _k._chk(probes)
        if tuple(Omega.shape) != (P, N):
            raise ValueError(f"top_eigenpairs: probes must be ({P}, {N}) = (rank + oversample, N), got {tuple(Omega.shape)}")
    Y = _k._chk(matvec(Omega).contiguous())
    passes = 1
    Q = None
    for it in range(int(power_iters) + 1):
        Q = _k.gram_orthonormalize(Y, rtol)
        if Q.shape[0] == 0:
            break
        Y = _k._chk(matvec(Q).contiguous())                # the last product is B = A Q of the projection
        passes += 1
    dev = Omega.device
    if Q.shape[0] == 0:
        return (torch.zeros(0, device=dev, dtype=torch.float64), torch.zeros(0, N, device=dev, dtype=torch.float32),
                dict(passes=passes, rows=0, dropped=P, residual=torch.zeros(0, device=dev, dtype=torch.float64)))
    B = Y
    T = _k.dot_nt(B, Q)
    ev, S = torch.linalg.eigh(0.5 * (T + T.T))
    r = min(rank, Q.shape[0])
    lam = ev.flip(0)[:r].clamp_min(0.0).contiguous()
    Sk = S.flip(1)[:, :r].T.contiguous()                # (r, rows)
    U = _k.rows_combine(Sk, Q)
    Rk = _k.axpby(_k.rows_combine(Sk, B), U, (-lam).float().contiguous(), 1.0, None, 1.0)      # S_k^T B - lam u, in place
    residual = torch.sqrt(_k.bdot(Rk, Rk).double()) / lam.max().clamp_min(1e-300)
    return lam, U, dict(passes=passes, rows=int(Q.shape[0]), dropped=P - int(Q.shape[0]), residual=residual)
