"""Float64 yardstick of the low-rank Laplace posterior (CPU torch; no product code on its path).

The GGN of a data set is G = sum_i J_i^T H_i J_i (x exp(-logvar) for the regressor, N/M = 1) with the autograd Jacobians
of ``last_layer_ref.jac64`` and the head Hessians of ``kfac_ref.head_hessians``.  It is kept as its square-root factor
W (M K, D), G = W^T W (rows L_i^T J_i with H_i = L_i L_i^T from an eigendecomposition), so that nets with thousands of
parameters need no D x D matrix: the operator is V -> (V W^T) W, the exact eigenpairs come from the small Gram W W^T, and
``dense()`` writes G out for the nets where that is cheap.

``subspace_iteration`` restates ``krylov.top_eigenpairs`` in float64 WITH THE PROBES AS AN ARGUMENT: the same order of
products, the same orthonormalisation rule (Gram eigenvalues above rtol x the largest, twice), the same projection.
``check_case`` asserts the two conditions under which its answer is comparable with a float32 run of the same
recurrence: (a) no row is dropped by either orthonormalisation, (b) lam_{rank+1} / lam_rank <= 0.8 in the exact spectrum.
Eigenvectors are never compared across implementations: only eigenvalues, projectors U^T U, variances and predictives.
"""
import math

import torch

import kfac_ref as kf
import last_layer_ref as ref

F64 = torch.float64
GAP = 0.8

# (rank, oversample) per net of tests/last_layer_kron_ref.py, chosen from the exact spectra (scalar and two-group prior)
# so that both conditions of ``check_case`` hold with power_iters = 1: the rank sits right before a gap
# (lam_{k+1} / lam_k = 0.15, 0.05, 0.24, 0.09, 0.12 in this order; at most 0.26 under the two-group prior) and
# P = rank + oversample stays inside the numerical rank with lam_P / lam_1 >= 7e-4.
CONFIG = {"sine_regressor": (4, 2), "xor_classifier": (3, 5), "mlp_ragged": (4, 8), "resnet_tiny": (3, 4), "flat_head": (2, 6)}
NETS = list(CONFIG)


def probes_for(name, D):
    """the (P, D) float32 probe block of a net, drawn once on the CPU: both sides start from these numbers"""
    rank, over = CONFIG[name]
    g = torch.Generator().manual_seed(1000 + NETS.index(name))
    return torch.randn(rank + over, D, generator=g, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- the algorithm, float64
def orthonormalize(Y, rtol=1e-10):
    """(Q, dropped): orthonormal rows spanning the rows of Y by two passes of Q = L^(-1/2) U^T Y on the Gram's
    eigendecomposition, keeping eigenvalues above rtol (first pass) / 0.25 (second) x the largest"""
    Q, rows = Y, Y.shape[0]
    if not bool((Y != 0).any()):
        return Y[:0], rows
    for it in range(2):
        G = Q @ Q.T
        ev, U = torch.linalg.eigh(0.5 * (G + G.T))
        keep = ev > (rtol if it == 0 else 0.25) * ev.max()
        Q = (U[:, keep] * ev[keep].rsqrt()).T @ Q
    return Q, rows - Q.shape[0]


def subspace_iteration(matvec, probes, rank, power_iters=1, rtol=1e-10):
    """``krylov.top_eigenpairs`` in float64 on the rows of ``probes`` (P, N): (lam (r,) descending, U (r, N), info) with
    info = dict(passes, dropped=[per orthonormalisation], residual (r,))"""
    Y = matvec(probes.to(F64))
    passes, dropped = 1, []
    Q = None
    for _ in range(power_iters + 1):
        Q, d = orthonormalize(Y, rtol)
        dropped.append(d)
        if Q.shape[0] == 0:
            return torch.zeros(0, dtype=F64), Q, dict(passes=passes, dropped=dropped, residual=torch.zeros(0, dtype=F64))
        Y = matvec(Q)
        passes += 1
    B = Y
    T = B @ Q.T
    ev, S = torch.linalg.eigh(0.5 * (T + T.T))
    r = min(rank, Q.shape[0])
    lam = ev.flip(0)[:r].clamp_min(0.0)
    Sk = S.flip(1)[:, :r].T
    U = Sk @ Q
    residual = (Sk @ B - lam[:, None] * U).norm(dim=1) / lam.max().clamp_min(1e-300)
    return lam, U, dict(passes=passes, dropped=dropped, residual=residual)


def check_case(lam_exact, rank, info):
    """the two conditions of the module docstring; ``lam_exact`` descending"""
    assert all(d == 0 for d in info["dropped"]), f"rows dropped by the orthonormalisation passes: {info['dropped']}"
    ratio = float(lam_exact[rank] / lam_exact[rank - 1]) if rank < lam_exact.numel() else 0.0
    assert ratio <= GAP, f"no gap after rank {rank}: lam_(k+1) / lam_k = {ratio:.3f}"
    return ratio


# ---------------------------------------------------------------------------------------------- the GGN of a net
def factor(state, Z, model_type):
    """W (M K, D) float64 with G = W^T W at N/M = 1 (x exp(-logvar) for the regressor)"""
    f, J = ref.jac64(state, Z, model_type)
    H = kf.head_hessians(f, model_type)
    ev, V = torch.linalg.eigh(H)
    Lt = ev.clamp_min(0.0).sqrt()[:, :, None] * V.transpose(1, 2)              # (n, K, K): H = Lt^T Lt
    W = (Lt @ J).reshape(-1, J.shape[2])
    return math.sqrt(ref.recal(state, Z.shape[0], model_type, None)) * W


def operator(W, isq=None):
    """V (P, D) -> V G, or V -> ((V o isq) G) o isq (the curvature whitened by a vector prior)"""
    if isq is None:
        return lambda V: (V @ W.T) @ W
    return lambda V: (((V * isq) @ W.T) @ W) * isq


def dense(W, isq=None):
    G = W.T @ W
    return G if isq is None else isq[:, None] * G * isq[None, :]


def exact_eigh(W, isq=None):
    """(lam (M K,) descending, U (M K, D) rows; rows of zero eigenvalues are zero) of W^T W from the small Gram"""
    Ww = W if isq is None else W * isq
    ev, V = torch.linalg.eigh(Ww @ Ww.T)
    ev, V = ev.flip(0).clamp_min(0.0), V.flip(1)
    pos = ev > 1e-14 * ev.max()
    U = torch.where(pos[:, None], (V.T @ Ww) * ev.clamp_min(1e-300).rsqrt()[:, None], torch.zeros_like(Ww))
    return ev, U


# ---------------------------------------------------------------------------------------------- the posterior, densely
def prior_vector(a, D):
    return torch.as_tensor(a, dtype=F64).expand(D).clone()


def whiten(lam, recal_nm, alpha=None):
    """lam_t: (N/M) lam / alpha for a scalar prior, (N/M) lam for a whitened operator (alpha None)"""
    return recal_nm * lam / (1.0 if alpha is None else alpha)


def precision_dense(U, lam_t, a):
    """A0^(1/2) (I + U^T diag(lam_t) U) A0^(1/2)"""
    sq = prior_vector(a, U.shape[1]).sqrt()
    return sq[:, None] * (torch.eye(U.shape[1], dtype=F64) + U.T @ (lam_t[:, None] * U)) * sq[None, :]


def sigma_dense(U, lam_t, a):
    """the inverse of :func:`precision_dense` through a dense solve"""
    P = precision_dense(U, lam_t, a)
    return torch.linalg.solve(0.5 * (P + P.T), torch.eye(P.shape[0], dtype=F64))


def sigma_closed(U, lam_t, a):
    """A0^(-1/2) (I - U^T diag(s) U) A0^(-1/2) written out (for nets too large for the solve)"""
    isq = prior_vector(a, U.shape[1]).rsqrt()
    s = lam_t / (1.0 + lam_t)
    return isq[:, None] * (torch.eye(U.shape[1], dtype=F64) - U.T @ (s[:, None] * U)) * isq[None, :]


def variance_ref(U, lam_t, a):
    s = lam_t / (1.0 + lam_t)
    return (1.0 - (s[:, None] * U * U).sum(0)) / prior_vector(a, U.shape[1])


def predict_ref(J, U, lam_t, a):
    """(B, K, K): J Sigma J^T for Jacobians J (B, K, D) without the D x D matrix"""
    isq = prior_vector(a, U.shape[1]).rsqrt()
    Jw = J * isq
    JU = Jw @ U.T
    s = lam_t / (1.0 + lam_t)
    return Jw @ Jw.transpose(1, 2) - torch.einsum("bkr,r,bmr->bkm", JU, s, JU)


def sample_map_ref(eps, U, lam_t, a):
    """A0^(-1/2) (I + U^T diag(1 / sqrt(1 + lam_t) - 1) U) eps for rows eps (S, D)"""
    isq = prior_vector(a, U.shape[1]).rsqrt()
    g = 1.0 / torch.sqrt(1.0 + lam_t) - 1.0
    return (eps + ((eps @ U.T) * g) @ U) * isq


def lml_ref(alpha, lam, D, theta2, rescale):
    """the evidence of the truncated spectrum (``last_layer_ref.lml_ref``)"""
    return ref.lml_ref(alpha, lam, D, theta2, rescale)


def projector(U):
    return U.T @ U
