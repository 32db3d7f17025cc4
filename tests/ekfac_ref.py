"""Float64 yardstick of the eigenvalue-corrected Kronecker-factored posterior (CPU torch; no product code on its path).

Everything comes from the autograd Jacobian J (n, K, D) of ``last_layer_ref.jac64`` and the head Hessians H_i of
``kfac_ref.head_hessians``.  For a layer block (offset, Mt, N) and a basis (V (Mt, Mt), Ub (N, N)),

    T_{i,k} = V^T mat(J_i[k]) Ub,    Lam[j][l] = sum_i sum_{k,m} T_{i,k}[j][l] H_i[k][m] T_{i,m}[j][l],

which is sum_r (V^T mat(J_i^T L_i e_k) Ub)^2 over the rows of any square-root factor H_i = L_i L_i^T, and the diagonal of
(V (x) Ub)^T G (V (x) Ub) for the exact block G = sum_i J_i^T H_i J_i.  The dense covariance of a block is
(V (x) Ub) diag(1 / (recal Lam + 1)) (V (x) Ub)^T, built with ``torch.kron``.
"""
import math

import torch

import kfac_ref as kf
import last_layer_kron_ref as kref
import last_layer_ref as ref

F64 = torch.float64
DENSE_CAP = 4096                     # blocks of more than this many parameters are not densified for the Frobenius checks


def jacobian(state, Z, model_type):
    """(f (n, K), J (n, K, D), H (n, K, K))"""
    f, J = ref.jac64(state, Z, model_type)
    return f, J, kf.head_hessians(f, model_type)


def block_rows(J, off, Mt, N):
    return J[:, :, off:off + Mt * N].reshape(J.shape[0], J.shape[1], Mt, N)


def scales_ref(J, H, state, bases):
    """[Lam_l (Mt, N)] of the module docstring, unscaled, for ``bases[l] = (V, Ub)`` (float64 CPU)"""
    out = []
    for (_, off, Mt, N, _, _), (V, Ub) in zip(kf.blocks_of(state), bases):
        Tm = V.T @ block_rows(J, off, Mt, N) @ Ub
        out.append(torch.einsum("ikjl,ikm,imjl->jl", Tm, H, Tm))
    return out


def scales_final_dense(state, Z, model_type, V, Ub):
    """Lam of the final Dense block from the features and probabilities alone (no Jacobian):
    Lam[j][l] = sum_i (V^T phit_i)_j^2 (Ub^T H_i Ub)_{ll}"""
    f, phit, _ = ref.features64(state, Z)
    H = kf.head_hessians(f, model_type)
    return ((phit @ V) ** 2).T @ torch.einsum("kl,ikm,ml->il", Ub, H, Ub)


def dense_covariance(V, Ub, Lam, recal):
    W = torch.kron(V, Ub)
    return (W * (1.0 / (recal * Lam + 1.0)).reshape(-1)[None, :]) @ W.T


def covariance_blocks(state, bases, Lams, recal):
    """[(offset, (Mt N, Mt N))], the shape of ``kfac_ref.covariance_blocks``'s first result"""
    return [(off, dense_covariance(V, Ub, Lam, recal)) for (_, off, _, _, _, _), (V, Ub), Lam in
            zip(kf.blocks_of(state), bases, Lams)]


def exact_block(J, H, off, Mt, N):
    """sum_i J_i^T H_i J_i over the block's slice, unscaled: (Mt N, Mt N)"""
    Jb = J[:, :, off:off + Mt * N]
    return torch.einsum("ikd,ikm,ime->de", Jb, H, Jb)


def orthonormal_bases(state, As, Ss, model_type):
    """[(U_A, U_S)] from the helper's own factors (the final classifier block centred)"""
    out = []
    for (u, _, _, _, _, _), A, S in zip(kf.blocks_of(state), As, Ss):
        S = kf.head_factor(state, u, S, model_type)
        out.append((torch.linalg.eigh(0.5 * (A + A.T))[1], torch.linalg.eigh(0.5 * (S + S.T))[1]))
    return out


def best_diagonal(G, Q):
    """diag(Q^T G Q): the s that minimises ||G - Q diag(s) Q^T||_F for orthonormal Q"""
    return torch.einsum("dq,de,eq->q", Q, G, Q)


def frobenius_error(G, Q, s):
    return float(torch.linalg.norm(G - (Q * s[None, :]) @ Q.T))


def spectrum_ref(state, Lams0, model_type, diag1):
    """the evidence spectrum at N/M = 1: Lam0_l (x exp(-logvar) for the regressor) per block and the remainder's GGN
    diagonal ``diag1`` (built at N/M = 1)"""
    scale = math.exp(-float(state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0
    parts = [scale * Lam.clamp_min(0.0).reshape(-1) for Lam in Lams0]
    parts.append(diag1[kf.remainder_of(state)].clamp_min(0.0))
    return torch.cat(parts)
