"""Float64 yardstick of the row-free Kronecker-factored predictive (CPU torch; no product code on its path).

For a layer block with patches at_{i,t} (Mt, a leading 1 for a bias) and cotangents G_{i,k,t} = dF_k / dz_{i,t} of the
raw convolution output (``kfac_ref.patches_and_cotangents``; the BN scale is inside G), the block's slice of the
Jacobian row of output k on example i is the per-example weight gradient, mat_l(J_i[k]) = At_i^T G_{i,k}, so in a
basis (V, Ub)

    T_{i,k} = V^T mat_l(J_i[k]) Ub = (At_i V)^T (G_{i,k} Ub),

and the block's term of u^T J_i Sigma J_i^T u under Sigma_l = (V (x) Ub) diag(R) (V (x) Ub)^T is
sum_{j,m} R[j][m] (sum_k u_k T_{i,k}[j][m])^2.  No Jacobian is formed here: ``tests/test_kfac_predict_sweep_cpu.py``
checks the identity against ``kfac_ref.predict_dense`` on the autograd Jacobian.
"""
import torch

import kfac_ref as kf

F64 = torch.float64


def projected_products(state, X, triples):
    """[T_l (n, K, Mt, N)] per block: (At_i V)^T (G_{i,k} Ub) for ``triples[l] = (V, R, Ub)`` (float64 CPU)"""
    _, ats, Gs = kf.patches_and_cotangents(state, X)
    out = []
    for at, G, (V, _, Ub) in zip(ats, Gs, triples):
        AV = at @ V                                                     # (n, T, Mt)
        GU = G @ Ub                                                     # (n, K, T, N)
        out.append(torch.einsum("itj,iktm->ikjm", AV, GU))
    return out


def block_terms(state, X, triples, U=None):
    """[(P, n)] per block: sum_{j,m} R[j][m] (sum_k U[p, i, k] T_{i,k}[j][m])^2; ``U`` None: the K one-hot probes, so
    entry [k, i] is the block's term of the variance of output k on example i"""
    out = []
    for T, (_, R, _) in zip(projected_products(state, X, triples), triples):
        if U is not None:
            T = torch.einsum("pik,ikjm->ipjm", torch.as_tensor(U, dtype=F64), T)
        out.append(torch.einsum("jm,ipjm->pi", R, T * T))
    return out


def block_covariances(state, X, triples):
    """[(n, K, K)] per block: sum_{j,m} R[j][m] T_{i,k}[j][m] T_{i,k'}[j][m]"""
    return [torch.einsum("ikjm,jm,iljm->ikl", T, R, T)
            for T, (_, R, _) in zip(projected_products(state, X, triples), triples)]


def remainder_covariance(J, rem, rem_var):
    """(n, K, K): the term of the parameters outside every block, from the Jacobian J (n, K, D)"""
    return torch.einsum("bkd,d,bmd->bkm", J[:, :, rem], rem_var, J[:, :, rem])


def predict_ref(state, X, triples, J, rem, rem_var):
    """(n, K, K) float64: the blocks' terms from patches and cotangents plus the remainder's from J"""
    return sum(block_covariances(state, X, triples)) + remainder_covariance(J, rem, rem_var)
