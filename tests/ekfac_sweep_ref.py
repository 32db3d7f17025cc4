"""Float64 yardstick of the EKFAC second moments from backward sweeps (CPU torch; no product code on its path).

The two projections are plain float64 products of the up-cast float32 inputs, each with an absolute-value twin for the
summation bound:

    AV[(i,t)][j] = sum_e at_{i,t}[e] V[e][j],    GU[r][m] = sum_c G[r][c] Ub[c][m],

at_{i,t} the im2col patch of image i at output position t in (kh, kw, ci) order, zero outside the image, with a leading 1
when the layer has a bias.  The second moments under raw head cotangents U (P, n, K) are

    Lam_l = 1 / divisor sum_p sum_i (V^T mat_l(J_i^T u_pi) Ub)^2

from the autograd Jacobian of ``last_layer_ref.jac64``; with the exact-expectation cotangents of ``fisher_ref`` they are
``ekfac_ref.scales_ref`` (tests/test_ekfac_sweep_cpu.py).
"""
import torch

import ekfac_ref as er
import kfac_ref as kf

F64 = torch.float64


def patch_matrix(X, geom):
    """((n OH OW), Mt) float64 patches of the float32 NHWC tensor X for geom = (IH, IW, C, KH, KW, stride, pad_h, pad_w,
    OH, OW, bias)"""
    IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias = geom
    n = X.shape[0]
    X = X.double().cpu()
    Mt = KH * KW * C + bias
    at = torch.zeros(n, OH, OW, Mt, dtype=F64)
    if bias:
        at[..., 0] = 1.0
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(KH):
                for kw in range(KW):
                    ih, iw = oh * stride - pad_h + kh, ow * stride - pad_w + kw
                    if 0 <= ih < IH and 0 <= iw < IW:
                        e = bias + (kh * KW + kw) * C
                        at[:, oh, ow, e:e + C] = X[:, ih, iw, :]
    return at.reshape(n * OH * OW, Mt)


def project_patches_ref(X, geom, V):
    """(AV, |at| |V|): the float64 product and its absolute-value twin"""
    at = patch_matrix(X, geom)
    V = V.double().cpu()
    return at @ V, at.abs() @ V.abs()


def rows_project_ref(G, Ub):
    """(GU, |G| |Ub|) for float32 rows G (R, N)"""
    G, Ub = G.double().cpu(), Ub.double().cpu()
    return G @ Ub, G.abs() @ Ub.abs()


def scales_from_cotangents_ref(J, U, divisor, state, bases):
    """[Lam_l (Mt, N)] = 1 / divisor sum_p sum_i (V^T mat_l(J_i^T u_pi) Ub)^2 for J (n, K, D), U (P, n, K) and
    ``bases[l] = (V, Ub)`` (float64 CPU)"""
    U = torch.as_tensor(U, dtype=F64).reshape(-1, J.shape[0], J.shape[1])
    out = []
    for (_, off, Mt, N, _, _), (V, Ub) in zip(kf.blocks_of(state), bases):
        rows = torch.einsum("pik,ikjl->pijl", U, er.block_rows(J, off, Mt, N))
        T = V.T @ rows @ Ub
        out.append((T * T).sum((0, 1)) / float(divisor))
    return out
