"""Float64 yardstick of the last-layer Laplace posterior (CPU torch; no product code on its path).

With phit_i = [1, phi_i] the input of the final Dense and theta_L = [bias (K), kernel (F, K) row-major],

    G[(f K + k), (g K + l)] = sum_i phit_i[f] phit_i[g] H_i[k, l],   H_i = diag(p_i) - p_i p_i^T  or  I (regressor),

scaled by N/M (x exp(-logvar) for the regressor).  The features come from ``NetSpec.forward(return_all=True)`` in the
dtype of the state (float64 in the tests).  ``tests/test_last_layer_cpu.py`` checks this helper against the oracle's
dense GGN slice and autograd Jacobians; ``tests/test_last_layer.py`` uses it as the reference of the HIP path.
"""
import math

import torch
from torch.func import jacrev

from lip_amd.utils import flatten_nn_params, param_layout
from oracle.lla import _flat_apply

F64 = torch.float64


def final_unit(net):
    return net.units[-1]


def layout_of_final_dense(state):
    """(bias offset, bias shape, kernel offset, kernel shape) from ``param_layout``"""
    u = final_unit(state.net)
    lay = {path: (off, tuple(shape)) for path, off, shape in param_layout(state.params)}
    return lay[u.bias] + lay[u.kernel]


def features64(state, X):
    """(f (n, K), phit (n, F + 1), p (n, K) softmax of f) of the state's dtype"""
    net = state.net
    out, vals = net.forward(state.params, state.batch_stats, X, return_all=True)
    phi = vals[final_unit(net).src].reshape(X.shape[0], -1)
    phit = torch.cat([torch.ones(X.shape[0], 1, dtype=phi.dtype), phi], dim=1)
    return out.detach(), phit.detach(), torch.softmax(out, dim=-1).detach()


def recal(state, M, model_type, full_set_size=None):
    r = (full_set_size or M) / M
    if model_type == "regressor":
        r *= math.exp(-float(state.params["logvar"]["logvar"]))
    return r


def gram_from_operands(phit, p):
    """sum_i phit_i phit_i^T (x) (diag(p_i) - p_i p_i^T) in flat (f K + k) order"""
    n, Ft = phit.shape
    K = p.shape[1]
    H = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    return torch.einsum("if,ig,ikl->fkgl", phit, phit, H).reshape(Ft * K, Ft * K)


def gram_identity_head(phit, K):
    Ft = phit.shape[1]
    return torch.einsum("if,ig,kl->fkgl", phit, phit, torch.eye(K, dtype=phit.dtype)).reshape(Ft * K, Ft * K)


def ggn_last_layer_ref(state, Z, model_type, full_set_size=None):
    f, phit, p = features64(state, Z)
    G = gram_from_operands(phit, p) if model_type == "classifier" else gram_identity_head(phit, f.shape[1])
    return recal(state, Z.shape[0], model_type, full_set_size) * G


def covariance_ref(G, a):
    """(G + diag(a))^-1, ``a`` a scalar or a (DL,) vector"""
    DL = G.shape[0]
    A = torch.diag(torch.as_tensor(a, dtype=F64).expand(DL).clone())
    Sinv = G + A
    return torch.linalg.solve(0.5 * (Sinv + Sinv.T), torch.eye(DL, dtype=F64))


def predict_ref(state, Xnew, S):
    """(f (B, K), cov (B, K, K)) with cov_b[k, l] = sum_{f,g} phit_b[f] phit_b[g] S[(f, k), (g, l)]"""
    f, phit, _ = features64(state, Xnew)
    K = f.shape[1]
    Ft = phit.shape[1]
    cov = torch.einsum("bf,bg,fkgl->bkl", phit, phit, S.reshape(Ft, K, Ft, K))
    return f, cov


def jac64(state, X, model_type):
    """(f (n, K), J (n, K, D)) by autograd; inference mode, so example i's outputs depend on example i only"""
    flat, unravel = flatten_nn_params(state.params)
    fn = _flat_apply(state, unravel, model_type)
    n = X.shape[0]
    f = fn(flat, X).reshape(n, -1)
    J = torch.stack([jacrev(lambda fp: fn(fp, X[i:i + 1]).reshape(-1))(flat) for i in range(n)])
    return f.detach(), J.detach()


def lml_ref(alpha, lam, DL, theta2, rescale):
    """the value of ``train_alpha._lml_from_spectrum`` restated: -1/2 alpha ||theta||^2 - 1/2 sum log1p(rescale lam / alpha)"""
    x = rescale * lam / alpha
    return float(-0.5 * alpha * theta2 + 0.5 * DL * math.log(alpha) - 0.5 * (torch.log1p(x).sum() + DL * math.log(alpha)))
