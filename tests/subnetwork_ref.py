"""Float64 yardstick of the subnetwork Laplace posterior (CPU torch; no product code on its path).

With S an index set of the flat parameter vector, G_S = G[S][:, S] of the oracle's dense GGN, the posterior covariance is
(G_S + diag(a[S]))^-1 and the predictive covariance of a test point J[:, S] Sigma J[:, S]^T with the autograd Jacobians
``last_layer_ref.jac64`` forms the way ``oracle/lla.py`` forms them for ``predict_lla_dense``.
"""
import torch

from last_layer_ref import covariance_ref, jac64, lml_ref  # noqa: F401  (re-used as they are)
from lip_amd.utils import param_layout

F64 = torch.float64


def block(G, idx):
    """G[idx][:, idx]"""
    return G[idx][:, idx].contiguous()


def predict_ref(state, Xnew, model_type, idx, Sigma):
    """(f (B, K), cov (B, K, K)) with cov_b = J_b[:, idx] Sigma J_b[:, idx]^T"""
    f, J = jac64(state, Xnew, model_type)
    Js = J[:, :, idx]
    return f, torch.einsum("bka,ac,blc->bkl", Js, Sigma, Js)


def layers_by_hand(state, wanted):
    """the flat indices of the leaves whose path is in ``wanted`` (a set of path tuples), from ``param_layout``"""
    out = []
    for path, off, shape in param_layout(state.params):
        n = 1
        for s in shape:
            n *= int(s)
        if tuple(path) in wanted:
            out.extend(range(off, off + n))
    return torch.tensor(sorted(out), dtype=torch.int64)


def top_variances_ref(diag, a, size):
    """the ``size`` indices of largest 1 / (diag_j + a_j) by an explicit (variance descending, index ascending) sort"""
    var = 1.0 / (diag.to(F64) + torch.as_tensor(a, dtype=F64))
    order = sorted(range(var.numel()), key=lambda j: (-float(var[j]), j))
    return torch.tensor(sorted(order[:size]), dtype=torch.int64), var
