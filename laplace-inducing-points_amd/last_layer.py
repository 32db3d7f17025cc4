"""Last-layer Laplace: a full, dense Gaussian over the final Dense layer, every earlier layer frozen at the MAP — the
baseline every Laplace comparison is run against.  Not a reference function.

With phit_i = [1, phi_i] the penultimate features and theta_L = [bias (K), kernel (F, K) row-major] (one contiguous
slice of the flat parameter vector, in this order), the GGN block is

    G[(f K + k), (g K + l)] = sum_i phit_i[f] phit_i[g] H_i[k, l],    H_i = diag(p_i) - p_i p_i^T  or  I,

a Kronecker-structured Gram of quantities the primal pass has cached already: the fit needs no backward sweep
(``lip_ll_ggn``, float64, streamed over example chunks).  The head is linear in theta_L, so the predictive covariance
of a test point is the quadratic form phit(x) (x) I_K applied to the posterior covariance (``lip_ll_predict``) and a
draw of the outputs is f(x) + phit(x) dW: no Jacobians, no JVPs.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _native as nv
from . import ggn as _ggn
from .distributions import MultivariateNormalFullCovariance
from .engine import last_layer_of
from .prior import check_dim, is_grouped
from .utils import flatten_nn_params, param_layout

LAST_LAYER_MAX_DIM = 8192


def last_layer_slice(state, max_dim: Optional[int] = LAST_LAYER_MAX_DIM) -> Tuple[int, int, int]:
    """``(offset, F, K)`` of the final Dense layer of ``state.net`` in the flat parameter vector, from the layer program
    and ``param_layout`` alone (pure Python, no GPU, nothing written).  Raises ``ValueError`` when the network does not
    end in a plain Dense, or when DL = (F + 1) K exceeds ``max_dim`` (``None``: no cap, for the factored posterior of
    ``last_layer_kron.py``) — before anything is allocated."""
    net = getattr(state, "net", None)
    if net is None:
        raise TypeError("the last-layer posterior needs state.net (a NetSpec layer program)")
    off, F, K = last_layer_of(net, {path: (o, shape) for path, o, shape in param_layout(state.params)})
    DL = (F + 1) * K
    if max_dim is not None and DL > max_dim:
        raise ValueError(f"the last layer has (F + 1) K = ({F} + 1) * {K} = {DL} parameters, more than "
                         f"LAST_LAYER_MAX_DIM = {max_dim}: a dense {DL} x {DL} covariance is not built; this is "
                         f"where a Kronecker-factored posterior is needed")
    return off, F, K


def _recal(state, M: int, model_type, full_set_size) -> float:
    """the N/M (x exp(-logvar) for the regressor) factor of ``compute_ggn_vp``"""
    recal = (full_set_size or M) / M
    if model_type == "regressor":
        recal *= math.exp(-_ggn._logvar(state))
    return recal


def _engines(state, Z, model_type, full_set_size, example_chunk):
    if example_chunk is None or example_chunk >= Z.shape[0]:
        return [_ggn.get_engine(state, Z, model_type)]
    return _ggn.ExampleChunkedGGN(state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk).engines


def compute_ggn_last_layer(state, Z, model_type, full_set_size=None, example_chunk: Optional[int] = None) -> torch.Tensor:
    """The GGN block of the final Dense layer, (N/M) sum_i phit_i phit_i^T (x) H_i (x exp(-logvar) for the regressor:
    the factors of :func:`ggn.compute_ggn_vp`) -> (DL, DL) float64 on the device, DL = (F + 1) K, rows and columns in
    the flat order of theta_L = theta[offset : offset + DL] (:func:`last_layer_slice`).  Accumulated in float64 from the
    cached features and probabilities of the primal pass (:meth:`LinearizedNet.last_layer_ggn`): no backward sweep,
    exactly symmetric, bitwise reproducible.  ``example_chunk`` binds the examples in chunks as
    :func:`ggn.compute_ggn_diag` does; all chunks add into one G."""
    _, F, K = last_layer_slice(state)
    recal = _recal(state, Z.shape[0], model_type, full_set_size)
    engines = _engines(state, Z, model_type, full_set_size, example_chunk)
    DL = (F + 1) * K
    G = torch.zeros(DL, DL, device=engines[0].device, dtype=torch.float64)
    for eng in engines:
        eng.last_layer_ggn(G)
    return G.mul_(recal)


def _prior_diag(alpha, off: int, DL: int, D: int, device) -> torch.Tensor:
    """(DL,) float64 diagonal of the prior precision A restricted to theta_L"""
    if is_grouped(alpha):
        return check_dim(alpha, D).vector(device, torch.float64)[off:off + DL]
    return torch.full((DL,), float(alpha), device=device, dtype=torch.float64)


def _covariance(G: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """(G + diag(a))^-1 in float64, symmetrised before the solve as in ``posterior_lla_dense``"""
    S_inv = G + torch.diag(a)
    S_inv = 0.5 * (S_inv + S_inv.T)
    return torch.linalg.solve(S_inv, torch.eye(S_inv.shape[0], device=S_inv.device, dtype=torch.float64))


def posterior_lla_last_layer(map_state, Z, model_type, alpha, full_set_size=None,
                             example_chunk: Optional[int] = None) -> MultivariateNormalFullCovariance:
    """N(theta_MAP[slice], (G + A)^-1) over theta_L = [bias, kernel] of the final Dense, float64 on the device; G of
    :func:`compute_ggn_last_layer`, A = alpha I or, for a :class:`prior.GroupedPrior`, diag(a[slice])."""
    off, F, K = last_layer_slice(map_state)
    DL = (F + 1) * K
    G = compute_ggn_last_layer(map_state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk)
    flat, _ = flatten_nn_params(map_state.params)
    S = _covariance(G, _prior_diag(alpha, off, DL, flat.numel(), G.device))
    loc = flat.detach()[off:off + DL].to(device=G.device, dtype=torch.float64)
    return MultivariateNormalFullCovariance(loc=loc, covariance_matrix=S)


_COV_CACHE = {}          # one entry: an evaluation loop calls predict once per loader batch with the same (state, Z)


def _cached_covariance(map_state, Z, model_type, alpha, full_set_size, example_chunk) -> torch.Tensor:
    """The fitted covariance (G + A)^-1, built once per (binding, prior, N, chunking), keyed like the sampler's parts
    (``sample._cached_parts``).  The entry holds the storage the key's pointers refer to, so they cannot be reused while
    it lives; ``clear_engine_cache`` drops it."""
    if _COV_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_COV_CACHE.clear)
    key = (_ggn.engine_key(map_state, Z, model_type), alpha.key() if is_grouped(alpha) else float(alpha), full_set_size,
           example_chunk)
    hit = _COV_CACHE.get(key)
    if hit is None:
        S = posterior_lla_last_layer(map_state, Z, model_type, alpha, full_set_size=full_set_size,
                                     example_chunk=example_chunk).covariance()
        _COV_CACHE.clear()
        hit = _COV_CACHE[key] = (S, (map_state.params, map_state.batch_stats, Z))
    return hit[0]


def _predict_cov(eng, S: torch.Tensor, diag: bool) -> torch.Tensor:
    """phit(x) (x) I_K applied to S for every point of the engine's binding: (B, K, K), or (B, K) for ``diag``"""
    _, F, K = eng.last_layer()
    cn = eng.cn
    phi = eng.prim[cn.a_off[cn.last_unit().src]:]
    out = torch.empty((eng.n, K) if diag else (eng.n, K, K), device=eng.device, dtype=torch.float64)
    nv.check(eng.lib.lip_ll_predict(phi.data_ptr(), F, eng.n, F, K, S.data_ptr(), out.data_ptr(), int(diag),
                                    nv.stream_ptr()), "lip_ll_predict")
    return out


def predict_lla_last_layer(map_state, Xnew, Z, model_type, alpha, full_set_size=None, cov: str = "full", batch: int = 256,
                           example_chunk: Optional[int] = None):
    """Closed-form linearised predictive of :func:`posterior_lla_last_layer`: mean f(x; theta_MAP) and the covariance
    (phit(x) (x) I_K)^T S (phit(x) (x) I_K) per test point (``lip_ll_predict``; the head is linear in theta_L, so this is
    J_L S J_L^T without Jacobians).  ``cov="full"`` returns what ``predict_lla_dense`` returns, a
    ``MultivariateNormalFullCovariance`` with (B, K, K) covariances (regressor: mean (B,), the (B, B) diagonal matrix);
    ``cov="diag"`` returns ``(mean, var)`` in the shapes of ``predict_lla_variances``.  The posterior is fitted once per
    call, and once per (state, Z, prior, N, chunking) across calls (a one-entry cache)."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    last_layer_slice(map_state)
    S = _cached_covariance(map_state, Z, model_type, alpha, full_set_size, example_chunk).contiguous()
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        outs.append(_predict_cov(eng, S, cov == "diag"))
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def predict_lla_last_layer_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1,
                                    example_chunk: Optional[int] = None) -> torch.Tensor:
    """Draws of the outputs under the last-layer posterior: f(x; theta_MAP) + phit(x) dW_s -> (S, B, K) float32, dW_s the
    zero-mean part of ``num_samples`` draws of the posterior's own ``.sample`` reshaped to (F + 1, K).  The head is
    linear in theta_L, so no JVP is needed."""
    _, F, K = last_layer_slice(map_state)
    post = posterior_lla_last_layer(map_state, Z, model_type, alpha, full_set_size=full_set_size,
                                    example_chunk=example_chunk)
    key = key if key is not None else 123
    dW = (post.sample((num_samples,), seed=key) - post.mean()).reshape(num_samples, F + 1, K)
    eng = _ggn.get_engine(map_state, Xnew, model_type)
    phi = eng.features().double()
    phit = torch.cat([torch.ones(eng.n, 1, device=phi.device, dtype=torch.float64), phi], dim=1)      # (B, F + 1)
    return (eng.outputs().double()[None] + phit @ dW).float()


def _spectrum_last_layer(X, state, model_type):
    """eigenvalues (float64, clamped at 0) of G built at N/M = 1, DL, ||theta_L||^2"""
    off, F, K = last_layer_slice(state)
    DL = (F + 1) * K
    G = compute_ggn_last_layer(state, X, model_type, full_set_size=None)
    if model_type != "regressor":
        # H_i 1 = p_i (1 - sum_k p_ik) = 0, so G vanishes on every x (x) 1_K.  The float32 probabilities sum to 1 +- 6e-8
        # and leak that much of lambda_max into those F + 1 directions, which log1p(r lambda / alpha) magnifies by
        # lambda_max / alpha: project them out, G <- P G P with P = I (x) (I_K - 1 1^T / K)
        G4 = G.reshape(F + 1, K, F + 1, K)
        G4 = G4 - G4.mean(dim=1, keepdim=True)
        G = (G4 - G4.mean(dim=3, keepdim=True)).reshape(DL, DL)
    lam = torch.linalg.eigvalsh(0.5 * (G + G.T)).clamp_min(0.0)
    flat, _ = flatten_nn_params(state.params)
    return lam, DL, float((flat.detach()[off:off + DL].double() ** 2).sum())
