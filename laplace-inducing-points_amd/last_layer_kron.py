"""Kronecker-factored last-layer Laplace: the posterior of ``last_layer.py`` without its size cap.  Not a reference
function.

With phit_i = [1, phi_i] (Ft = F + 1 entries; the bias is feature 0) and theta_L = [bias (K), kernel (F, K) row-major],
flat index f K + k, the curvature is approximated by one Kronecker product of two Grams over the M bound examples,

    G_kron = c A (x) Bf,   A = sum_i phit_i phit_i^T (Ft, Ft),   Bf = sum_i diag(p_i) - p_i p_i^T  or  M I  (K, K),

c = recal / M with recal the N/M (x exp(-logvar)) factor of ``compute_ggn_vp``.  For the Gaussian head, and for M = 1,
G_kron is the dense last-layer GGN exactly.  Both factors come from what the primal pass has cached
(``lip_ll_kron_factors``: float64, no backward sweep, bitwise reproducible).

The prior is alpha I or a :class:`prior.GroupedPrior` whose restriction to theta_L is constant along k: a[(f, k)] = a_f.
With d = a_f^(-1/2), At = diag(d) A diag(d) = Ut diag(lam) Ut^T, Bf = Ub diag(mu) Ub^T, V = diag(d) Ut and
R[j][l] = 1 / (c lam_j mu_l + 1) the posterior covariance diagonalises exactly,

    S[(f,k)][(g,m)] = sum_{j,l} V[f][j] V[g][j] Ub[k][l] Ub[m][l] R[j][l],

so the fit is two ``eigh`` calls of sizes Ft and K, the predictive of a point is u = V^T phit, s_l = sum_j u_j^2 R[j][l],
cov = Ub diag(s) Ub^T (``lip_ll_kron_predict``) and a draw is dW = V (E o sqrt(R)) Ub^T.  The host algebra below is
float64 torch on the device of the factors and runs on CPU tensors as well.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _native as nv
from . import ggn as _ggn
from .distributions import KroneckerNormal, MultivariateNormalFullCovariance
from .last_layer import _engines, _recal, last_layer_slice
from .prior import check_dim, is_grouped
from .utils import flatten_nn_params


def prior_rows(alpha, off: int, F: int, K: int, D: int) -> torch.Tensor:
    """(F + 1,) float64 CPU: the prior precision a_f of row f of theta_L (row 0 the bias, row 1 + j kernel row j), from
    the group table alone.  Raises ``ValueError`` when a :class:`prior.GroupedPrior` varies along k within a row."""
    Ft = F + 1
    if not is_grouped(alpha):
        return torch.full((Ft,), float(alpha), dtype=torch.float64)
    check_dim(alpha, D)
    rows = torch.full((Ft,), float("nan"), dtype=torch.float64)
    for g, (name, segs) in enumerate(alpha.table):
        for o, n in segs:
            s, e = max(o, off) - off, min(o + n, off + Ft * K) - off
            if s >= e:
                continue
            seen = rows[s // K:(e + K - 1) // K]                    # every row this segment touches, whole or in part
            clash = ~torch.isnan(seen) & (seen != alpha.values[g])
            if bool(clash.any()):
                raise ValueError(f"prior group {name!r} gives row {s // K + int(clash.nonzero()[0])} of the last layer's "
                                 f"({Ft}, {K}) parameter block a second precision: the Kronecker-factored posterior needs "
                                 f"a prior that is constant along the K outputs of each row (one precision per tensor or "
                                 f"per layer is)")
            seen.fill_(float(alpha.values[g]))
    return rows


def centre(Bf: torch.Tensor) -> torch.Tensor:
    """C Bf C with C = I - 1 1^T / K: (diag(p) - p p^T) 1 = p (1 - sum p) = 0, but float32 probabilities sum to
    1 +- 6e-8 and leak that much into the exactly-null direction 1_K (see ``last_layer._spectrum_last_layer``)"""
    Bf = Bf - Bf.mean(dim=0, keepdim=True)
    return Bf - Bf.mean(dim=1, keepdim=True)


def _eigh(Mx: torch.Tensor):
    lam, U = torch.linalg.eigh(0.5 * (Mx + Mx.T))
    return lam.clamp_min(0.0), U


def factor_posterior(A: torch.Tensor, Bf: torch.Tensor, a_rows: torch.Tensor, c: float, classifier: bool):
    """``(V (Ft, Ft), R (Ft, K), Ub (K, K), lam (Ft,), mu (K,))`` of the module docstring from the two factors, the row
    precisions a_f and c; float64 on the device of ``A``"""
    A, Bf = A.double(), Bf.double().to(A.device)
    d = a_rows.to(device=A.device, dtype=torch.float64).rsqrt()
    lam, Ut = _eigh(d[:, None] * A * d[None, :])
    mu, Ub = _eigh(centre(Bf) if classifier else Bf)
    R = 1.0 / (c * lam[:, None] * mu[None, :] + 1.0)
    return (d[:, None] * Ut).contiguous(), R.contiguous(), Ub.contiguous(), lam, mu


def predictive_cov(phit: torch.Tensor, V: torch.Tensor, R: torch.Tensor, Ub: torch.Tensor, diag: bool) -> torch.Tensor:
    """the predictive of ``lip_ll_kron_predict`` in torch (any device): (B, K, K), or (B, K) for ``diag``"""
    s = (phit.double() @ V) ** 2 @ R
    if diag:
        return s @ (Ub * Ub).T
    return torch.einsum("kl,bl,ml->bkm", Ub, s, Ub)


def kron_spectrum(lam: torch.Tensor, mu: torch.Tensor, M: int) -> torch.Tensor:
    """the (Ft K,) spectrum outer(lam_A, mu_B) / M of A (x) Bf / M: what ``_lml_from_spectrum`` takes at N/M = 1"""
    return (lam[:, None] * mu[None, :] / M).reshape(-1)


def compute_kron_factors_last_layer(state, Z, model_type, example_chunk: Optional[int] = None):
    """``(A (F + 1, F + 1), Bf (K, K), M)``: the two unscaled factors summed over the M = len(Z) examples, float64 on the
    device (:meth:`LinearizedNet.last_layer_kron_factors`), chunked like :func:`last_layer.compute_ggn_last_layer`; all
    chunks add into one pair."""
    _, F, K = last_layer_slice(state, max_dim=None)
    engines = _engines(state, Z, model_type, None, example_chunk)
    dev = engines[0].device
    A = torch.zeros(F + 1, F + 1, device=dev, dtype=torch.float64)
    Bf = torch.zeros(K, K, device=dev, dtype=torch.float64)
    for eng in engines:
        eng.last_layer_kron_factors(A, Bf)
    return A, Bf, Z.shape[0]


def _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk):
    """(V, R, Ub, lam, mu, c) of the fitted posterior; the prior is checked before anything is allocated"""
    off, F, K = last_layer_slice(map_state, max_dim=None)
    D = flatten_nn_params(map_state.params)[0].numel()
    a_rows = prior_rows(alpha, off, F, K, D)
    A, Bf, M = compute_kron_factors_last_layer(map_state, Z, model_type, example_chunk=example_chunk)
    c = _recal(map_state, M, model_type, full_set_size) / M
    return factor_posterior(A, Bf, a_rows, c, model_type != "regressor") + (c,)


def posterior_lla_last_layer_kron(map_state, Z, model_type, alpha, full_set_size=None,
                                  example_chunk: Optional[int] = None) -> KroneckerNormal:
    """N(theta_MAP[slice], (c A (x) Bf + diag(a))^-1) over theta_L of the final Dense in factored form, float64 on the
    device; no size cap: nothing of size DL x DL is built."""
    off, F, K = last_layer_slice(map_state, max_dim=None)
    V, R, Ub, lam, mu, c = _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk)
    flat, _ = flatten_nn_params(map_state.params)
    loc = flat.detach()[off:off + (F + 1) * K].to(device=V.device, dtype=torch.float64)
    return KroneckerNormal(loc, V, R, Ub, spectrum=(lam, mu, c))


_FIT_CACHE = {}          # one entry, as last_layer._COV_CACHE


def _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk):
    """(V, R, Ub) fitted once per (binding, prior, N, chunking); ``clear_engine_cache`` drops the entry"""
    if _FIT_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_FIT_CACHE.clear)
    key = (_ggn.engine_key(map_state, Z, model_type), alpha.key() if is_grouped(alpha) else float(alpha), full_set_size,
           example_chunk)
    hit = _FIT_CACHE.get(key)
    if hit is None:
        fit = _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk)[:3]
        _FIT_CACHE.clear()
        hit = _FIT_CACHE[key] = (fit, (map_state.params, map_state.batch_stats, Z))
    return hit[0]


def _predict_cov(eng, V, R, Ub, diag: bool) -> torch.Tensor:
    _, F, K = eng.last_layer()
    cn = eng.cn
    phi = eng.prim[cn.a_off[cn.last_unit().src]:]
    out = torch.empty((eng.n, K) if diag else (eng.n, K, K), device=eng.device, dtype=torch.float64)
    doubles = C.c_int64(0)
    nv.check(eng.lib.lip_ll_kron_predict_scratch(eng.n, F, K, C.byref(doubles)), "lip_ll_kron_predict_scratch")
    scratch = torch.empty(max(1, doubles.value), device=eng.device, dtype=torch.float64)
    nv.check(eng.lib.lip_ll_kron_predict(phi.data_ptr(), F, eng.n, F, K, V.data_ptr(), R.data_ptr(), Ub.data_ptr(),
                                         out.data_ptr(), int(diag), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_ll_kron_predict")
    return out


def predict_lla_last_layer_kron(map_state, Xnew, Z, model_type, alpha, full_set_size=None, cov: str = "full",
                                batch: int = 256, example_chunk: Optional[int] = None):
    """Closed-form linearised predictive of :func:`posterior_lla_last_layer_kron` (``lip_ll_kron_predict``), in the return
    shapes and types of :func:`last_layer.predict_lla_last_layer`.  The posterior is fitted once per
    (state, Z, prior, N, chunking) across calls (a one-entry cache)."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    V, R, Ub = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk)
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        outs.append(_predict_cov(eng, V, R, Ub, cov == "diag"))
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def predict_lla_last_layer_kron_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1,
                                         example_chunk: Optional[int] = None) -> torch.Tensor:
    """Draws of the outputs under the factored posterior: f(x; theta_MAP) + phit(x) dW_s -> (S, B, K) float32, dW_s the
    zero-mean part of ``num_samples`` draws of :meth:`KroneckerNormal.sample` reshaped to (F + 1, K); no JVP."""
    _, F, K = last_layer_slice(map_state, max_dim=None)
    post = posterior_lla_last_layer_kron(map_state, Z, model_type, alpha, full_set_size=full_set_size,
                                         example_chunk=example_chunk)
    key = key if key is not None else 123
    dW = (post.sample((num_samples,), seed=key) - post.mean()).reshape(num_samples, F + 1, K)
    eng = _ggn.get_engine(map_state, Xnew, model_type)
    phi = eng.features().double()
    phit = torch.cat([torch.ones(eng.n, 1, device=phi.device, dtype=torch.float64), phi], dim=1)      # (B, F + 1)
    return (eng.outputs().double()[None] + phit @ dW).float()


def _spectrum_last_layer_kron(X, state, model_type) -> Tuple[torch.Tensor, int, float]:
    """eigenvalues (float64, clamped at 0) of G_kron built at N/M = 1, i.e. outer(lam_A, mu_B) / M (x exp(-logvar) for
    the regressor), DL, ||theta_L||^2: the triple of ``last_layer._spectrum_last_layer``, from two ``eigvalsh`` calls"""
    off, F, K = last_layer_slice(state, max_dim=None)
    DL = (F + 1) * K
    A, Bf, M = compute_kron_factors_last_layer(state, X, model_type)
    lam = torch.linalg.eigvalsh(0.5 * (A + A.T)).clamp_min(0.0)
    Bc = centre(Bf) if model_type != "regressor" else Bf
    mu = torch.linalg.eigvalsh(0.5 * (Bc + Bc.T)).clamp_min(0.0)
    spec = kron_spectrum(lam, mu, M)
    if model_type == "regressor":
        spec = spec * math.exp(-_ggn._logvar(state))
    flat, _ = flatten_nn_params(state.params)
    return spec, DL, float((flat.detach()[off:off + DL].double() ** 2).sum())
