"""Subnetwork Laplace: a full, dense Gaussian over an arbitrary index set S of the flat parameter vector, every other
parameter frozen at the MAP.  Not a reference function.

    G[a, c] = (N/M) sum_i sum_k (J_i^T L_i e_k)[S_a] (J_i^T L_i e_k)[S_c]        (x exp(-logvar) for the regressor)

is the S x S block of the GGN of :func:`ggn.compute_ggn_vp`.  The per-example factor rows come from one backward sweep
of K one-hot probes (``lip_vjp_rows``) in class blocks; each block's S columns are gathered to a compact float32 panel
and Gram-multiplied in float64 on the matrix pipe (``lip_sub_gram``): no (M K, S) float64 copy, example chunks and
class chunks add into one G.  The predictive covariance of a test point is J_S(x) Sigma J_S(x)^T (``lip_sub_predict``)
and a draw of the outputs is f(x) + J_S(x) d_theta_S, the posterior draw scattered into a zero D-vector and pushed
through the engine's JVP.  The last-layer posterior (``last_layer.py``) is the special case S = the last-layer slice.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import ggn as _ggn
from .distributions import MultivariateNormalFullCovariance
from .engine import LinearizedNet
from .last_layer import _covariance, _engines, _recal
from .prior import check_dim, is_grouped
from .utils import flatten_nn_params, param_layout

SUBNETWORK_MAX_DIM = 8192


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _dim(state) -> int:
    return sum(_numel(shape) for _, _, shape in param_layout(state.params))


def check_indices(indices, D: int) -> torch.Tensor:
    """``indices`` as a sorted int64 CPU vector; raises ``ValueError`` for an empty set, more than
    ``SUBNETWORK_MAX_DIM`` entries (before anything of that size is built), a non-integer dtype, an entry outside
    [0, D) or a duplicate."""
    idx = torch.as_tensor(indices).detach().cpu().reshape(-1)
    if idx.numel() == 0:
        raise ValueError("the subnetwork is empty")
    if idx.numel() > SUBNETWORK_MAX_DIM:
        raise ValueError(f"the subnetwork has {idx.numel()} parameters, more than SUBNETWORK_MAX_DIM = "
                         f"{SUBNETWORK_MAX_DIM}: a dense {idx.numel()} x {idx.numel()} covariance is not built")
    if idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
        raise ValueError(f"subnetwork indices must be integers, got {idx.dtype}")
    idx = idx.to(torch.int64)
    if int(idx.min()) < 0 or int(idx.max()) >= D:
        raise ValueError(f"subnetwork indices must lie in [0, {D})")
    idx = torch.sort(idx).values
    if idx.numel() > 1 and bool((idx[1:] == idx[:-1]).any()):
        raise ValueError("subnetwork indices must be distinct")
    return idx


def _path_matcher(spec) -> Callable:
    if callable(spec):
        return spec
    prefixes = [spec] if isinstance(spec, (str, tuple)) else list(spec)
    if not prefixes:
        raise ValueError("'layers' needs at least one parameter-path prefix")

    def match(path):
        name = "/".join(str(p) for p in path)
        for pre in prefixes:
            if isinstance(pre, tuple):
                if tuple(path[:len(pre)]) == pre:
                    return True
            elif name == pre or name.startswith(str(pre).rstrip("/") + "/"):
                return True
        return False

    return match


def _prior_vector(alpha, D: int, device, dtype=torch.float64) -> torch.Tensor:
    """(D,) prior precisions of a scalar or a :class:`prior.GroupedPrior`"""
    if is_grouped(alpha):
        return check_dim(alpha, D).vector(device, dtype)
    if alpha is None:
        raise ValueError("'largest_variance' needs the prior precision alpha")
    return torch.full((D,), float(alpha), device=device, dtype=dtype)


def top_variances(diag: torch.Tensor, a: torch.Tensor, size: int) -> torch.Tensor:
    """indices of the ``size`` largest marginal variances 1 / (diag_j + a_j), ties to the lower index; sorted int64 CPU"""
    var = 1.0 / (diag.double() + a.double())
    order = torch.sort(var.cpu(), descending=True, stable=True).indices        # stable: equal variances keep index order
    return torch.sort(order[:size]).values


def subnetwork_indices(state, select, size=None, *, Z=None, model_type=None, alpha=None, full_set_size=None,
                       example_chunk: Optional[int] = None) -> torch.Tensor:
    """The index set of a subnetwork posterior: a sorted, distinct int64 CPU tensor of flat-parameter indices.

    ``select``: an explicit index tensor or list (validated, sorted); ``"layers"`` with ``size`` a list of
    parameter-path prefixes (tuples, or ``"/"``-joined strings) or a callable ``path -> bool`` over
    ``utils.param_layout`` — whole tensors; ``"largest_variance"``: the ``size`` parameters of largest marginal
    variance 1 / (diag_j + a_j) of the diagonal posterior (:func:`ggn.compute_ggn_diag` on ``Z``, ``alpha`` a scalar or
    a :class:`prior.GroupedPrior`), ties to the lower index.  More than ``SUBNETWORK_MAX_DIM`` indices raise before
    anything is allocated."""
    D = _dim(state)
    if not isinstance(select, str):
        return check_indices(select, D)
    if select == "layers":
        if size is None:
            raise ValueError("'layers' takes the path prefixes (or a callable path -> bool) as `size`")
        match = _path_matcher(size)
        segs = [(off, _numel(shape)) for path, off, shape in param_layout(state.params) if match(path) and _numel(shape)]
        total = sum(n for _, n in segs)
        if total == 0:
            raise ValueError("the 'layers' selection matches no parameter")
        if total > SUBNETWORK_MAX_DIM:
            raise ValueError(f"the selected layers hold {total} parameters, more than SUBNETWORK_MAX_DIM = "
                             f"{SUBNETWORK_MAX_DIM}")
        return check_indices(torch.cat([torch.arange(o, o + n, dtype=torch.int64) for o, n in segs]), D)
    if select == "largest_variance":
        if size is None or int(size) < 1 or int(size) > min(D, SUBNETWORK_MAX_DIM):
            raise ValueError(f"'largest_variance' needs 1 <= size <= min(D, SUBNETWORK_MAX_DIM) = "
                             f"{min(D, SUBNETWORK_MAX_DIM)}")
        if Z is None or model_type is None:
            raise ValueError("'largest_variance' needs Z and model_type")
        diag = _ggn.compute_ggn_diag(state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk)
        return top_variances(diag, _prior_vector(alpha, D, diag.device), int(size))
    raise ValueError("select must be an index tensor, 'layers' or 'largest_variance'")


def compute_ggn_subnetwork(state, Z, model_type, indices, full_set_size=None, example_chunk: Optional[int] = None,
                           class_chunk: Optional[int] = None) -> torch.Tensor:
    """The GGN block over ``indices``: ((N/M) sum_i J_i^T H_i J_i)[S][:, S] (x exp(-logvar) for the regressor: the
    factors of :func:`ggn.compute_ggn_vp`) -> (S, S) float64 on the device, rows and columns in the sorted order of
    :func:`check_indices`.  ``example_chunk`` binds the examples in chunks as :func:`ggn.compute_ggn_diag` does and
    ``class_chunk`` caps the probes per sweep; all chunks add into one G (:meth:`LinearizedNet.subnetwork_gram`)."""
    idx = check_indices(indices, _dim(state))
    recal = _recal(state, Z.shape[0], model_type, full_set_size)
    engines = _engines(state, Z, model_type, full_set_size, example_chunk)
    dev = engines[0].device
    G = torch.zeros(idx.numel(), idx.numel(), device=dev, dtype=torch.float64)
    idx_d = idx.to(dev)
    for eng in engines:
        eng.subnetwork_gram(idx_d, G, class_chunk=class_chunk)
    return G.mul_(recal)


def _prior_diag(alpha, idx: torch.Tensor, D: int, device) -> torch.Tensor:
    """(S,) float64 diagonal of the prior precision restricted to theta[idx]"""
    if is_grouped(alpha):
        return check_dim(alpha, D).vector(device, torch.float64)[idx.to(device)]
    return torch.full((idx.numel(),), float(alpha), device=device, dtype=torch.float64)


def posterior_from_ggn(G: torch.Tensor, alpha, idx: torch.Tensor, flat: torch.Tensor) -> MultivariateNormalFullCovariance:
    """N(theta[idx], (G + diag(a[idx]))^-1) from a given (S, S) float64 block, on the device of ``G`` (CPU included)"""
    S = _covariance(G, _prior_diag(alpha, idx, flat.numel(), G.device))
    loc = flat.detach()[idx].to(device=G.device, dtype=torch.float64)
    return MultivariateNormalFullCovariance(loc=loc, covariance_matrix=S)


def posterior_lla_subnetwork(map_state, Z, model_type, alpha, indices, full_set_size=None,
                             example_chunk: Optional[int] = None) -> MultivariateNormalFullCovariance:
    """N(theta_MAP[S], (G + A_S)^-1) over the parameters ``indices``, float64 on the device; G of
    :func:`compute_ggn_subnetwork`, A_S = alpha I or, for a :class:`prior.GroupedPrior`, diag(a[S])."""
    flat, _ = flatten_nn_params(map_state.params)
    idx = check_indices(indices, flat.numel())
    G = compute_ggn_subnetwork(map_state, Z, model_type, idx, full_set_size=full_set_size, example_chunk=example_chunk)
    return posterior_from_ggn(G, alpha, idx, flat)


_COV_CACHE = {}          # one entry, as last_layer._COV_CACHE


def _cached_covariance(map_state, Z, model_type, alpha, idx, full_set_size, example_chunk) -> torch.Tensor:
    """The fitted covariance, built once per (binding, prior, N, chunking, indices); ``clear_engine_cache`` drops it"""
    if _COV_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_COV_CACHE.clear)
    key = (_ggn.engine_key(map_state, Z, model_type), alpha.key() if is_grouped(alpha) else float(alpha), full_set_size,
           example_chunk, idx.numel(), hash(idx.numpy().tobytes()))
    hit = _COV_CACHE.get(key)
    if hit is None or not torch.equal(hit[1], idx):
        S = posterior_lla_subnetwork(map_state, Z, model_type, alpha, idx, full_set_size=full_set_size,
                                     example_chunk=example_chunk).covariance()
        _COV_CACHE.clear()
        hit = _COV_CACHE[key] = (S, idx.clone(), (map_state.params, map_state.batch_stats, Z))
    return hit[0]


def predict_lla_subnetwork(map_state, Xnew, Z, model_type, alpha, indices, full_set_size=None, cov: str = "full",
                           batch: int = 256, example_chunk: Optional[int] = None):
    """Closed-form linearised predictive of :func:`posterior_lla_subnetwork`: mean f(x; theta_MAP) and the covariance
    J_S(x) Sigma J_S(x)^T per test point (``lip_sub_predict``).  Return shapes and types are those of
    :func:`last_layer.predict_lla_last_layer`: ``cov="full"`` a ``MultivariateNormalFullCovariance`` with (B, K, K)
    covariances (regressor: mean (B,), the (B, B) diagonal matrix), ``cov="diag"`` ``(mean, var)``.  ``batch`` test points
    are bound at a time, fewer for ``cov="full"`` when their (K, batch, D) float32 rows would exceed 2 GiB.  The posterior is
    fitted once per (state, Z, prior, N, chunking, indices) across calls (a one-entry cache)."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    idx = check_indices(indices, _dim(map_state))
    S = _cached_covariance(map_state, Z, model_type, alpha, idx, full_set_size, example_chunk).contiguous()
    idx_d = idx.to(S.device)
    if cov == "full":
        # the full form reads all K rows of a point at once: bind no more points than one (K, n, D) row block holds
        # (LinearizedNet.subnetwork_predict would chunk over points itself, at one repeated sweep per chunk)
        fit = (LinearizedNet.ROW_BLOCK_BYTES // (4 * _dim(map_state))) // int(map_state.net.num_outputs)
        if fit < 1:
            raise ValueError("the K Jacobian rows of one test point exceed the row-block cap: use cov='diag'")
        batch = min(int(batch), fit)
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        outs.append(eng.subnetwork_predict(idx_d, S, cov == "diag"))
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def predict_lla_subnetwork_scalable(map_state, Xnew, Z, model_type, alpha, indices, key=None, full_set_size=None,
                                    num_samples=1, example_chunk: Optional[int] = None) -> torch.Tensor:
    """Draws of the outputs under the subnetwork posterior: f(x; theta_MAP) + J_S(x) d_theta_S -> (S, B, K) float32.  The
    zero-mean part of ``num_samples`` draws of the posterior's own ``.sample`` is scattered into zero (num_samples, D)
    vectors and pushed through the engine's JVP ('raw')."""
    flat, _ = flatten_nn_params(map_state.params)
    idx = check_indices(indices, flat.numel())
    post = posterior_lla_subnetwork(map_state, Z, model_type, alpha, idx, full_set_size=full_set_size,
                                    example_chunk=example_chunk)
    key = key if key is not None else 123
    d_theta = post.sample((num_samples,), seed=key) - post.mean()                      # (num_samples, S) float64
    eng = _ggn.get_engine(map_state, Xnew, model_type)
    V = torch.zeros(num_samples, eng.D, device=eng.device, dtype=torch.float32)
    V[:, idx.to(eng.device)] = d_theta.float()
    return eng.outputs()[None] + eng.jvp(V, "raw")


def _spectrum_subnetwork(X, state, model_type, indices):
    """eigenvalues (float64, clamped at 0) of G built at N/M = 1, |S|, ||theta_S||^2"""
    flat, _ = flatten_nn_params(state.params)
    idx = check_indices(indices, flat.numel())
    G = compute_ggn_subnetwork(state, X, model_type, idx, full_set_size=None)
    lam = torch.linalg.eigvalsh(0.5 * (G + G.T)).clamp_min(0.0)
    return lam, idx.numel(), float((flat.detach()[idx].double() ** 2).sum())
