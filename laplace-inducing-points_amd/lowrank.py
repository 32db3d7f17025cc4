"""Low-rank Laplace over every parameter (``LowRankLaplace`` of the common libraries): the Gaussian whose precision is
the prior plus the leading eigenpairs of the GGN of a whole data set.  Not a reference function.

With the prior A0 = alpha I or diag(a) (a :class:`prior.GroupedPrior`) and G the GGN summed over the M = len(Z) examples
at N/M = 1 (x exp(-logvar) for the regressor: the convention of ``train_alpha._spectrum``), the fit finds the ``rank``
leading eigenpairs (lam_j, ut_j) of the whitened curvature A0^(-1/2) G A0^(-1/2) and the posterior is

    precision  = A0^(1/2) (I + (N/M) Ut^T diag(lam) Ut) A0^(1/2),
    covariance = A0^(-1/2) (I - Ut^T diag(s) Ut) A0^(-1/2),    s_j = lam_t_j / (1 + lam_t_j),   lam_t = (N/M) lam

(:class:`distributions.LowRankNormal`).  For a scalar prior the whitening is a number: the operator is G itself, ONE fit
serves every alpha and every N/M, and lam_t = (N/M) lam / alpha.  For a grouped prior the columns of the probe block
are scaled by a^(-1/2) before and after every product.  Unlike the Kronecker-factored and diagonal posteriors it keeps
the correlations between layers; unlike the last-layer and subnetwork ones it freezes nothing.  Every direction the fit
discards keeps the prior variance: truncation over-states the variance, never under-states it.

The fit is matrix-free (:func:`krylov.top_eigenpairs`): randomized block subspace iteration on the GGN-vector product
of the engine with P = rank + oversample probes per block, ``power_iters + 2`` passes over the data; every dense step is
a HIP primitive of ``krylov.py`` (CholeskyQR2 on ``lip_dot_nt_f64``, ``lip_rows_combine``).  Data sets larger than one
binding go through :class:`ggn.ExampleChunkedGGN` (``example_chunk``), which keeps the primal cache of EVERY chunk on the
device: data sets whose caches do not fit are out of scope.  Memory: U is 4 rank D bytes, next to three (P, D) float32
work blocks during the fit.

The closed-form predictive needs no Jacobian rows: var_k = J A0^-1 J^T - sum_j s_j (J A0^(-1/2) ut_j)^2, the first term
one weighted-norm backward sweep (``lip_vjp_wnorm``) and the second one tangent-forward block of the rows A0^(-1/2) ut_j
(scaled once per fit), subtracted in float64.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ggn as _ggn
from . import krylov
from .distributions import LowRankNormal, MultivariateNormalFullCovariance
from .last_layer import _recal
from .prior import check_dim, is_grouped
from .utils import flatten_nn_params

DEFAULT_RANK = 64


def ggn_operator(state, Z, model_type, example_chunk: Optional[int] = None, isq: Optional[torch.Tensor] = None):
    """the block operator V (P, D) -> V G of the GGN summed over the examples of Z at N/M = 1 (x exp(-logvar) for the
    regressor), through one engine or, with ``example_chunk`` < len(Z), :class:`ggn.ExampleChunkedGGN`; ``isq`` (D,)
    float32 on the device whitens it: V -> ((V o isq) G) o isq.  Returns ``(matvec, device)``."""
    M = Z.shape[0]
    if example_chunk is None or example_chunk >= M:
        eng = _ggn.get_engine(state, Z, model_type)
        scale = _recal(state, M, model_type, None)
        apply, dev = (lambda V: eng.ggn_vp(V, scale, 0.0)), eng.device
    else:
        # a probe workspace of the size of ``ggn.shared_workspace``: a 256-probe block then runs in one pass per chunk
        total = torch.cuda.get_device_properties(Z.device if Z.is_cuda else torch.device("cuda")).total_memory
        op = _ggn.ExampleChunkedGGN(state, Z, model_type, full_set_size=None, example_chunk=example_chunk,
                                    workspace_bytes=min(32 << 30, total // 8))
        apply, dev = (lambda V: op(V)), op.engine.device
    if isq is None:
        return apply, dev
    return (lambda V: apply(V * isq).mul_(isq)), dev


def compute_ggn_lowrank(state, Z, model_type, rank: int, prior=None, example_chunk: Optional[int] = None, **solver):
    """``(lam (r,) float64 descending, U (r, D) float32 orthonormal rows, info)``: the ``rank`` leading eigenpairs of
    a^(-1/2) G a^(-1/2), G the GGN summed over the M = len(Z) examples at N/M = 1 (x exp(-logvar) for the regressor) and
    ``a`` the vector of a :class:`prior.GroupedPrior`; with a scalar ``prior`` or none the operator is G itself (the
    whitening is then a division of ``lam``).  ``solver`` goes to :func:`krylov.top_eigenpairs` (``oversample``,
    ``power_iters``, ``seed``, ``probes``, ``rtol``).  ``example_chunk`` binds the examples in chunks whose primal caches
    all stay on the device."""
    if int(rank) < 1:
        raise ValueError(f"rank must be at least 1, got {rank}")
    D = flatten_nn_params(state.params)[0].numel()
    if is_grouped(prior):
        check_dim(prior, D)
    isq = None
    dev = Z.device if Z.is_cuda else torch.device("cuda")
    if is_grouped(prior):
        isq = prior.vector(dev, torch.float64).rsqrt().float()
    matvec, dev = ggn_operator(state, Z, model_type, example_chunk, isq)
    return krylov.top_eigenpairs(matvec, D, int(rank), device=dev, **solver)


_FIT_CACHE = {}          # one entry, as kfac._FIT_CACHE


def _solver_key(solver):
    return tuple((k, (v.data_ptr(), v._version, tuple(v.shape)) if torch.is_tensor(v) else v) for k, v in sorted(solver.items()))


def _cached_fit(state, Z, model_type, prior, rank, example_chunk, solver):
    """``(lam, U, info, Us)`` computed once per (binding, grouped prior, rank, chunking, solver arguments): a scalar
    prior is not part of the key (one fit serves every alpha).  ``Us`` = U o a^(-1/2), the scaled copy the predictive
    pushes through the tangent-forward pass, is U itself for a scalar prior.  ``clear_engine_cache`` drops the entry."""
    if _FIT_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_FIT_CACHE.clear)
    grouped = is_grouped(prior)
    key = (_ggn.engine_key(state, Z, model_type), prior.key() if grouped else None, int(rank), example_chunk, _solver_key(solver))
    hit = _FIT_CACHE.get(key)
    if hit is None:
        lam, U, info = compute_ggn_lowrank(state, Z, model_type, rank, prior=prior if grouped else None,
                                           example_chunk=example_chunk, **solver)
        Us = U * prior.vector(U.device, torch.float64).rsqrt().float() if grouped else U
        _FIT_CACHE.clear()
        hit = _FIT_CACHE[key] = ((lam, U, info, Us), (state.params, state.batch_stats, Z, solver))
    return hit[0]


def _whitened(lam: torch.Tensor, alpha, Z, full_set_size) -> torch.Tensor:
    """lam_t: (N/M) lam for a grouped prior (the operator was whitened), (N/M) lam / alpha for a scalar one"""
    nm = (full_set_size or Z.shape[0]) / Z.shape[0]
    return nm * lam if is_grouped(alpha) else nm * lam / float(alpha)


def posterior_lla_lowrank(map_state, Z, model_type, alpha, full_set_size=None, rank: int = DEFAULT_RANK,
                          example_chunk: Optional[int] = None, **solver) -> LowRankNormal:
    """N(theta_MAP, A0^(-1/2) (I - Ut^T diag(s) Ut) A0^(-1/2)) over the whole flat vector from the ``rank`` leading
    eigenpairs of the whitened GGN (module docstring), Ut float32 on the device; nothing of size D x D is built.  The fit
    is cached (a one-entry cache); for a scalar ``alpha`` it does not depend on alpha or ``full_set_size``."""
    lam, U, _, _ = _cached_fit(map_state, Z, model_type, alpha, rank, example_chunk, solver)
    flat, _ = flatten_nn_params(map_state.params)
    loc = flat.detach().to(device=U.device, dtype=torch.float64)
    prior = alpha.vector(U.device, torch.float64) if is_grouped(alpha) else float(alpha)
    return LowRankNormal(loc, U, _whitened(lam, alpha, Z, full_set_size), prior)


def predict_lla_lowrank(map_state, Xnew, Z, model_type, alpha, full_set_size=None, rank: int = DEFAULT_RANK,
                        cov: str = "diag", batch: int = 256, example_chunk: Optional[int] = None, **solver):
    """Closed-form linearised predictive of :func:`posterior_lla_lowrank`: the mean f(x; theta_MAP) and
    var_k = J_k A0^-1 J_k^T - sum_j s_j (J_k A0^(-1/2) ut_j)^2 per test point, float64, without Jacobian rows: the first
    term is the weighted-norm sweep of K one-hot probes (:meth:`LinearizedNet.vjp_wnorm`, weights 1 / a), the second one
    tangent-forward block of the scaled eigenvector rows through the test batch's engine; the subtraction runs in
    float64.  ``cov="full"`` returns the K x K covariances from the polarisation probes of :func:`lla.predict_lla_diag`
    (K <= 32).  Return shapes and types are those of :func:`lla.predict_lla_diag`, regressor included."""
    from .lla import POLARISATION_MAX_K, covariance_from_polarisation, polarisation_probes
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    K = int(map_state.net.num_outputs)
    if cov == "full" and K > POLARISATION_MAX_K:
        raise ValueError(f"cov='full' takes K (K + 1) / 2 probes per test batch: refused for K = {K} > "
                         f"{POLARISATION_MAX_K} outputs (use cov='diag')")
    lam, U, _, Us = _cached_fit(map_state, Z, model_type, alpha, rank, example_chunk, solver)
    lam_t = _whitened(lam, alpha, Z, full_set_size)
    s = lam_t / (1.0 + lam_t)
    grouped = is_grouped(alpha)
    ia = (1.0 / alpha.vector(U.device, torch.float64)).float() if grouped else None
    inv = 1.0 if grouped else 1.0 / float(alpha)          # a scalar prior scales both terms afterwards
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        if cov == "diag":
            E = torch.eye(K, device=eng.device, dtype=torch.float32)[:, None, :].expand(K, eng.n, K).contiguous()
            first = eng.vjp_wnorm(E, ia, "raw").T.double()                              # (B, K)
        else:
            E, ks, kps = polarisation_probes(K)
            Pr = E.to(eng.device)[:, None, :].expand(E.shape[0], eng.n, K).contiguous()
            first = covariance_from_polarisation(eng.vjp_wnorm(Pr, ia, "raw").T, ks.to(eng.device), kps.to(eng.device), K)
        if Us.shape[0]:
            JU = eng.jvp(Us, "raw").permute(1, 2, 0).double()                           # (B, K, r)
            second = (JU * JU * s).sum(-1) if cov == "diag" else torch.einsum("bkr,r,bmr->bkm", JU, s, JU)
            first = first - second
        outs.append(inv * first)
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    f_out = 0.5 * (f_out + f_out.transpose(-1, -2))
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def predict_lla_lowrank_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1,
                                 rank: int = DEFAULT_RANK, example_chunk: Optional[int] = None, **solver) -> torch.Tensor:
    """Draws of the outputs under :func:`posterior_lla_lowrank`: f(x; theta_MAP) + J(x) d_theta_s -> (S, B, K) float32
    through the engine's JVP, as :func:`kfac.predict_lla_kfac_scalable` draws them; the draws of the parameters are the
    two-pass scheme of :meth:`LowRankNormal.sample`."""
    from .kfac import draws_from_posterior
    post = posterior_lla_lowrank(map_state, Z, model_type, alpha, full_set_size=full_set_size, rank=rank,
                                 example_chunk=example_chunk, **solver)
    return draws_from_posterior(post, map_state, Xnew, model_type, key, num_samples)


def _spectrum_lowrank(X, state, model_type, rank: int = DEFAULT_RANK, example_chunk: Optional[int] = None,
                      **solver) -> Tuple[torch.Tensor, int, float]:
    """the ``rank`` leading eigenvalues (float64, clamped at 0) of the GGN built at N/M = 1 (x exp(-logvar) for the
    regressor), D, ||theta||^2: the truncated spectrum ``_lml_from_spectrum`` takes; the directions left out count as
    flat (log1p(0) = 0), so the evidence's log-determinant is a lower bound of the full one.  The fit is the cached one of
    the posterior (scalar prior)."""
    lam, _, _, _ = _cached_fit(state, X, model_type, None, rank, example_chunk, solver)
    flat, _ = flatten_nn_params(state.params)
    return lam, flat.numel(), float((flat.detach().double() ** 2).sum())
