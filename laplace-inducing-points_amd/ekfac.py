"""Eigenvalue-corrected Kronecker-factored Laplace over every layer (EKFAC; George et al., 2018): the posterior of
``kfac.py`` with every block's eigenvalues replaced by the exact second moments of the per-example gradients in the
block's Kronecker eigenbasis.  Not a reference function.

KFAC's block c_l A_l (x) S_l is exact for one example on a Dense layer only: for M > 1 it takes a product of sums for
a sum of Kronecker products, and for a convolution it also treats positions as uncorrelated.  EKFAC keeps the
eigenbasis Q_l = U_A (x) U_S of that block and replaces the eigenvalues lam_j mu_m by

    s*_{jm} = diag(Q_l^T G_l Q_l)_{(j,m)} = recal sum_i sum_k ((U_A^T mat_l(J_i^T L_i e_k) U_S)[j][m])^2,

G_l the exact GGN block, J_i^T L_i e_k the rows of the square-root factor (``lip_vjp_rows``, 'l') and mat_l the (Mt, N)
matrix of a row's slice.  Among all matrices Q_l diag(s) Q_l^T this one is nearest G_l in Frobenius norm, so the block is
never further from G_l than KFAC's and equals it wherever KFAC is exact.

With a prior diag(a) constant along each row, d = a^(-1/2), D = diag(d) (x) I, the fit is that of ``kfac.fit_blocks``
(V = d o U_t from the eigenvectors of D A D, Ub those of S, the final classifier block centred) followed by one pass
over the factor rows (:meth:`LinearizedNet.kfac_eigen_sqsums`, ``lip_kfac_eigen_sqsum``):

    Lam = sum_i sum_k (V^T mat_l(J_i^T L_i e_k) Ub)^2,    R = 1 / (recal Lam + 1).

The precision is D^-1 (D G D + I) D^-1 and diag((U_t (x) Ub)^T D G D (U_t (x) Ub)) = recal Lam, so the covariance is
(V (x) Ub) diag(R) (V (x) Ub)^T: a :class:`distributions.KroneckerNormal` like KFAC's with another R, and the
predictive (``lip_kfac_predict``), the draws and the JVP route run unchanged.  The parameters outside every block keep
the exact GGN diagonal.

Cost: the default fit (``moments="rows"``) needs the M K factor rows of width D once, in class blocks of at most
``ROW_BLOCK_BYTES``, next to the KFAC fit.  It is meant for heads with few outputs, like the closed-form KFAC predictive,
not for K = 1000.

``moments="sweep"`` forms the same Lam without any row: the block's slice of a row is the per-example weight gradient
At_i^T G_i diag(s) (At_i the im2col patches, G_i the cotangent rows of the layer, s the frozen BN scale), so
V^T mat_l(.) Ub = (At_i V)^T (G_i diag(s) Ub), and one backward sweep projects both operands per layer and square-sums the
per-(probe, example) products (:meth:`LinearizedNet.kfac_eigen_sqsums_sweep`, ``lip_vjp_eigen``).  That route also takes
the curvature specs of ``fisher.py`` (``curvature=``; the basis' KFAC factors and the remainder's diagonal then use the
same spec), which makes the fit usable at K = 1000.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from . import ggn as _ggn
from . import kfac as _kfac
from .distributions import KFACNormal, KroneckerNormal
from .last_layer import _engines, _recal
from .last_layer_kron import _eigh, centre
from .utils import flatten_nn_params


MOMENTS = ("rows", "sweep")


def _route(moments, curvature):
    """the checked ``moments`` of a fit: a curvature spec implies the sweep when ``moments`` is left at None, and is
    refused with the rows route; ``ValueError`` before anything is bound"""
    from . import fisher
    spec = fisher.resolve(curvature)
    if moments is None:
        moments = "rows" if spec is None else "sweep"
    if moments not in MOMENTS:
        raise ValueError(f"moments must be 'rows' or 'sweep', got {moments!r}")
    if spec is not None and moments == "rows":
        raise ValueError("a curvature spec is taken by moments='sweep' only: the rows route pushes the K one-hot probes "
                         "of the exact GGN")
    return moments


def compute_ekfac_scales(state, Z, model_type, bases, example_chunk: Optional[int] = None,
                         class_chunk: Optional[int] = None, *, moments: str = "rows", curvature=None) -> List[torch.Tensor]:
    """``[Lam_l (Mt, N)]``: sum_i sum_k (V_l^T mat_l(J_i^T L_i e_k) Ub_l)^2 over the M = len(Z) examples for the
    ``bases[l] = (V_l, Ub_l)`` of every layer block, float64 on the device, unscaled; chunked like
    :func:`kfac.compute_kfac_factors`, all chunks add into one matrix per block.  ``moments="rows"`` reads the factor
    rows (:meth:`LinearizedNet.kfac_eigen_sqsums`); ``moments="sweep"`` forms the same sums inside backward sweeps
    without any D-wide row (:meth:`LinearizedNet.kfac_eigen_sqsums_sweep`) and also takes a ``curvature`` spec of
    ``fisher.py``: (1 / divisor) sum_p sum_i (V_l^T mat_l(J_i^T u_pi) Ub_l)^2 over that spec's raw cotangents."""
    from . import fisher
    moments = _route(moments, curvature)
    spec = fisher.checked(curvature, state, Z, model_type)
    blocks = _kfac.block_table(state)
    engines = _engines(state, Z, model_type, None, example_chunk)
    dev = engines[0].device
    Lams = [torch.zeros(b.Mt, b.N, device=dev, dtype=torch.float64) for b in blocks]
    if moments == "rows":
        for eng in engines:
            eng.kfac_eigen_sqsums(bases, Lams, class_chunk=class_chunk)
    elif spec is None:
        for eng in engines:
            eng.kfac_eigen_sqsums_sweep(bases, Lams, class_chunk=class_chunk)
    else:
        source = fisher.source_for(spec, state, Z, model_type)
        for j, eng in enumerate(engines):
            U, divisor = source(eng, j * example_chunk if len(engines) > 1 else 0)
            eng.kfac_eigen_sqsums_sweep(bases, Lams, class_chunk=class_chunk, probes=U, divisor=divisor)
    return Lams


def corrected_fits(fits, Lams, recal: float):
    """[(V, R, Ub)] with R = 1 / (recal Lam + 1) from the ``kfac.fit_blocks`` tuples and the eigenbasis second moments
    (any device, CPU included)"""
    return [(f[0], (1.0 / (recal * Lam.clamp_min(0.0) + 1.0)).contiguous(), f[2]) for f, Lam in zip(fits, Lams)]


def block_eigenvalues(Lams, recal: float) -> List[torch.Tensor]:
    """[Ev (Mt, N)] = recal Lam clamped at 0: the corrected eigenvalues in the whitened basis, R = 1 / (Ev + 1)
    (:func:`corrected_fits`); what the grid predictive and ``kfac.rescale_fit`` take next to (V, Ub)"""
    return [(recal * Lam.clamp_min(0.0)).contiguous() for Lam in Lams]


def _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments="rows", curvature=None):
    """(blocks, [(V, R, Ub)], rem_idx, rem_var, rem_prior); the prior is checked before anything is allocated.  Under a
    curvature spec the KFAC factors that give the basis, the second moments and the remainder's diagonal all use it.
    The tuple is a ``kfac.Fit``: it carries Ev = recal Lam (clamped at 0) of every block, R = 1 / (Ev + 1), and the
    remainder's curvature for the grid of prior precisions."""
    blocks = _kfac.block_table(map_state)
    D = flatten_nn_params(map_state.params)[0].numel()
    rows = [_kfac.block_prior_rows(alpha, b, D) for b in blocks]
    rem = _kfac.remainder_indices(blocks, D)
    a_rem = _kfac._remainder_prior(alpha, rem, D)
    blocks, As, Ss, M = _kfac.compute_kfac_factors(map_state, Z, model_type, example_chunk=example_chunk, curvature=curvature)
    recal = _recal(map_state, M, model_type, full_set_size)
    kfits = _kfac.fit_blocks(blocks, As, Ss, rows, recal, M, model_type != "regressor")
    Lams = compute_ekfac_scales(map_state, Z, model_type, [(f[0], f[2]) for f in kfits], example_chunk=example_chunk,
                                **_route_kwargs(moments, curvature))
    fits = corrected_fits(kfits, Lams, recal)
    dev = As[0].device
    rem_var = h_rem = torch.zeros(0, device=dev, dtype=torch.float64)
    if rem.numel():
        diag = _ggn.compute_ggn_diag(map_state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk,
                                     curvature=curvature)
        h_rem = diag.double()[rem.to(dev)]
        rem_var = 1.0 / (a_rem.to(dev) + h_rem)
    return _kfac.Fit.of((blocks, fits, rem.to(dev), rem_var, a_rem.to(dev)), block_eigenvalues(Lams, recal), h_rem)


_FIT_CACHE = {}          # one entry, as kfac._FIT_CACHE


def _route_kwargs(moments, curvature):
    """the keywords of :func:`compute_ekfac_scales` for a route: none for the default, so the rows route is called as
    it always was"""
    kw = {}
    if moments != "rows":
        kw["moments"] = moments
    if curvature is not None:
        kw["curvature"] = curvature
    return kw


def _fit_key(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments, curvature):
    """the cache key of a fit: (binding, prior, N, chunking, moments route, curvature spec)"""
    from .fisher import spec_key
    return (_ggn.engine_key(map_state, Z, model_type), _kfac._prior_key(alpha), full_set_size, example_chunk, moments,
            spec_key(curvature))


def _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments=None, curvature=None):
    """the fit, computed once per (binding, prior, N, chunking, moments route, curvature spec); ``clear_engine_cache``
    drops the entry"""
    moments = _route(moments, curvature)
    if _FIT_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_FIT_CACHE.clear)
    key = _fit_key(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments, curvature)
    hit = _FIT_CACHE.get(key)
    if hit is None:
        fit = _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments, curvature)
        _FIT_CACHE.clear()
        hit = _FIT_CACHE[key] = (fit, (map_state.params, map_state.batch_stats, Z, curvature))
    return hit[0]


def posterior_from_fit(flat: torch.Tensor, blocks, fits, rem_idx, rem_var, rem_prior=None) -> KFACNormal:
    """the :class:`KFACNormal` of a fit, on the device of its factors (CPU included); the blocks carry no spectrum: R is
    not a product of eigenvalues"""
    dev = fits[0][0].device
    loc = flat.detach().to(device=dev, dtype=torch.float64)
    parts = [(b.off, KroneckerNormal(loc[b.off:b.off + b.Mt * b.N], V, R, Ub, spectrum=None))
             for b, (V, R, Ub) in zip(blocks, fits)]
    return KFACNormal(loc, parts, (rem_idx, rem_var), remainder_prior=rem_prior)


def posterior_lla_ekfac(map_state, Z, model_type, alpha, full_set_size=None, example_chunk: Optional[int] = None, *,
                        moments: Optional[str] = None, curvature=None) -> KFACNormal:
    """N(theta_MAP, blockdiag((V_l (x) Ub_l) diag(R_l) (V_l (x) Ub_l)^T, remainder)) over the whole flat vector in
    factored form, float64 on the device, R_l from the eigenbasis second moments of the module docstring; nothing of
    size D x D, and no Mt N x Mt N matrix, is built.  The fit is cached per (state, Z, prior, N, chunking, moments,
    curvature spec) (a one-entry cache).  ``moments``: "rows" (the default without a spec) or "sweep"
    (:func:`compute_ekfac_scales`); ``curvature``: a spec of ``fisher.py`` for the basis' factors, the second moments
    and the remainder's diagonal, which implies the sweep."""
    blocks, fits, rem_idx, rem_var, rem_prior = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk,
                                                            moments, curvature)
    flat, _ = flatten_nn_params(map_state.params)
    return posterior_from_fit(flat, blocks, fits, rem_idx, rem_var, rem_prior)


def predict_lla_ekfac(map_state, Xnew, Z, model_type, alpha, full_set_size=None, cov: str = "full", batch: int = 256,
                      example_chunk: Optional[int] = None, *, moments: Optional[str] = None, curvature=None,
                      route: Optional[str] = None):
    """Closed-form linearised predictive of :func:`posterior_lla_ekfac` (:meth:`LinearizedNet.kfac_predict` with the
    corrected R), in the return shapes and types, and with the batching and refusals, of :func:`kfac.predict_lla_kfac`;
    ``route="sweep"`` as there (:meth:`LinearizedNet.kfac_predict_sweep`: no Jacobian rows), independent of ``moments``
    and ``curvature``, which choose the fit."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    _kfac.checked_route(route)
    _, fits, rem_idx, rem_var, _ = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments,
                                               curvature)
    return _kfac.predictive_from_fit(map_state, Xnew, model_type, fits, (rem_idx, rem_var), cov, batch,
                                     **_kfac.route_kwargs(route))


def predict_lla_ekfac_grid(map_state, Xnew, Z, model_type, alpha, scales, full_set_size=None, batch: int = 256,
                           example_chunk: Optional[int] = None, *, moments: Optional[str] = None, curvature=None,
                           route: Optional[str] = None):
    """:func:`predict_lla_ekfac` (``cov="diag"``) at the priors s_g ``alpha`` for every s_g of ``scales`` at once, in
    the shapes of :func:`kfac.predict_lla_kfac_grid`: one fit at ``alpha`` (the basis and the second moments in it do
    not move with s: Lam -> Lam / s), one pass over the rows of a test batch, Ev = recal Lam clamped at 0.  ``moments``
    and ``curvature`` choose the fit, ``route`` the predictive, as in :func:`predict_lla_ekfac`."""
    _kfac.checked_route(route)
    scales = _kfac.checked_scales(scales)
    fit = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, moments, curvature)
    _, fits, rem_idx, _, a_rem = fit
    return _kfac.grid_predictive_from_fit(map_state, Xnew, model_type, fits, fit.Evs, (rem_idx, a_rem, fit.h_rem), scales,
                                          batch, **_kfac.route_kwargs(route))


def predict_lla_ekfac_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1,
                               example_chunk: Optional[int] = None, *, moments: Optional[str] = None,
                               curvature=None) -> torch.Tensor:
    """Draws of the outputs under :func:`posterior_lla_ekfac`: f(x; theta_MAP) + J(x) d_theta_s -> (S, B, K) float32
    through the engine's JVP, as :func:`kfac.predict_lla_kfac_scalable` draws them."""
    post = posterior_lla_ekfac(map_state, Z, model_type, alpha, full_set_size=full_set_size, example_chunk=example_chunk,
                               moments=moments, curvature=curvature)
    return _kfac.draws_from_posterior(post, map_state, Xnew, model_type, key, num_samples)


def orthonormal_bases(blocks, As, Ss, classifier: bool):
    """[(U_t, Ub)] per block: the eigenvectors of A_l and of S_l (the final classifier block centred), the basis of a
    scalar prior whatever its value; float64 on the factors' device"""
    return [(_eigh(A)[1].contiguous(), _eigh(centre(S) if (classifier and b.final) else S)[1].contiguous())
            for b, A, S in zip(blocks, As, Ss)]


def _spectrum_ekfac(X, state, model_type, *, moments: Optional[str] = None, curvature=None) -> Tuple[torch.Tensor, int, float]:
    """eigenvalues (float64, clamped at 0) of the eigenvalue-corrected curvature built at N/M = 1 (x exp(-logvar) for the
    regressor): the concatenation of Lam0_l, the second moments in the orthonormal basis U_t (x) Ub summed over the M
    examples (the diagonal of Q^T (sum_i J_i^T H_i J_i) Q, where KFAC has outer(lam_l, mu_l) / (M T_l)), with the
    remainder's GGN diagonal appended, D, ||theta||^2.  For a scalar prior the basis does not depend on alpha."""
    moments = _route(moments, curvature)
    blocks, As, Ss, M = _kfac.compute_kfac_factors(state, X, model_type, curvature=curvature)
    Lams = compute_ekfac_scales(state, X, model_type, orthonormal_bases(blocks, As, Ss, model_type != "regressor"),
                                **_route_kwargs(moments, curvature))
    spec = torch.cat([Lam.clamp_min(0.0).reshape(-1) for Lam in Lams])
    if model_type == "regressor":
        spec = spec * math.exp(-_ggn._logvar(state))
    flat, _ = flatten_nn_params(state.params)
    D = flat.numel()
    rem = _kfac.remainder_indices(blocks, D)
    if rem.numel():
        diag = _ggn.compute_ggn_diag(state, X, model_type, curvature=curvature)
        spec = torch.cat([spec, diag.double()[rem.to(diag.device)].clamp_min(0.0)])
    return spec, D, float((flat.detach().double() ** 2).sum())
