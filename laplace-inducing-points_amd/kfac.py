"""Kronecker-factored Laplace over every layer (KFAC; KFC for convolutions): a Gaussian over the whole flat parameter
vector whose covariance is block-diagonal with one Kronecker-factored block per weight tensor.  Not a reference function.

A layer l is every unit of kind ``"conv"`` of the ``NetSpec`` (a Dense is a 1x1 convolution on a 1x1 map, a Dense on a
feature map an h x w VALID convolution with one output position).  Its block is the contiguous flat slice
[bias (N)] + kernel (M x N row-major), M = KH KW Cin in HWIO order, read as an (Mt, N) matrix with the bias as row 0
when the unit has one (``engine.kfac_block_table``).  With at_{i,t} the im2col patch of the layer's input at output
position t of example i (zero outside the image, a leading 1 for the bias) and g_{i,t,k} the cotangent of the raw
convolution output for column k of the square-root Hessian factor,

    A_l = sum_i sum_t at_{i,t} at_{i,t}^T  (Mt, Mt),    S_l = sum_i sum_t sum_k g_{i,t,k} g_{i,t,k}^T  (N, N),
    G_l = (recal / (M T_l)) A_l (x) S_l,

M the number of bound examples, T_l = OH OW and recal the N/M (x exp(-logvar)) factor of ``compute_ggn_vp``.  At
T_l = 1 this is c A (x) Bf of ``last_layer_kron.py``, and the final Dense block reproduces that module (its classifier
factor is centred as there).  A_l comes from the cached primal activations (``lip_kfac_input_gram``), every S_l from one
backward sweep of K one-hot probes (``lip_vjp_kron``); both are float64 Grams, bitwise reproducible.

Every parameter outside a layer block (BN scale and bias) gets the exact GGN diagonal of ``compute_ggn_diag`` and is
independent of everything else; a net without BN has no such parameter and runs no square-sum sweep.

The prior is a scalar alpha or a :class:`prior.GroupedPrior` that is constant along the N outputs of each row of each
block (the rule of ``last_layer_kron.prior_rows``).  The host algebra of a block is that module's
(``factor_posterior``, ``distributions.KroneckerNormal``).
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from . import ggn as _ggn
from .distributions import KFACNormal, KroneckerNormal
from .engine import KfacBlock, LinearizedNet, kfac_block_table
from .last_layer import _engines, _recal
from .last_layer_kron import factor_posterior, prior_rows
from .prior import check_dim, is_grouped
from .utils import flatten_nn_params, param_layout


def block_table(state) -> List[KfacBlock]:
    """the layer blocks of ``state.net`` from the layer program and ``param_layout`` alone (pure Python, no GPU)"""
    net = getattr(state, "net", None)
    if net is None:
        raise TypeError("the Kronecker-factored posterior needs state.net (a NetSpec layer program)")
    return kfac_block_table(net, {path: (o, shape) for path, o, shape in param_layout(state.params)})


def prior_rows_no_bias(alpha, off: int, M: int, N: int, D: int) -> torch.Tensor:
    """(M,) float64 CPU: :func:`last_layer_kron.prior_rows` for an (M, N) block without a bias row, row j kernel row j;
    raises ``ValueError`` when a :class:`prior.GroupedPrior` varies along the N outputs within a row"""
    if not is_grouped(alpha):
        return torch.full((M,), float(alpha), dtype=torch.float64)
    check_dim(alpha, D)
    rows = torch.full((M,), float("nan"), dtype=torch.float64)
    for g, (name, segs) in enumerate(alpha.table):
        for o, n in segs:
            s, e = max(o, off) - off, min(o + n, off + M * N) - off
            if s >= e:
                continue
            seen = rows[s // N:(e + N - 1) // N]
            clash = ~torch.isnan(seen) & (seen != alpha.values[g])
            if bool(clash.any()):
                raise ValueError(f"prior group {name!r} gives row {s // N + int(clash.nonzero()[0])} of the ({M}, {N}) "
                                 f"kernel block at flat offset {off} a second precision: the Kronecker-factored posterior "
                                 f"needs a prior that is constant along the N outputs of each row of each block")
            seen.fill_(float(alpha.values[g]))
    return rows


def block_prior_rows(alpha, b: KfacBlock, D: int) -> torch.Tensor:
    """(Mt,) row precisions of one block"""
    if b.bias:
        return prior_rows(alpha, b.off, b.Mt - 1, b.N, D)
    return prior_rows_no_bias(alpha, b.off, b.Mt, b.N, D)


def remainder_indices(blocks: List[KfacBlock], D: int) -> torch.Tensor:
    """sorted int64 CPU indices of the parameters outside every block"""
    keep = torch.ones(D, dtype=torch.bool)
    for b in blocks:
        keep[b.off:b.off + b.Mt * b.N] = False
    return keep.nonzero().reshape(-1)


def _remainder_prior(alpha, idx: torch.Tensor, D: int) -> torch.Tensor:
    if is_grouped(alpha):
        return check_dim(alpha, D).vector("cpu", torch.float64)[idx]
    return torch.full((idx.numel(),), float(alpha), dtype=torch.float64)


def compute_kfac_factors(state, Z, model_type, example_chunk: Optional[int] = None, class_chunk: Optional[int] = None, *,
                         curvature=None):
    """``(blocks, As, Ss, M)``: the layer blocks and their two unscaled factors summed over the M = len(Z) examples,
    float64 on the device (:meth:`LinearizedNet.kfac_factors`), chunked like
    :func:`last_layer_kron.compute_kron_factors_last_layer`; all chunks add into one pair per block.  ``curvature``
    (a spec of ``fisher.py``) builds the output factors S_l from that spec's raw cotangents, divided by its divisor,
    instead of the K one-hot probes; the input factors A_l are the same either way."""
    from . import fisher
    spec = fisher.checked(curvature, state, Z, model_type)
    blocks = block_table(state)
    engines = _engines(state, Z, model_type, None, example_chunk)
    dev = engines[0].device
    As = [torch.zeros(b.Mt, b.Mt, device=dev, dtype=torch.float64) for b in blocks]
    Ss = [torch.zeros(b.N, b.N, device=dev, dtype=torch.float64) for b in blocks]
    if spec is None:
        for eng in engines:
            eng.kfac_factors(As, Ss, class_chunk=class_chunk)
    else:
        source = fisher.source_for(spec, state, Z, model_type)
        for j, eng in enumerate(engines):
            U, divisor = source(eng, j * example_chunk if len(engines) > 1 else 0)
            eng.kfac_factors(As, Ss, class_chunk=class_chunk, probes=U, divisor=divisor)
    return engines[0].kfac_blocks(), As, Ss, Z.shape[0]


def fit_blocks(blocks, As, Ss, rows, recal: float, M: int, classifier: bool):
    """[(V, R, Ub, lam, mu, c)] per block from the factors and the row precisions: ``factor_posterior`` with
    c_l = recal / (M T_l); the final Dense block of a classifier is centred.  Float64 on the device of the factors
    (CPU included)."""
    return [factor_posterior(A, S, a, recal / (M * b.T), classifier and b.final) + (recal / (M * b.T),)
            for b, A, S, a in zip(blocks, As, Ss, rows)]


def block_eigenvalues(fits) -> List[torch.Tensor]:
    """[Ev (Mt, N)] = c outer(lam, mu) of the :func:`fit_blocks` tuples: the eigenvalues of every block's curvature in its
    whitened basis, R = 1 / (Ev + 1); what the grid predictive and :func:`rescale_fit` take next to (V, Ub)"""
    return [(c * lam[:, None] * mu[None, :]).contiguous() for _, _, _, lam, mu, c in fits]


def rescale_fit(triples, Evs, rem, s: float):
    """The fit at the prior s a from the fit at a, without any ``eigh``: for a common factor s > 0 the whitened factor
    D A D only scales, so the eigenvectors stay and the eigenvalues divide by s.  ``triples``: the (V, R, Ub) (or longer
    ``fit_blocks`` tuples; R is not read) of every block, ``Evs``: their eigenvalues in the whitened basis
    (:func:`block_eigenvalues`; ``recal * Lam.clamp_min(0)`` for EKFAC), ``rem`` = (indices, a_rem, h_rem): the remainder's
    parameters, their precisions at a and their curvature.  -> ``([(V / sqrt(s), 1 / (Ev / s + 1), Ub)], rem_var)``,
    the covariance V [1 / (Ev + s)] V^T (x) Ub Ub^T per block and 1 / (s a_d + h_d) for the remainder; float64 on the
    device of the operands (CPU included)."""
    s = float(s)
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"the scale of a prior must be a finite positive number, got {s!r}")
    out = [((f[0] / math.sqrt(s)).contiguous(), (1.0 / (Ev / s + 1.0)).contiguous(), f[2]) for f, Ev in zip(triples, Evs)]
    _, a_rem, h_rem = rem
    return out, 1.0 / (s * a_rem + h_rem)


class Fit(tuple):
    """The tuple a private ``_fit`` returns, unchanged in length and order, carrying next to it what the grid of prior
    precisions needs of the same fit: ``Evs``, every block's eigenvalues in its whitened basis, and ``h_rem``, the
    remainder's curvature.  With them the fit holds the posterior at every multiple of the prior (:func:`rescale_fit`)."""
    Evs = None
    h_rem = None

    @classmethod
    def of(cls, items, Evs, h_rem):
        out = cls(items)
        out.Evs, out.h_rem = Evs, h_rem
        return out


def _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, curvature=None):
    """(blocks, fits, rem_idx, rem_var, rem_prior), a :class:`Fit`; the prior is checked before anything is allocated"""
    blocks = block_table(map_state)
    D = flatten_nn_params(map_state.params)[0].numel()
    rows = [block_prior_rows(alpha, b, D) for b in blocks]
    rem = remainder_indices(blocks, D)
    a_rem = _remainder_prior(alpha, rem, D)
    blocks, As, Ss, M = compute_kfac_factors(map_state, Z, model_type, example_chunk=example_chunk, curvature=curvature)
    fits = fit_blocks(blocks, As, Ss, rows, _recal(map_state, M, model_type, full_set_size), M, model_type != "regressor")
    dev = As[0].device
    rem_var = h_rem = torch.zeros(0, device=dev, dtype=torch.float64)
    if rem.numel():
        diag = _ggn.compute_ggn_diag(map_state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk,
                                     curvature=curvature)
        h_rem = diag.double()[rem.to(dev)]
        rem_var = 1.0 / (a_rem.to(dev) + h_rem)
    return Fit.of((blocks, fits, rem.to(dev), rem_var, a_rem.to(dev)), block_eigenvalues(fits), h_rem)


def _prior_key(alpha):
    return alpha.key() if is_grouped(alpha) else float(alpha)


_FIT_CACHE = {}          # one entry, as last_layer_kron._FIT_CACHE


def _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, curvature=None):
    """the fit, computed once per (binding, prior, N, chunking, curvature spec); ``clear_engine_cache`` drops the entry"""
    if _FIT_CACHE.clear not in _ggn._CLEAR_HOOKS:
        _ggn._CLEAR_HOOKS.append(_FIT_CACHE.clear)
    key = (_ggn.engine_key(map_state, Z, model_type), _prior_key(alpha), full_set_size, example_chunk)
    if curvature is not None:
        from .fisher import spec_key
        if spec_key(curvature) is not None:
            key = key + (spec_key(curvature),)
    hit = _FIT_CACHE.get(key)
    if hit is None:
        fit = _fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, curvature)
        _FIT_CACHE.clear()
        hit = _FIT_CACHE[key] = (fit, (map_state.params, map_state.batch_stats, Z, curvature))
    return hit[0]


def posterior_from_fit(flat: torch.Tensor, blocks, fits, rem_idx, rem_var, rem_prior=None) -> KFACNormal:
    """the :class:`KFACNormal` of a fit, on the device of its factors (CPU included)"""
    dev = fits[0][0].device
    loc = flat.detach().to(device=dev, dtype=torch.float64)
    parts = [(b.off, KroneckerNormal(loc[b.off:b.off + b.Mt * b.N], V, R, Ub, spectrum=(lam, mu, c)))
             for b, (V, R, Ub, lam, mu, c) in zip(blocks, fits)]
    return KFACNormal(loc, parts, (rem_idx, rem_var), remainder_prior=rem_prior)


def posterior_lla_kfac(map_state, Z, model_type, alpha, full_set_size=None, example_chunk: Optional[int] = None, *,
                       curvature=None) -> KFACNormal:
    """N(theta_MAP, blockdiag((G_l + diag(a))^-1, remainder)) over the whole flat vector in factored form, float64 on
    the device; nothing of size D x D, and no Mt N x Mt N matrix, is built.  The fit is cached per
    (state, Z, prior, N, chunking, curvature spec) (a one-entry cache).  ``curvature``: a spec of ``fisher.py`` for the
    output factors and the remainder's diagonal (:func:`compute_kfac_factors`)."""
    blocks, fits, rem_idx, rem_var, rem_prior = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk,
                                                            curvature)
    flat, _ = flatten_nn_params(map_state.params)
    return posterior_from_fit(flat, blocks, fits, rem_idx, rem_var, rem_prior)


def predict_lla_kfac(map_state, Xnew, Z, model_type, alpha, full_set_size=None, cov: str = "full", batch: int = 256,
                     example_chunk: Optional[int] = None, *, curvature=None, route: Optional[str] = None):
    """Closed-form linearised predictive of :func:`posterior_lla_kfac`: mean f(x; theta_MAP) and
    sum_l J_l(x) Sigma_l J_l(x)^T + sum_d J_d(x)^2 var_d per test point (``lip_kfac_predict`` per layer block on the
    Jacobian rows of ``lip_vjp_rows``), in the return shapes and types of
    :func:`last_layer_kron.predict_lla_last_layer_kron`.  ``batch`` test points are bound at a time, fewer for
    ``cov="full"`` when their (K, batch, D) float32 rows would exceed 2 GiB.  ``route="sweep"`` forms the same sums
    inside one backward sweep per test batch without any Jacobian row (:func:`predictive_from_fit`); the default
    (None) is ``"rows"``."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    checked_route(route)
    _, fits, rem_idx, rem_var, _ = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, curvature)
    return predictive_from_fit(map_state, Xnew, model_type, [(V, R, Ub) for V, R, Ub, _, _, _ in fits], (rem_idx, rem_var),
                               cov, batch, **route_kwargs(route))


ROUTES = ("rows", "sweep")


def checked_route(route) -> str:
    """the route of a predictive, None standing for the default; ``ValueError`` for anything else"""
    route = "rows" if route is None else route
    if route not in ROUTES:
        raise ValueError(f"route must be 'rows' or 'sweep', got {route!r}")
    return route


def route_kwargs(route):
    """the keywords of :func:`predictive_from_fit` for a route: none for the default, so the rows route is called as it
    always was"""
    return {} if checked_route(route) == "rows" else {"route": route}


def predictive_from_fit(map_state, Xnew, model_type, triples, rem, cov: str, batch: int, route: str = "rows"):
    """the predictive of :func:`predict_lla_kfac` from the (V, R, Ub) of every block and the remainder's
    (indices, variances): :meth:`LinearizedNet.kfac_predict` on ``batch`` test points at a time.  ``route="sweep"``:
    :meth:`LinearizedNet.kfac_predict_sweep` instead, which forms no Jacobian row, so it has no row-block cap and does
    not reduce ``batch`` for ``cov="full"`` (which it takes for K <= 32 outputs, by polarisation); its sums are float32
    where the rows route multiplies in float64.  An unknown route raises ``ValueError`` before any engine is bound."""
    from .distributions import MultivariateNormalFullCovariance
    rem_idx, rem_var = rem
    sweep = checked_route(route) == "sweep"
    if sweep and cov == "full":
        from .lla import POLARISATION_MAX_K
        K = int(map_state.net.num_outputs)
        if K > POLARISATION_MAX_K:
            raise ValueError(f"cov='full' on the sweep route takes K (K + 1) / 2 probes per test batch: refused for K = {K} "
                             f"> {POLARISATION_MAX_K} outputs (use cov='diag')")
    if cov == "full" and not sweep:
        D = flatten_nn_params(map_state.params)[0].numel()
        fit = (LinearizedNet.ROW_BLOCK_BYTES // (4 * D)) // int(map_state.net.num_outputs)
        if fit < 1:
            raise ValueError("the K Jacobian rows of one test point exceed the row-block cap: use cov='diag'")
        batch = min(int(batch), fit)
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        predict = eng.kfac_predict_sweep if sweep else eng.kfac_predict
        outs.append(predict(triples, (rem_idx, rem_var), diag=cov == "diag"))
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def checked_scales(scales) -> List[float]:
    """the scales of a grid as floats; ``ValueError`` unless there is at least one and all are finite and positive"""
    vals = [float(s) for s in torch.as_tensor(scales, dtype=torch.float64).reshape(-1).tolist()]
    if not vals or not all(math.isfinite(s) and s > 0.0 for s in vals):
        raise ValueError("scales must be one or more finite positive numbers")
    return vals


def grid_predictive_from_fit(map_state, Xnew, model_type, triples, Evs, rem, scales, batch: int, route: str = "rows"):
    """the predictive of :func:`predict_lla_kfac_grid` from the (V, R, Ub) and Ev of every block and the remainder's
    (indices, a_rem, h_rem): :meth:`LinearizedNet.kfac_predict_grid` on ``batch`` test points at a time, one pass over
    their Jacobian rows for all scales.  ``route="sweep"``: :meth:`LinearizedNet.kfac_predict_sweep` once per scale on
    the triples of :func:`rescale_fit`, no Jacobian row and no refit."""
    scales = checked_scales(scales)
    sweep = checked_route(route) == "sweep"
    if sweep:
        rescaled = [rescale_fit(triples, Evs, rem, s) for s in scales]
    else:
        bases = [(f[0], f[2]) for f in triples]
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = _ggn.get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        if sweep:
            outs.append(torch.stack([eng.kfac_predict_sweep(t, (rem[0], var), diag=True) for t, var in rescaled]))
        else:
            outs.append(eng.kfac_predict_grid(bases, Evs, rem, scales))
        means.append(eng.outputs().double())
    f_mean, f_var = torch.cat(means), torch.cat(outs, dim=1)
    return (f_mean.squeeze(-1), f_var.squeeze(-1)) if model_type == "regressor" else (f_mean, f_var)


def predict_lla_kfac_grid(map_state, Xnew, Z, model_type, alpha, scales, full_set_size=None, batch: int = 256,
                          example_chunk: Optional[int] = None, *, curvature=None, route: Optional[str] = None):
    """:func:`predict_lla_kfac` (``cov="diag"``) at the priors s_g ``alpha`` for every s_g of ``scales`` at once:
    ``(f_mean (B, K), f_var (G, B, K))`` float64, (B,) and (G, B) for a regressor; ``alpha`` a scalar or a
    :class:`prior.GroupedPrior`, which every s_g multiplies as a whole.  The whitened factor of a block only scales with
    s, so ONE fit at ``alpha`` (cached as :func:`predict_lla_kfac`'s) and one projection T = V^T J Ub per test batch
    serve the whole grid: var_g = sum T^2 / (Ev + s_g) + sum_d J_d^2 / (s_g a_d + h_d) (``lip_kfac_predict_grid``).
    ``route="sweep"`` runs the row-free predictive once per scale on the rescaled fit instead (:func:`rescale_fit`);
    the default (None) is ``"rows"``."""
    checked_route(route)
    scales = checked_scales(scales)
    fit = _cached_fit(map_state, Z, model_type, alpha, full_set_size, example_chunk, curvature)
    _, fits, rem_idx, _, a_rem = fit
    return grid_predictive_from_fit(map_state, Xnew, model_type, [(V, R, Ub) for V, R, Ub, _, _, _ in fits], fit.Evs,
                                    (rem_idx, a_rem, fit.h_rem), scales, batch, **route_kwargs(route))


def predict_lla_kfac_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1,
                              example_chunk: Optional[int] = None, *, curvature=None) -> torch.Tensor:
    """Draws of the outputs under :func:`posterior_lla_kfac`: f(x; theta_MAP) + J(x) d_theta_s -> (S, B, K) float32,
    d_theta_s the zero-mean part of ``num_samples`` draws of :meth:`KFACNormal.sample` pushed through the engine's JVP
    ('raw'), as :func:`lla.predict_lla_diag_scalable` does.  This is the route for heads like ResNet-50's: K = 1000
    Jacobian rows per test point make the default closed form of :func:`predict_lla_kfac` impractical there (its
    ``route="sweep"`` forms no rows), while a draw costs one tangent-forward pass whatever K is."""
    post = posterior_lla_kfac(map_state, Z, model_type, alpha, full_set_size=full_set_size, example_chunk=example_chunk,
                              curvature=curvature)
    return draws_from_posterior(post, map_state, Xnew, model_type, key, num_samples)


def draws_from_posterior(post: KFACNormal, map_state, Xnew, model_type, key, num_samples) -> torch.Tensor:
    """f(x; theta_MAP) + J(x) d_theta_s for ``num_samples`` seeded draws of ``post`` through the engine's JVP"""
    key = key if key is not None else 123
    d_theta = post.sample((num_samples,), seed=key, dtype=torch.float64) - post.mean()
    eng = _ggn.get_engine(map_state, Xnew, model_type, workspace_bytes=4 << 30)
    return eng.outputs()[None] + eng.jvp(d_theta.float(), "raw")


def kfac_spectrum(blocks, As, Ss, M: int, classifier: bool) -> torch.Tensor:
    """the concatenation of outer(lam_l, mu_l) / (M T_l) over the blocks: the spectrum of blockdiag(A_l (x) S_l / (M T_l)),
    what ``_lml_from_spectrum`` takes at N/M = 1; the final classifier block centred.  Float64 on the factors' device."""
    from .last_layer_kron import centre
    parts = []
    for b, A, S in zip(blocks, As, Ss):
        S = centre(S) if (classifier and b.final) else S
        lam = torch.linalg.eigvalsh(0.5 * (A + A.T)).clamp_min(0.0)
        mu = torch.linalg.eigvalsh(0.5 * (S + S.T)).clamp_min(0.0)
        parts.append((lam[:, None] * mu[None, :] / (M * b.T)).reshape(-1))
    return torch.cat(parts)


def _spectrum_kfac(X, state, model_type, curvature=None) -> Tuple[torch.Tensor, int, float]:
    """eigenvalues (float64, clamped at 0) of the Kronecker-factored curvature built at N/M = 1 (x exp(-logvar) for the
    regressor) with the remainder's GGN diagonal appended, D, ||theta||^2"""
    blocks, As, Ss, M = compute_kfac_factors(state, X, model_type, curvature=curvature)
    spec = kfac_spectrum(blocks, As, Ss, M, model_type != "regressor")
    if model_type == "regressor":
        spec = spec * math.exp(-_ggn._logvar(state))
    flat, _ = flatten_nn_params(state.params)
    D = flat.numel()
    rem = remainder_indices(blocks, D)
    if rem.numel():
        diag = _ggn.compute_ggn_diag(state, X, model_type, curvature=curvature)
        spec = torch.cat([spec, diag.double()[rem.to(diag.device)].clamp_min(0.0)])
    return spec, D, float((flat.detach().double() ** 2).sum())
