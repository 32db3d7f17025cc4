"""Linearised-Laplace API — same call surface as the reference's ``src/lla.py``.

``compute_curvature_approx`` (``:11``), ``compute_curvature_approx_dense`` (``:26``),
``posterior_lla_dense`` (``:37``), ``predict_lla_dense`` (``:51``), ``predict_la_samples_dense``
(``:84``), ``predict_lla_scalable`` (``:133``), ``materialize_covariance`` (``:160``).
Network derivatives come from the HIP engine; the small dense solves use torch.linalg on the device
(SURVEY K10).
"""
from __future__ import annotations

import math

import torch

from .distributions import MultivariateNormalDiag, MultivariateNormalFullCovariance
from .engine import LinearizedNet
from .ggn import BlockOperator, compute_ggn_dense, compute_ggn_diag, compute_ggn_vp, get_engine
from .last_layer import (LAST_LAYER_MAX_DIM, posterior_lla_last_layer, predict_lla_last_layer,     # noqa: F401
                         predict_lla_last_layer_scalable)                                         # beside their diagonal twins
from .last_layer_kron import (posterior_lla_last_layer_kron, predict_lla_last_layer_kron,            # noqa: F401
                              predict_lla_last_layer_kron_scalable)
from .kfac import posterior_lla_kfac, predict_lla_kfac, predict_lla_kfac_grid, predict_lla_kfac_scalable   # noqa: F401
from .fisher import Cotangents, EmpiricalFisher, MCFisher, sample_head_cotangents                 # noqa: F401
from .ekfac import posterior_lla_ekfac, predict_lla_ekfac, predict_lla_ekfac_grid, predict_lla_ekfac_scalable   # noqa: F401
from .lowrank import posterior_lla_lowrank, predict_lla_lowrank, predict_lla_lowrank_scalable     # noqa: F401
from .subnetwork import (SUBNETWORK_MAX_DIM, posterior_lla_subnetwork, predict_lla_subnetwork,      # noqa: F401
                         predict_lla_subnetwork_scalable, subnetwork_indices)
from .link import LINKS, bridge_predictive, cholesky_semidefinite, link_predictive, mc_predictive   # noqa: F401
from .prior import check_dim, is_grouped
from .sample import sample, sample_diag
from .utils import flatten_nn_params


def compute_curvature_approx(map_state, Z, model_type, alpha, full_set_size=None):
    """``src/lla.py:11-23``: v -> GGN v + alpha v (alpha fused into the engine call).  With a
    :class:`prior.GroupedPrior` for ``alpha``: v -> GGN v + a (.) v (``lip_ggn_vp_diag``)."""
    vp = compute_ggn_vp(map_state, Z, model_type=model_type, full_set_size=full_set_size)
    eng = vp.engine
    M = Z.shape[0]
    N = full_set_size or M
    scale = N / M * (math.exp(-float(map_state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0)
    if is_grouped(alpha):
        from .ggn import attach_quadratic_forms_diag
        a = check_dim(alpha, eng.D).vector(eng.device)
        return attach_quadratic_forms_diag(BlockOperator(lambda V: eng.ggn_vp_diag(V, scale, a), (eng.D,), (eng.D,), eng,
                                                         "curvature_vp[grouped]"), eng, scale, a)
    from .ggn import attach_quadratic_forms
    return attach_quadratic_forms(BlockOperator(lambda V: eng.ggn_vp(V, scale, float(alpha)), (eng.D,), (eng.D,), eng, "curvature_vp"),
                                  eng, scale, float(alpha))


def compute_curvature_approx_dense(map_state, x, model_type, alpha, full_set_size=None):
    """``src/lla.py:26-34``: ``(GGN + alpha I, theta_MAP, unravel_fn)``."""
    GGN, flat_params_map, unravel_fn = compute_ggn_dense(map_state, x, model_type=model_type, full_set_size=full_set_size)
    GGN = GGN + alpha * torch.eye(GGN.shape[0], device=GGN.device, dtype=GGN.dtype)
    return GGN, flat_params_map, unravel_fn


def posterior_lla_dense(map_state, x, model_type, alpha, full_set_size=None, return_unravel_fn=False):
    """``src/lla.py:37-48``: N(theta_MAP, (GGN + alpha I)^-1); the solve runs in float64 on the device
    (the reference casts the mean to float64, ``:43``)."""
    S_inv, flat_params_map, unravel_fn = compute_curvature_approx_dense(
        map_state, x, model_type=model_type, alpha=alpha, full_set_size=full_set_size)
    S_inv = S_inv.double()
    S_inv = 0.5 * (S_inv + S_inv.T)
    S = torch.linalg.solve(S_inv, torch.eye(S_inv.shape[0], device=S_inv.device, dtype=torch.float64))
    dist = MultivariateNormalFullCovariance(loc=flat_params_map.double(), covariance_matrix=S)
    return (dist, unravel_fn) if return_unravel_fn else dist


def _jacobians(map_state, Xnew, model_type):
    """Per-test-point Jacobians (B, K, D) and outputs (B, K) from an engine bound to Xnew."""
    eng = get_engine(map_state, Xnew, model_type)
    B, K = eng.n, eng.K
    U = torch.zeros(B * K, B, K, device=eng.device, dtype=torch.float32)
    idx = torch.arange(B * K, device=eng.device)
    U[idx, idx // K, idx % K] = 1.0
    J = eng.vjp(U, "raw").reshape(B, K, eng.D)
    return J, eng.outputs()


def predict_lla_dense(map_state, Xnew, Z, model_type, alpha, full_set_size=None):
    """``src/lla.py:51-82``: f_cov_i = J_i S J_i^T per test point ((B, K, K); a diagonal (B, B) matrix for
    the regressor, ``:77``)."""
    S_inv, flat_params_map, _ = compute_curvature_approx_dense(map_state, Z, model_type=model_type, alpha=alpha,
                                                               full_set_size=full_set_size)
    S_inv = S_inv.double()
    S = torch.linalg.solve(0.5 * (S_inv + S_inv.T), torch.eye(S_inv.shape[0], device=S_inv.device, dtype=torch.float64))
    J, f = _jacobians(map_state, Xnew, model_type)
    J = J.double()
    f_mean = f.double().squeeze()
    f_cov = J @ S @ J.transpose(-1, -2)                       # (B, K, K)
    if model_type == "regressor":
        f_cov = torch.diag(f_cov.reshape(-1))
    return MultivariateNormalFullCovariance(loc=f_mean, covariance_matrix=f_cov)


def predict_la_samples_dense(map_state, Xnew, Z, model_type, alpha, full_set_size=None, num_mc_samples=100, key=None):
    """``src/lla.py:84-129``: non-linearised LA — sample theta ~ N(theta_MAP, S) and run the network
    (plotting helper in the reference; the forward passes use the torch functional NetSpec forward on
    the device)."""
    S_inv, flat_params_map, unravel_fn = compute_curvature_approx_dense(map_state, Z, model_type=model_type, alpha=alpha,
                                                                        full_set_size=full_set_size)
    dev = S_inv.device
    S = torch.linalg.inv(S_inv.double())
    dist = MultivariateNormalFullCovariance(flat_params_map.double(), S)
    flat_samples = dist.sample((num_mc_samples,), seed=0 if key is None else int(key)).float()
    net = map_state.net
    stats = {k: v for k, v in map_state.batch_stats.items()} if map_state.batch_stats else {}
    from .utils import tree_map
    stats = tree_map(lambda t: torch.as_tensor(t).to(dev, torch.float32), stats)
    X = Xnew.to(dev, torch.float32)
    outs = [net.forward(unravel_fn(fp), stats, X) for fp in flat_samples]
    out = torch.stack(outs)
    return out.squeeze(-1) if model_type == "regressor" else out


def predict_lla_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1, **sample_kw):
    """``src/lla.py:133-156``: f(x; theta_MAP) + J(x) w_s, w_s = sample(...)  -> (S, B, C).
    One engine is bound to the test batch; the S JVPs run as one tangent-forward block (the reference
    maps them sequentially, ``:154``).  ``sample_kw`` goes to :func:`sample` (``reference_compat=True`` for the
    reference's clipped small-space Lanczos)."""
    flat_params, _ = flatten_nn_params(map_state.params)
    D = flat_params.shape[0]
    key = key if key is not None else 123                                       # :136
    w_samples = sample(map_state, Z, D, alpha=alpha, key=key, model_type=model_type, num_samples=num_samples,
                       full_set_size=full_set_size, **sample_kw)
    eng = get_engine(map_state, Xnew, model_type, workspace_bytes=4 << 30)      # a per-batch binding: capped workspace
    fmu = eng.outputs()                                                         # (B, C)
    dys = eng.jvp(w_samples, "raw")                                             # (S, B, C)
    return fmu[None] + dys


def posterior_lla_diag(map_state, Z, model_type, alpha, full_set_size=None, *, curvature=None) -> MultivariateNormalDiag:
    """Diagonal Laplace posterior N(theta_MAP, diag(1 / (alpha + diag(GGN)))) with the GGN of
    :func:`compute_ggn_vp` (N/M, exp(-logvar)).  Not a reference function: the diagonal-LA baseline; its variances
    are the per-weight uncertainties.  ``curvature``: a spec of ``fisher.py`` (Monte-Carlo or empirical Fisher diagonal
    in place of the exact one)."""
    diag = compute_ggn_diag(map_state, Z, model_type, full_set_size=full_set_size, curvature=curvature)
    flat_params, _ = flatten_nn_params(map_state.params)
    loc = flat_params.detach().to(device=diag.device, dtype=diag.dtype)
    if is_grouped(alpha):
        return MultivariateNormalDiag(loc, variance=1.0 / (check_dim(alpha, diag.numel()).vector(diag.device) + diag))
    return MultivariateNormalDiag(loc, variance=1.0 / (float(alpha) + diag))


def predict_lla_diag_scalable(map_state, Xnew, Z, model_type, alpha, key=None, full_set_size=None, num_samples=1, *,
                              curvature=None):
    """:func:`predict_lla_scalable` with draws of the diagonal posterior (:func:`sample_diag`):
    f(x; theta_MAP) + J(x) w_s -> (S, B, C).  Not a reference function."""
    flat_params, _ = flatten_nn_params(map_state.params)
    D = flat_params.shape[0]
    key = key if key is not None else 123
    w_samples = sample_diag(map_state, Z, D, alpha=alpha, key=key, model_type=model_type, num_samples=num_samples,
                            full_set_size=full_set_size, curvature=curvature)
    eng = get_engine(map_state, Xnew, model_type, workspace_bytes=4 << 30)
    fmu = eng.outputs()
    dys = eng.jvp(w_samples, "raw")
    return fmu[None] + dys


def _cross_gram64(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A B^T for (a, D), (b, D) float32 factors with float64 accumulation (``lip_dot_nt_f64``)."""
    from . import krylov
    return krylov.dot_nt(A.contiguous(), B.contiguous())


def _factor_and_core(map_state, Z, model_type, alpha, full_set_size):
    """The factor Wm (d, D) of the inducing-point GGN and C = (alpha/beta I + Wm Wm^T)^-1 on range(Wm Wm^T) (float64):
    S = alpha^-1 (I - Wm^T C Wm).
    With a :class:`prior.GroupedPrior` (A = diag(a)): Gt = sum_g G_g / alpha_g = Wm A^-1 Wm^T, C = (I/beta + Gt)^-1 on
    range(Gt) with the same eigenvalue cut, S = A^-1 - A^-1 Wm^T C Wm A^-1 (Woodbury); the factor then comes back with
    its columns scaled, Wm A^-1, the only form the predictives use (one (d, D) block is held, not two)."""
    from .ggn import gram_from_factor, grouped_grams, materialize_factor
    eng_z = get_engine(map_state, Z, model_type)
    M = Z.shape[0]
    N = full_set_size or M
    beta = N / M
    c = math.exp(-0.5 * float(map_state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0
    Wm = materialize_factor(eng_z, c)                                   # (d, D)
    if is_grouped(alpha):
        grams = grouped_grams(Wm, check_dim(alpha, eng_z.D))
        Gt = (grams / alpha.values.to(grams.device)[:, None, None]).sum(0)
        lam, Ug = torch.linalg.eigh(0.5 * (Gt + Gt.T))
        keep = lam > 1e-6 * lam.max().clamp_min(1e-300)
        Cm = (Ug * torch.where(keep, 1.0 / (1.0 / beta + lam.clamp_min(0.0)), torch.zeros_like(lam))) @ Ug.T
        return Wm * (1.0 / alpha.vector(Wm.device, torch.float64)).float(), Cm
    Gd = gram_from_factor(Wm)
    # (alpha/beta I + Gd)^-1 restricted to range(Gd): on the null space of Gd (the classifier's factor has rank
    # M (K-1)) J W vanishes exactly, but its rounding error would be amplified by beta/alpha there
    lam, Ug = torch.linalg.eigh(0.5 * (Gd + Gd.T))
    keep = lam > 1e-6 * lam.max().clamp_min(1e-300)
    Cm = (Ug * torch.where(keep, 1.0 / (alpha / beta + lam.clamp_min(0.0)), torch.zeros_like(lam))) @ Ug.T
    return Wm, Cm


def predict_lla_marginals(map_state, Xnew, Z, model_type, alpha, full_set_size=None, batch: int = 64):
    """The exact linearised predictive of ``predict_lla_dense`` (``src/lla.py:51-82``) — mean f(x; theta_MAP) and the
    K x K covariance J(x) S J(x)^T per test point, S = (alpha I + beta W W^T)^-1 — without anything D x D:
    S = alpha^-1 (I - W (alpha/beta I + W^T W)^-1 W^T)  =>  J S J^T = alpha^-1 (J J^T - (J W) C (J W)^T).
    The Jacobian rows of a test batch come from ONE per-example backward sweep of K probes (``lip_vjp_rows``), J W is a
    float64-accumulated product against the factor.  Per-point marginals are what the Monte-Carlo estimates of
    ``predict_lla_scalable`` feed into (NLL, accuracy, Brier, ECE): this gives them exactly (no sampling noise in the
    covariance).  It is not faster than the sampled route at the CIFAR config (0.86 s against 0.34 s per 256-image
    batch with 200 draws: the float64 products dominate), so it is the reference point, not the default.
    Not a reference function (its scalable predictive is sample-based only); returned like ``predict_lla_dense``."""
    Wm, Cm = _factor_and_core(map_state, Z, model_type, alpha, full_set_size)
    d = Wm.shape[0]
    means, covs = [], []
    ia = (1.0 / alpha.vector(Wm.device, torch.float64)).float() if is_grouped(alpha) else None     # Wm is Wm A^-1 then
    for s0 in range(0, Xnew.shape[0], batch):
        Xb = Xnew[s0:s0 + batch]
        eng = get_engine(map_state, Xb, model_type)
        K = eng.K
        E = torch.eye(K, device=eng.device, dtype=torch.float32)[:, None, :].expand(K, eng.n, K).contiguous()
        J = eng.vjp_rows(E, "raw").permute(1, 0, 2)                     # (B, K, D)
        if ia is None:
            JJ = torch.stack([_cross_gram64(J[i], J[i]) for i in range(J.shape[0])])
            JW = _cross_gram64(J.reshape(-1, eng.D), Wm).reshape(eng.n, K, d)
            cov = (JJ - JW @ Cm @ JW.transpose(-1, -2)) / alpha
        else:
            # J S J^T = J A^-1 J^T - (J A^-1 Wm^T) C (.)^T: the rows scaled by 1 / a for the first product, the second
            # against the scaled factor
            Ja = J * ia
            JJ = torch.stack([_cross_gram64(Ja[i], J[i]) for i in range(J.shape[0])])
            JW = _cross_gram64(J.reshape(-1, eng.D), Wm).reshape(eng.n, K, d)
            cov = JJ - JW @ Cm @ JW.transpose(-1, -2)
        means.append(eng.outputs().double())
        covs.append(0.5 * (cov + cov.transpose(-1, -2)))
    f_mean, f_cov = torch.cat(means), torch.cat(covs)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_cov.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_cov)


POLARISATION_MAX_K = 32


def polarisation_probes(K: int):
    """The K (K + 1) / 2 output cotangents e_k + e_k' (k <= k') whose weighted norms determine a K x K quadratic form,
    and their index pairs: (P, K) float32 rows, (P,) k, (P,) k'."""
    ks, kps = torch.triu_indices(K, K)
    E = torch.zeros(ks.numel(), K)
    E[torch.arange(ks.numel()), ks] += 1.0
    E[torch.arange(ks.numel()), kps] += 1.0
    return E, ks, kps


def covariance_from_polarisation(q: torch.Tensor, ks: torch.Tensor, kps: torch.Tensor, K: int) -> torch.Tensor:
    """S (..., K, K) from q[..., j] = (e_k + e_k')^T S (e_k + e_k') over the pairs of :func:`polarisation_probes`:
    S_kk = q_kk / 4, S_kk' = (q_kk' - S_kk - S_k'k') / 2; float64, symmetric by construction."""
    q = q.double()
    diag_pos = (ks == kps).nonzero().squeeze(-1)
    sd = q[..., diag_pos] / 4.0                                         # (..., K): the pairs (k, k) come in k order
    off = (q - sd[..., ks] - sd[..., kps]) / 2.0
    S = torch.zeros(*q.shape[:-1], K, K, dtype=torch.float64, device=q.device)
    S[..., ks, kps] = off
    S[..., kps, ks] = off
    S[..., torch.arange(K), torch.arange(K)] = sd
    return S


def predict_lla_diag(map_state, Xnew, Z, model_type, alpha, full_set_size=None, cov: str = "diag", batch: int = 256, *,
                     curvature=None):
    """Closed-form linearised predictive of the diagonal posterior of :func:`posterior_lla_diag`: the mean
    f(x; theta_MAP) (B, K) and the variances var_k(x) = sum_d sigma_d^2 J(x)[k, d]^2 (B, K), float64 — what
    :func:`predict_lla_diag_scalable` estimates from draws, without draws.  One weighted-norm backward sweep of K
    one-hot probes per test batch (:meth:`LinearizedNet.vjp_wnorm`): no Jacobian rows are written.
    ``cov="full"`` returns the K x K covariances J diag(sigma^2) J^T as a ``MultivariateNormalFullCovariance`` like
    ``predict_lla_dense``, from the K (K + 1) / 2 probes e_k + e_k' of the same kernel (polarisation; K <= 32).
    A regressor comes back in the shapes of ``predict_lla_dense``: mean (B,), variances (B,) (``cov="full"``: the
    (B, B) diagonal matrix).  Not a reference function."""
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    w = posterior_lla_diag(map_state, Z, model_type, alpha, full_set_size=full_set_size, curvature=curvature).variance()
    means, outs = [], []
    for s0 in range(0, Xnew.shape[0], batch):
        eng = get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        K = eng.K
        if cov == "diag":
            E = torch.eye(K, device=eng.device, dtype=torch.float32)[:, None, :].expand(K, eng.n, K).contiguous()
            outs.append(eng.vjp_wnorm(E, w, "raw").T.double())                          # (B, K)
        else:
            if K > POLARISATION_MAX_K:
                raise ValueError(f"cov='full' takes K (K + 1) / 2 probes per test batch: refused for K = {K} > "
                                 f"{POLARISATION_MAX_K} outputs (use cov='diag')")
            E, ks, kps = polarisation_probes(K)
            U = E.to(eng.device)[:, None, :].expand(E.shape[0], eng.n, K).contiguous()
            q = eng.vjp_wnorm(U, w, "raw").T                                            # (B, K (K + 1) / 2)
            outs.append(covariance_from_polarisation(q, ks.to(eng.device), kps.to(eng.device), K))
        means.append(eng.outputs().double())
    f_mean, f_out = torch.cat(means), torch.cat(outs)
    if cov == "diag":
        return (f_mean.squeeze(-1), f_out.squeeze(-1)) if model_type == "regressor" else (f_mean, f_out)
    if model_type == "regressor":
        return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=torch.diag(f_out.reshape(-1)))
    return MultivariateNormalFullCovariance(loc=f_mean.squeeze(), covariance_matrix=f_out)


def predict_lla_variances(map_state, Xnew, Z, model_type, alpha, full_set_size=None, batch: int = 256):
    """Marginal variances of the inducing-point posterior: the mean f(x; theta_MAP) and the diagonal of the
    covariances :func:`predict_lla_marginals` returns, (B, K) float64 each, without the (B, K, D) Jacobian rows:
    var_k = (||J_k||^2 - (J W)_k C (J W)_k^T) / alpha.  ||J_k||^2 is the unweighted norm sweep of K one-hot probes
    (:meth:`LinearizedNet.vjp_wnorm`, ``w=None``), J W one tangent-forward block of the factor rows through the test
    batch's engine; the subtraction runs in float64.  Not a reference function."""
    Wm, Cm = _factor_and_core(map_state, Z, model_type, alpha, full_set_size)
    means, vars_ = [], []
    ia = None
    if is_grouped(alpha):
        # var_k = ||J_k||^2 in the A^-1 metric - (J A^-1 Wm^T)_k C (.)^T: the weighted-norm sweep with w = 1 / a and the
        # tangent-forward block of the factor scaled by 1 / a (what _factor_and_core returned, built once per call)
        ia = (1.0 / alpha.vector(Wm.device, torch.float64)).float()
    for s0 in range(0, Xnew.shape[0], batch):
        eng = get_engine(map_state, Xnew[s0:s0 + batch], model_type)
        K = eng.K
        E = torch.eye(K, device=eng.device, dtype=torch.float32)[:, None, :].expand(K, eng.n, K).contiguous()
        jj = eng.vjp_wnorm(E, ia, "raw").T.double()                                     # (B, K)
        JW = eng.jvp(Wm, "raw").permute(1, 2, 0).double()                               # (B, K, d)
        quad = ((JW @ Cm) * JW).sum(-1)
        vars_.append((jj - quad) / alpha if ia is None else jj - quad)
        means.append(eng.outputs().double())
    f_mean, f_var = torch.cat(means), torch.cat(vars_)
    return (f_mean.squeeze(-1), f_var.squeeze(-1)) if model_type == "regressor" else (f_mean, f_var)


def probit_predictive(f_mean: torch.Tensor, f_var: torch.Tensor, logvar=None):
    """Predictive of a Gaussian over the network outputs without draws.  Classifier (``logvar`` None): the probit
    approximation softmax(f / sqrt(1 + pi / 8 var)) -> class probabilities.  Regressor (``logvar`` = the observation
    noise log-variance): (mean, var + exp(logvar))."""
    if logvar is not None:
        return f_mean, f_var + math.exp(float(logvar))
    return torch.softmax(f_mean / torch.sqrt(1.0 + (math.pi / 8.0) * f_var), dim=-1)


def materialize_covariance(f_cov_vp, N, out_dim, mode="diag"):
    """``src/lla.py:160-217``: probe an operator with the K = N*out_dim basis vectors."""
    K = N * out_dim
    I = torch.eye(K, dtype=torch.float64)
    if mode == "diag":
        return torch.stack([torch.as_tensor(f_cov_vp(I[i])).reshape(K)[i] for i in range(K)]).reshape(N, out_dim)
    if mode == "full":
        return torch.stack([torch.as_tensor(f_cov_vp(I[i])).reshape(K) for i in range(K)], dim=1)
    raise ValueError("mode must be 'diag' or 'full'")
