"""Log-marginal-likelihood in the prior precision alpha — the reference's ``src/train_alpha.py`` ("next" row N2).

``log_marginal_likelihood`` (``:13-44``), ``update_alpha`` (``:47-59``), ``train_map_then_alpha`` (``:65-121``: MAP steps
on theta interleaved with hyper-steps on alpha) and ``fit_alpha`` (its alpha hyper-steps for a fixed theta).

  log p(D | alpha) = -1/2 alpha ||theta||^2 + 1/2 D log alpha - 1/2 [ log det(I_d + (N/n)/alpha W^T W) + D log alpha ]

W^T W does not depend on alpha, so after ONE Gram (d engine rows + a float64 GEMM) and ONE eigendecomposition the
value and the exact gradient w.r.t. log alpha are O(d) scalar formulas — the reference rebuilds the Gram with
d x (M VJP + M JVP) network passes inside every ``jax.grad`` call (``:32,56``).

Layer-wise precisions (``*_layerwise``, not reference functions): with A = diag(a), a_j = alpha_{g(j)},
det(A + r W W^T) = prod_g alpha_g^{D_g} det(I_d + r sum_g G_g / alpha_g) with the per-group Grams G_g of
``ggn.grouped_grams`` — again independent of the precisions, so ONE pass over the materialised factor is followed by
d x d float64 algebra per evaluation (a Cholesky factorisation) for the value and the exact gradient in all log alpha_g.

``grid_search_alpha`` is the reference's validation grid search (``src/grid_search.py:9-88``); for the closed-form KFAC
and EKFAC posteriors the whole grid comes from one fit and one pass per validation batch (``kfac.predict_lla_kfac_grid``).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import torch

from .ggn import build_WTW, compute_W_vps, get_engine, grouped_grams, materialize_factor
from .prior import GroupedPrior
from .utils import count_model_params, flatten_nn_params


def _spectrum(X, state, model_type):
    """eigenvalues (float64, clamped at 0) of W^T W built at N/M = 1 (``:28-32``), D, ||theta||^2"""
    W, WT = compute_W_vps(state, X, model_type, full_set_size=None)
    inner = WT.out_shape
    d = math.prod(inner)
    WTW = build_WTW(W, WT, inner, d, dtype=torch.float64, block=1)
    lam = torch.linalg.eigvalsh(WTW).clamp_min(0.0)
    flat_p, _ = flatten_nn_params(state.params)
    D = flat_p.numel()
    return lam, D, float((flat_p.double() ** 2).sum())


def _lml_from_spectrum(alpha: float, lam: torch.Tensor, D: int, theta2: float, rescale: float):
    x = rescale * lam / alpha
    logdet_lowrank = torch.log1p(x).sum()
    logdet_term = logdet_lowrank + D * math.log(alpha)                     # :36
    log_prior = -0.5 * alpha * theta2 + 0.5 * D * math.log(alpha)          # :40-42
    value = log_prior - 0.5 * logdet_term                                  # :44
    # d/d(log alpha): -1/2 alpha ||theta||^2 + 1/2 sum_i x_i / (1 + x_i)
    grad_log_alpha = -0.5 * alpha * theta2 + 0.5 * (x / (1.0 + x)).sum()
    return float(value), float(grad_log_alpha)


def log_marginal_likelihood(alpha, X, state, model_type: str, full_set_size: Optional[int] = None) -> float:
    """``src/train_alpha.py:13-44``: log p(D|alpha) up to alpha-independent constants."""
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum(X, state, model_type)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])[0]


def log_marginal_likelihood_and_grad(alpha, X, state, model_type, full_set_size=None) -> Tuple[float, float]:
    """value and d/d(log alpha) (what ``jax.grad(loss_fn)(log_alpha)`` differentiates, ``:54-56``)"""
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum(X, state, model_type)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])


@dataclasses.dataclass
class Adam:
    """optax.adam(lr) restated for a scalar (b1 = 0.9, b2 = 0.999, eps = 1e-8, eps_root = 0)."""
    lr: float
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8

    def init(self, _param=None):
        return dict(count=0, mu=0.0, nu=0.0)

    def update(self, grad: float, opt_state):
        c = opt_state["count"] + 1
        mu = self.b1 * opt_state["mu"] + (1 - self.b1) * grad
        nu = self.b2 * opt_state["nu"] + (1 - self.b2) * grad * grad
        mu_hat, nu_hat = mu / (1 - self.b1 ** c), nu / (1 - self.b2 ** c)
        return -self.lr * mu_hat / (math.sqrt(nu_hat) + self.eps), dict(count=c, mu=mu, nu=nu)


def update_alpha(log_alpha: float, opt_state, opt: Adam, *lm_args):
    """``src/train_alpha.py:47-59``: one Adam step of gradient *ascent* on log alpha (descent on -L)."""
    _, g = log_marginal_likelihood_and_grad(math.exp(log_alpha), *lm_args)
    upd, new_state = opt.update(-g, opt_state)
    return log_alpha + upd, new_state


def _fit_from_spectrum(lam, D, theta2, rescale, alpha0, alpha_lr, steps):
    """``steps`` Adam ascent steps on log alpha from a spectrum: ``(alpha, [(alpha, value) before each step])``"""
    opt = Adam(alpha_lr)
    st = opt.init()
    la = math.log(alpha0)
    history = []
    for _ in range(steps):
        v, g = _lml_from_spectrum(math.exp(la), lam, D, theta2, rescale)
        history.append((math.exp(la), v))
        upd, st = opt.update(-g, st)
        la += upd
    return math.exp(la), history


def fit_alpha(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2, steps: int = 200):
    """The alpha hyper-steps of ``train_map_then_alpha`` (``:76-78,91-100``) for a fixed theta; the spectrum of
    W^T W is computed once and reused by every step."""
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum(X, state, model_type)
    return _fit_from_spectrum(lam, D, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def train_map_then_alpha(state, train_loader, test_loader, *, model_type: str, num_epochs: int = 500, alpha0: float = 1.0,
                         alpha_lr: float = 5e-2, alpha_every: int = 5, burnin: int = 100, full_set_size: Optional[int] = None,
                         optimizer=None, log=None):
    """``src/train_alpha.py:65-121``: every epoch runs the MAP steps of ``train_map.MapTrainer`` over ``train_loader`` at
    the prior precision exp(log_alpha); after epoch ``e >= burnin`` with ``(e + 1) % alpha_every == 0`` one hyper-step
    (:func:`update_alpha`) moves log_alpha on the evidence of the epoch's LAST batch at the current state.  Returns
    ``(state, alpha)``.  ``optimizer``: the ``train_map.Adam`` of the MAP steps (default ``Adam(1e-3)``).  ``log``, when
    given, is called after every epoch with ``dict(epoch, train_loss, alpha, hyper_state, hyper_batch)`` (the state and
    batch of the epoch's hyper-step, or None) and, every fourth epoch as in the reference, ``test_nll`` / ``test_acc`` of
    ``test_loader`` in eval mode."""
    from .train_map import MapTrainer
    log_alpha = math.log(alpha0)
    opt_h = Adam(alpha_lr)
    opt_hs = opt_h.init()
    trainer = MapTrainer(state, model_type, alpha0, optimizer)
    for epoch in range(int(num_epochs)):
        trainer.set_alpha(math.exp(log_alpha))
        loss, last = float("nan"), None
        for x, y in train_loader:
            loss = trainer.step(x, y)
            last = x
        hyper_state = None
        if last is not None and epoch >= burnin and (epoch + 1) % alpha_every == 0:
            hyper_state = trainer.state()
            log_alpha, opt_hs = update_alpha(log_alpha, opt_hs, opt_h, last, hyper_state, model_type, full_set_size)
        if log is not None:
            rec = dict(epoch=epoch, train_loss=loss, alpha=math.exp(log_alpha), hyper_state=hyper_state,
                       hyper_batch=last if hyper_state is not None else None)
            if epoch % 4 == 0:
                rec["test_nll"], rec["test_acc"] = trainer.evaluate(test_loader)
            log(rec)
    return trainer.state(), math.exp(log_alpha)


def log_marginal_likelihood_last_layer(alpha, X, state, model_type: str, full_set_size: Optional[int] = None) -> float:
    """:func:`log_marginal_likelihood` of the last-layer model (every earlier layer frozen): the spectrum is that of the
    dense last-layer GGN (``last_layer.compute_ggn_last_layer`` at N/M = 1), D = DL = (F + 1) K and
    ||theta||^2 = ||theta_L||^2.  Not a reference function."""
    from .last_layer import _spectrum_last_layer
    N = full_set_size or X.shape[0]
    lam, DL, theta2 = _spectrum_last_layer(X, state, model_type)
    return _lml_from_spectrum(float(alpha), lam, DL, theta2, N / X.shape[0])[0]


def fit_alpha_last_layer(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2,
                         steps: int = 200):
    """:func:`fit_alpha` on the last-layer evidence: ``(alpha, history)``; the spectrum is computed once."""
    from .last_layer import _spectrum_last_layer
    N = full_set_size or X.shape[0]
    lam, DL, theta2 = _spectrum_last_layer(X, state, model_type)
    return _fit_from_spectrum(lam, DL, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def log_marginal_likelihood_last_layer_kron(alpha, X, state, model_type: str, full_set_size: Optional[int] = None) -> float:
    """:func:`log_marginal_likelihood_last_layer` under the Kronecker-factored curvature c A (x) Bf
    (``last_layer_kron.py``; no size cap): the spectrum is outer(lam_A, mu_B) / M from two small ``eigvalsh`` calls.
    Scalar alpha.  Not a reference function."""
    from .last_layer_kron import _spectrum_last_layer_kron
    N = full_set_size or X.shape[0]
    lam, DL, theta2 = _spectrum_last_layer_kron(X, state, model_type)
    return _lml_from_spectrum(float(alpha), lam, DL, theta2, N / X.shape[0])[0]


def fit_alpha_last_layer_kron(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2,
                              steps: int = 200):
    """:func:`fit_alpha` on the Kronecker-factored last-layer evidence: ``(alpha, history)``; the factors and their two
    eigendecompositions are computed once."""
    from .last_layer_kron import _spectrum_last_layer_kron
    N = full_set_size or X.shape[0]
    lam, DL, theta2 = _spectrum_last_layer_kron(X, state, model_type)
    return _fit_from_spectrum(lam, DL, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def log_marginal_likelihood_kfac(alpha, X, state, model_type: str, full_set_size: Optional[int] = None, *,
                                 curvature=None) -> float:
    """:func:`log_marginal_likelihood` under the Kronecker-factored curvature of every layer (``kfac.py``): the spectrum
    is the concatenation of outer(lam_l, mu_l) / (M T_l) over the layer blocks and the GGN diagonal of the parameters
    outside every block, D and ||theta||^2 those of the whole vector.  Scalar alpha.  ``curvature``: a spec of
    ``fisher.py`` for the output factors and that diagonal.  Not a reference function."""
    from .kfac import _spectrum_kfac
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_kfac(X, state, model_type, curvature)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])[0]


def fit_alpha_kfac(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2, steps: int = 200, *,
                   curvature=None):
    """:func:`fit_alpha` on the Kronecker-factored evidence: ``(alpha, history)``; the factors and their
    eigendecompositions are computed once (with the curvature spec ``curvature`` of ``fisher.py`` when one is given)."""
    from .kfac import _spectrum_kfac
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_kfac(X, state, model_type, curvature)
    return _fit_from_spectrum(lam, D, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def log_marginal_likelihood_ekfac(alpha, X, state, model_type: str, full_set_size: Optional[int] = None, *,
                                  moments: Optional[str] = None, curvature=None) -> float:
    """:func:`log_marginal_likelihood_kfac` under the eigenvalue-corrected curvature (``ekfac.py``): in the spectrum every
    block's outer(lam_l, mu_l) / (M T_l) is replaced by the second moments of the factor rows in the block's orthonormal
    Kronecker eigenbasis, which a scalar alpha does not move.  Scalar alpha.  ``moments`` / ``curvature``: the route of
    the second moments and the curvature spec of ``fisher.py`` (:func:`ekfac.posterior_lla_ekfac`).  Not a reference
    function."""
    from .ekfac import _spectrum_ekfac
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_ekfac(X, state, model_type, moments=moments, curvature=curvature)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])[0]


def fit_alpha_ekfac(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2, steps: int = 200, *,
                    moments: Optional[str] = None, curvature=None):
    """:func:`fit_alpha` on the eigenvalue-corrected evidence: ``(alpha, history)``; the factors, their
    eigendecompositions and the second moments (``moments`` / ``curvature`` as in
    :func:`log_marginal_likelihood_ekfac`) are computed once."""
    from .ekfac import _spectrum_ekfac
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_ekfac(X, state, model_type, moments=moments, curvature=curvature)
    return _fit_from_spectrum(lam, D, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def log_marginal_likelihood_lowrank(alpha, X, state, model_type: str, full_set_size: Optional[int] = None, rank: Optional[int] = None,
                                    example_chunk: Optional[int] = None, **solver) -> float:
    """:func:`log_marginal_likelihood` under the low-rank curvature (``lowrank.py``): the spectrum is the ``rank`` leading
    eigenvalues of the GGN of X from the matrix-free fit (``lowrank.DEFAULT_RANK`` when not given), every other direction
    flat; D and ||theta||^2 are those of the whole vector.  A scalar alpha does not move the eigenpairs, so one cached fit
    serves every alpha.  Scalar alpha.  Not a reference function."""
    from .lowrank import DEFAULT_RANK, _spectrum_lowrank
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_lowrank(X, state, model_type, rank or DEFAULT_RANK, example_chunk, **solver)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])[0]


def fit_alpha_lowrank(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2, steps: int = 200,
                      rank: Optional[int] = None, example_chunk: Optional[int] = None, **solver):
    """:func:`fit_alpha` on the low-rank evidence: ``(alpha, history)``; the eigenpairs are computed once."""
    from .lowrank import DEFAULT_RANK, _spectrum_lowrank
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_lowrank(X, state, model_type, rank or DEFAULT_RANK, example_chunk, **solver)
    return _fit_from_spectrum(lam, D, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def log_marginal_likelihood_subnetwork(alpha, X, state, model_type: str, indices, full_set_size: Optional[int] = None) -> float:
    """:func:`log_marginal_likelihood` of the subnetwork model (every parameter outside ``indices`` frozen): the spectrum
    is that of the dense subnetwork GGN (``subnetwork.compute_ggn_subnetwork`` at N/M = 1), D = |S| and
    ||theta||^2 = ||theta_S||^2.  No null-space projection is applied (an arbitrary index set has no known one), so on a
    classifier whose set holds the whole final layer the float32 softmax leak that
    ``last_layer._spectrum_last_layer`` removes stays in.  Scalar alpha.  Not a reference function."""
    from .subnetwork import _spectrum_subnetwork
    N = full_set_size or X.shape[0]
    lam, DS, theta2 = _spectrum_subnetwork(X, state, model_type, indices)
    return _lml_from_spectrum(float(alpha), lam, DS, theta2, N / X.shape[0])[0]


def fit_alpha_subnetwork(X, state, model_type, indices, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2,
                         steps: int = 200):
    """:func:`fit_alpha` on the subnetwork evidence: ``(alpha, history)``; the spectrum is computed once."""
    from .subnetwork import _spectrum_subnetwork
    N = full_set_size or X.shape[0]
    lam, DS, theta2 = _spectrum_subnetwork(X, state, model_type, indices)
    return _fit_from_spectrum(lam, DS, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


# ---- validation grid search (the reference's ``src/grid_search.py:9-88``) ------------------------------------------------
def refinement_points(grid, best: int):
    """the three refinement values of ``grid_search_alpha`` (``:49-64``): one quarter, one half and three quarters, in
    log10, of the bracket between the best point's two neighbours (at an end: the end point and its one neighbour)"""
    n = len(grid)
    if n < 2:
        raise ValueError("the refinement needs a coarse grid of at least two points")
    lo, hi = (0, 1) if best == 0 else ((n - 2, n - 1) if best == n - 1 else (best - 1, best + 1))
    ll, lr = math.log10(grid[lo]), math.log10(grid[hi])
    return [10.0 ** ((3.0 * ll + lr) / 4.0), 10.0 ** ((ll + lr) / 2.0), 10.0 ** ((ll + 3.0 * lr) / 4.0)]


def grid_search_alpha(state, Z0, val_loader, full_set_size, model_type, num_mc_samples=30, scalable=True, log10_min=-3,
                      log10_max=2, n_coarse=7, refine=True, rng_key=0, verbose=True, *, posterior: str = "inducing",
                      link: str = "probit", alpha_base=None, seed: int = 0, indices=None, rank=None, curvature=None,
                      route=None, return_history: bool = False):
    """``src/grid_search.py:9-88``: the prior precision with the smallest validation NLL on a coarse log grid
    ``logspace(log10_min, log10_max, n_coarse)`` (float64) followed, with ``refine``, by three points inside the bracket
    around the coarse best (:func:`refinement_points`); the first minimum over coarse-then-refined values wins.

    ``posterior="inducing"`` is the reference's search: every value goes through ``evaluate.eval_dataset`` (the MC
    predictive of the inducing-point posterior, ``num_mc_samples`` / ``scalable``) with ``rng=rng_key``, which the
    reference omits.  ``posterior="kfac"`` / ``"ekfac"``: two calls of ``evaluate.eval_dataset_closed_form_grid``, the
    coarse grid and the refinement, so one fit and two passes over ``val_loader`` serve the whole search; every other
    closed-form posterior of ``evaluate.eval_dataset_closed_form`` is evaluated value by value.  ``link`` / ``seed`` /
    ``indices`` / ``rank`` / ``curvature`` / ``route`` go to the closed-form evaluation.

    ``alpha_base=None``: the grid values are the precisions and a float comes back.  A :class:`prior.GroupedPrior`: the
    grid values multiply it as a whole and the scaled ``GroupedPrior`` comes back.  ``return_history=True``:
    ``(alpha, [(alpha, nll)])`` in evaluation order.  ``val_loader`` is walked once per evaluation, so it must be
    re-iterable: a list of (x, y) batches or a ``DataLoader``, not a generator."""
    from . import evaluate
    grid = [float(a) for a in torch.logspace(float(log10_min), float(log10_max), int(n_coarse), dtype=torch.float64).tolist()]
    base = 1.0 if alpha_base is None else alpha_base

    def evaluate_values(values):
        if posterior == "inducing":
            return [evaluate.eval_dataset(state, val_loader, Z0, alpha=evaluate.scaled_prior(base, a),
                                          full_set_size=full_set_size, model_type=model_type, num_mc_samples=num_mc_samples,
                                          rng=rng_key, scalable=scalable)[0] for a in values]
        res = evaluate.eval_dataset_closed_form_grid(state, val_loader, Z0, base, values, full_set_size, model_type, posterior,
                                                     link, seed=seed, indices=indices, rank=rank, curvature=curvature,
                                                     route=route)
        return [r[0] for r in res]

    def report(values, nlls):
        if verbose:
            for a, v in zip(values, nlls):
                print(f"alpha={a:9.3e}  NLL={v:.4f}")

    values = list(grid)
    nlls = [float(v) for v in evaluate_values(grid)]
    report(grid, nlls)
    if refine:
        best = min(range(len(grid)), key=lambda i: nlls[i])                   # the first minimum
        fine = refinement_points(grid, best)
        if verbose:
            print("\n-- refinement pass --")
        fine_nlls = [float(v) for v in evaluate_values(fine)]
        report(fine, fine_nlls)
        values += fine
        nlls += fine_nlls
    best = min(range(len(values)), key=lambda i: nlls[i])
    if verbose:
        print(f"\n>>> selected  alpha* = {values[best]:9.3e}  (val NLL = {nlls[best]:.4f})")
    alpha = values[best] if alpha_base is None else evaluate.scaled_prior(alpha_base, values[best])
    if return_history:
        return alpha, [(a if alpha_base is None else evaluate.scaled_prior(alpha_base, a), v) for a, v in zip(values, nlls)]
    return alpha


# ---- layer-wise precisions ------------------------------------------------------------------------------------------
def grouped_spectrum(X, state, model_type, prior: GroupedPrior):
    """``(grams (G, d, d) float64, sizes (G,), theta_sqnorms (G,) float64)`` of the factor built at N/M = 1 like
    :func:`_spectrum`: what the layer-wise evidence needs of the network, for the group table of ``prior`` (its values
    are not used)."""
    eng = get_engine(state, X, model_type)
    if prior.D != eng.D:
        raise ValueError(f"the prior covers {prior.D} parameters, the network has {eng.D}")
    c = math.exp(-0.5 * float(state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0
    grams = grouped_grams(materialize_factor(eng, c), prior)
    flat_p, _ = flatten_nn_params(state.params)
    return grams, prior.sizes, prior.group_sqnorms(flat_p).to(grams.device)


def lml_layerwise(log_alphas, grams: torch.Tensor, theta_sqnorms: torch.Tensor, rescale: float):
    """``(value, grad)``: value = -1/2 sum_g alpha_g ||theta_g||^2 - 1/2 logdet(I_d + rescale sum_g G_g / alpha_g) (the
    convention of :func:`_lml_from_spectrum`, in which the D_g log alpha_g terms cancel) and its gradient (G,) float64
    in log alpha_g:  -1/2 alpha_g ||theta_g||^2 + 1/2 (rescale / alpha_g) tr((I + rescale Gt)^-1 G_g).
    Float64 torch on the device of ``grams`` (CPU included); one Cholesky factorisation of the d x d matrix."""
    grams = grams.double()
    la = torch.as_tensor(log_alphas, dtype=torch.float64, device=grams.device).reshape(-1)
    t2 = torch.as_tensor(theta_sqnorms, dtype=torch.float64, device=grams.device).reshape(-1)
    alphas = torch.exp(la)
    d = grams.shape[-1]
    Mx = torch.eye(d, dtype=torch.float64, device=grams.device) + rescale * (grams / alphas[:, None, None]).sum(0)
    L = torch.linalg.cholesky(0.5 * (Mx + Mx.T))
    logdet = 2.0 * torch.log(torch.diagonal(L)).sum()
    value = -0.5 * (alphas * t2).sum() - 0.5 * logdet
    Minv = torch.cholesky_inverse(L)
    traces = (Minv[None] * grams).sum((1, 2))                              # tr(M^-1 G_g): both symmetric
    grad = -0.5 * alphas * t2 + 0.5 * (rescale / alphas) * traces
    return float(value), grad


def log_marginal_likelihood_layerwise(prior: GroupedPrior, X, state, model_type: str, full_set_size: Optional[int] = None) -> float:
    """log p(D | alpha_1 .. alpha_G) up to precision-independent constants, at the precisions of ``prior``"""
    N = full_set_size or X.shape[0]
    grams, _, t2 = grouped_spectrum(X, state, model_type, prior)
    return lml_layerwise(torch.log(prior.values), grams, t2, N / X.shape[0])[0]


def _adam_update(opt: Adam, grad: torch.Tensor, opt_state):
    """:meth:`Adam.update` applied per component of a float64 vector (the scalar class is left alone)"""
    c = opt_state["count"] + 1
    mu = opt.b1 * opt_state["mu"] + (1 - opt.b1) * grad
    nu = opt.b2 * opt_state["nu"] + (1 - opt.b2) * grad * grad
    mu_hat, nu_hat = mu / (1 - opt.b1 ** c), nu / (1 - opt.b2 ** c)
    return -opt.lr * mu_hat / (torch.sqrt(nu_hat) + opt.eps), dict(count=c, mu=mu, nu=nu)


def fit_log_alphas(grams, theta_sqnorms, rescale: float, log_alphas0, alpha_lr: float = 5e-2, steps: int = 200):
    """The hyper-steps of :func:`fit_alpha` on all log alpha_g at once, from the Grams: ``(log_alphas, history)`` with
    history = [(alphas (G,) float64 on the CPU, value)] before each step.  With G = 1 it walks :func:`fit_alpha`'s
    trajectory."""
    la = torch.as_tensor(log_alphas0, dtype=torch.float64, device=grams.device).reshape(-1).clone()
    opt = Adam(alpha_lr)
    st = dict(count=0, mu=torch.zeros_like(la), nu=torch.zeros_like(la))
    history = []
    for _ in range(steps):
        v, g = lml_layerwise(la, grams, theta_sqnorms, rescale)
        history.append((torch.exp(la).cpu(), v))
        upd, st = _adam_update(opt, -g, st)
        la = la + upd
    return la, history


def fit_alpha_layerwise(X, state, model_type, full_set_size=None, groups="layer", alpha0: float = 1.0,
                        alpha_lr: float = 5e-2, steps: int = 200):
    """:func:`fit_alpha` with one precision per group (``groups`` as in :class:`prior.GroupedPrior`) for a fixed theta:
    ``(GroupedPrior, history)``.  The per-group Grams are built once; every step is d x d algebra."""
    N = full_set_size or X.shape[0]
    prior = GroupedPrior(state.params, alpha0, groups)
    grams, _, t2 = grouped_spectrum(X, state, model_type, prior)
    la, history = fit_log_alphas(grams, t2, N / X.shape[0], torch.log(prior.values), alpha_lr, steps)
    return prior.with_values(torch.exp(la).cpu()), history


# ---- the diagonal posterior, and layer-wise precisions for the structured posteriors (``evidence.py``) -----------------
def _spectrum_diag(X, state, model_type, curvature=None):
    """the GGN diagonal built at N/M = 1 (float64, clamped at 0), D, ||theta||^2: the spectrum of the diagonal posterior"""
    from .ggn import compute_ggn_diag
    diag = compute_ggn_diag(state, X, model_type, curvature=curvature).double().clamp_min(0.0)
    flat_p, _ = flatten_nn_params(state.params)
    return diag, flat_p.numel(), float((flat_p.detach().double() ** 2).sum())


def log_marginal_likelihood_diag(alpha, X, state, model_type: str, full_set_size: Optional[int] = None, *,
                                 curvature=None) -> float:
    """:func:`log_marginal_likelihood` under the diagonal posterior (``lla.posterior_lla_diag``): the spectrum is the exact
    GGN diagonal.  ``alpha``: a scalar or a :class:`prior.GroupedPrior` with any grouping; ``curvature``: a spec of
    ``fisher.py`` for the diagonal.  Not a reference function."""
    N = full_set_size or X.shape[0]
    if isinstance(alpha, GroupedPrior):
        from . import evidence
        plan = evidence.plan_diag(state, X, model_type, alpha, curvature=curvature)
        return evidence.lml_structured(torch.log(alpha.values), plan, N / X.shape[0])[0]
    lam, D, theta2 = _spectrum_diag(X, state, model_type, curvature)
    return _lml_from_spectrum(float(alpha), lam, D, theta2, N / X.shape[0])[0]


def fit_alpha_diag(X, state, model_type, full_set_size=None, alpha0: float = 1.0, alpha_lr: float = 5e-2, steps: int = 200, *,
                   curvature=None):
    """:func:`fit_alpha` on the evidence of the diagonal posterior: ``(alpha, history)``; the diagonal is built once."""
    N = full_set_size or X.shape[0]
    lam, D, theta2 = _spectrum_diag(X, state, model_type, curvature)
    return _fit_from_spectrum(lam, D, theta2, N / X.shape[0], alpha0, alpha_lr, steps)


def _fit_structured(plan, prior: GroupedPrior, rescale: float, alpha_lr: float, steps: int):
    from . import evidence
    la, history = evidence.fit_log_alphas_structured(plan, rescale, torch.log(prior.values), alpha_lr, steps)
    return prior.with_values(torch.exp(la).cpu()), history


def fit_alpha_diag_layerwise(X, state, model_type, full_set_size=None, groups="layer", alpha0: float = 1.0,
                             alpha_lr: float = 5e-2, steps: int = 200, *, curvature=None):
    """:func:`fit_alpha_diag` with one precision per group (``groups`` as in :class:`prior.GroupedPrior`, any grouping)
    for a fixed theta: ``(GroupedPrior, history)``, the history that of :func:`fit_log_alphas`.  The diagonal is built
    once; every step is one evaluation of ``lip_evidence_terms``.  The prior goes into ``lla.posterior_lla_diag``."""
    from . import evidence
    N = full_set_size or X.shape[0]
    prior = GroupedPrior(state.params, alpha0, groups)
    plan = evidence.plan_diag(state, X, model_type, prior, curvature=curvature)
    return _fit_structured(plan, prior, N / X.shape[0], alpha_lr, steps)


def log_marginal_likelihood_kfac_layerwise(prior: GroupedPrior, X, state, model_type: str, full_set_size: Optional[int] = None,
                                           *, curvature=None) -> float:
    """:func:`log_marginal_likelihood_kfac` at the precisions of ``prior``, which must be constant over every layer block
    (``groups="layer"``): then the Kronecker eigenbasis of a block does not move with the precisions and the evidence is
    two grouped sums over c_l lam_i mu_j and the remainder's GGN diagonal (``evidence.py``)."""
    from . import evidence
    N = full_set_size or X.shape[0]
    plan = evidence.plan_kfac(state, X, model_type, prior, curvature=curvature)
    return evidence.lml_structured(torch.log(prior.values), plan, N / X.shape[0])[0]


def fit_alpha_kfac_layerwise(X, state, model_type, full_set_size=None, groups="layer", alpha0: float = 1.0,
                             alpha_lr: float = 5e-2, steps: int = 200, *, curvature=None):
    """:func:`fit_alpha_kfac` with one precision per group: ``(GroupedPrior, history)``.  The factors and their
    eigenvalues are computed once; a grouping that cuts a layer block (``"tensor"`` on a layer with a bias) is refused
    before anything is bound.  The prior goes into ``kfac.posterior_lla_kfac`` and its predictives."""
    from . import evidence
    N = full_set_size or X.shape[0]
    prior = GroupedPrior(state.params, alpha0, groups)
    plan = evidence.plan_kfac(state, X, model_type, prior, curvature=curvature)
    return _fit_structured(plan, prior, N / X.shape[0], alpha_lr, steps)


def log_marginal_likelihood_ekfac_layerwise(prior: GroupedPrior, X, state, model_type: str, full_set_size: Optional[int] = None,
                                            *, moments: Optional[str] = None, curvature=None) -> float:
    """:func:`log_marginal_likelihood_ekfac` at the precisions of ``prior`` (constant over every layer block, as
    :func:`log_marginal_likelihood_kfac_layerwise` asks): the grouped sums run over the eigenbasis second moments."""
    from . import evidence
    N = full_set_size or X.shape[0]
    plan = evidence.plan_ekfac(state, X, model_type, prior, moments=moments, curvature=curvature)
    return evidence.lml_structured(torch.log(prior.values), plan, N / X.shape[0])[0]


def fit_alpha_ekfac_layerwise(X, state, model_type, full_set_size=None, groups="layer", alpha0: float = 1.0,
                              alpha_lr: float = 5e-2, steps: int = 200, *, moments: Optional[str] = None, curvature=None):
    """:func:`fit_alpha_ekfac` with one precision per group: ``(GroupedPrior, history)``; the factors, their
    eigendecompositions and the second moments are computed once.  The prior goes into ``ekfac.posterior_lla_ekfac`` and
    its predictives."""
    from . import evidence
    N = full_set_size or X.shape[0]
    prior = GroupedPrior(state.params, alpha0, groups)
    plan = evidence.plan_ekfac(state, X, model_type, prior, moments=moments, curvature=curvature)
    return _fit_structured(plan, prior, N / X.shape[0], alpha_lr, steps)
