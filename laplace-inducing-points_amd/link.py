"""Links from a Gaussian over the logits to class probabilities, for every closed-form predictive.  Not a reference function.

Each ``predict_lla_*`` ends in ``(f_mean, f_var)`` (``cov="diag"``) or a ``MultivariateNormalFullCovariance`` of (B, K, K)
covariances (``cov="full"``).  :func:`link_predictive` turns either into (B, K) probabilities by one of four links:

* ``"probit"`` — ``lla.probit_predictive``, softmax(m / sqrt(1 + pi / 8 v)); a full covariance contributes its diagonal.
* ``"mc"`` — the softmax integrated over the Gaussian by ``num_samples`` draws on the device (``lip_link_mc``: one fused
  draw -> softmax -> accumulate kernel, no (S, B, K) tensor).  The only link that uses the off-diagonal covariances: a
  full covariance goes through ``lip_link_chol`` (K <= 64).  The draw of (sample, ``example_offset`` + row) is a pure
  function of ``seed`` and those two indices, so results repeat bit for bit and do not depend on how a test set is cut
  into batches.  With ``return_uncertainty`` also the split of the predictive entropy into its expected (aleatoric)
  part and the mutual information (epistemic part), from the same draws.
* ``"bridge"`` — the Laplace bridge to a Dirichlet, a_k = (1 / v_k)(1 - 2 / K + exp(m_k) sum_l exp(-m_l) / K^2), probs =
  a / sum a.  ``"bridge_norm"``: the same after vbar = mean_k(v) / sqrt(K / 2), m <- m / sqrt(vbar), v <- v / vbar.
"""
from __future__ import annotations

import math

import torch

from .distributions import MultivariateNormalFullCovariance

LINKS = ("probit", "mc", "bridge", "bridge_norm")
MC_MAX_CLASSES = 8192             # lip_link_mc with variances
MC_FACTOR_MAX_CLASSES = 64        # lip_link_mc with a factor, lip_link_chol


def _mean_and_cov(f_mean, f_cov):
    """-> (mean (B, K), variances (B, K) or None, covariances (B, K, K) or None)"""
    if isinstance(f_mean, MultivariateNormalFullCovariance):
        if f_cov is not None:
            raise ValueError("give a distribution alone, or a mean and its variances or covariances")
        f_mean, f_cov = f_mean.mean(), f_mean.covariance()
    elif isinstance(f_cov, MultivariateNormalFullCovariance):
        f_cov = f_cov.covariance()
    if not (torch.is_tensor(f_mean) and torch.is_tensor(f_cov)):
        raise ValueError("link_predictive takes (f_mean, f_var) tensors or a MultivariateNormalFullCovariance")
    if f_cov.dim() == 3 and f_cov.shape[-1] == f_cov.shape[-2] and f_mean.numel() == f_cov.shape[0] * f_cov.shape[-1]:
        return f_mean.reshape(f_cov.shape[0], f_cov.shape[-1]), None, f_cov      # loc of one test point comes squeezed
    if f_mean.dim() != 2:
        raise ValueError(f"links are for classifiers: a (B, K) mean of logits, not {tuple(f_mean.shape)} (a regressor's "
                         "predictive is lla.probit_predictive(f_mean, f_var, logvar))")
    if tuple(f_cov.shape) != tuple(f_mean.shape):
        raise ValueError(f"mean {tuple(f_mean.shape)} with variances or covariances {tuple(f_cov.shape)}")
    return f_mean, f_cov, None


def bridge_predictive(f_mean: torch.Tensor, f_var: torch.Tensor, normalise: bool = False, return_alpha: bool = False):
    """The Laplace bridge in float64: Dirichlet parameters a (B, K) of the Gaussian N(f_mean, diag(f_var)) over the logits
    and the Dirichlet mean a / sum a.  ``normalise``: the variance-normalised form (``link="bridge_norm"``)."""
    m, v = f_mean.double(), f_var.double()
    if not bool((v > 0).all()):
        raise ValueError("the Laplace bridge divides by the variances: every f_var must be positive")
    K = m.shape[-1]
    if normalise:
        vbar = v.mean(-1, keepdim=True) / math.sqrt(K / 2.0)
        m, v = m / torch.sqrt(vbar), v / vbar
    a = (1.0 - 2.0 / K + torch.exp(m + torch.logsumexp(-m, dim=-1, keepdim=True)) / K ** 2) / v
    probs = a / a.sum(-1, keepdim=True)
    return (probs, a) if return_alpha else probs


def _check_flags(flags: torch.Tensor, what: str) -> None:
    dead = torch.nonzero(flags)
    if dead.numel():
        raise ValueError(f"{what}: row {int(dead[0])} is dead (the first of {dead.numel()})")


def cholesky_semidefinite(cov: torch.Tensor) -> torch.Tensor:
    """Lower factors L (B, K, K) float32 with L L^T = cov for (B, K, K) float64 device covariances that may be
    rank-deficient (``lip_link_chol``: a column whose pivot is at most 2^-20 max_i C_ii is zero).  K <= 64."""
    from . import _native as nv
    B, K = cov.shape[0], cov.shape[-1]
    if K > MC_FACTOR_MAX_CLASSES:
        raise ValueError(f"a full covariance is factored for at most {MC_FACTOR_MAX_CLASSES} classes, not {K}: take the "
                         "marginal variances (cov=\"diag\")")
    cov = cov.to(torch.float64).contiguous()
    L = torch.empty(B, K, K, device=cov.device, dtype=torch.float32)
    flags = torch.empty(B, device=cov.device, dtype=torch.int32)
    nv.check(nv.load().lip_link_chol(nv.ptr(cov), B, K, nv.ptr(L), nv.ptr(flags), nv.stream_ptr()), "lip_link_chol")
    _check_flags(flags, "a covariance with a non-finite entry or a negative diagonal")
    return L


def mc_predictive(f_mean: torch.Tensor, f_var=None, factor=None, num_samples: int = 1000, seed: int = 0,
                  example_offset: int = 0):
    """``lip_link_mc`` on device tensors: (probs (B, K), mean_entropy (B,)) float64 from the mean (B, K) and exactly one of
    the variances (B, K) and a lower factor (B, K, K) float32."""
    from . import _native as nv
    B, K = f_mean.shape
    cap = MC_MAX_CLASSES if factor is None else MC_FACTOR_MAX_CLASSES
    if K > cap:
        raise ValueError(f"the Monte-Carlo link takes at most {cap} classes in this form, not {K}")
    m = f_mean.to(torch.float64).contiguous()
    v = None if f_var is None else f_var.to(device=m.device, dtype=torch.float64).contiguous()
    Lf = None if factor is None else factor.to(device=m.device, dtype=torch.float32).contiguous()
    probs = torch.empty(B, K, device=m.device, dtype=torch.float64)
    ent = torch.empty(B, device=m.device, dtype=torch.float64)
    flags = torch.empty(B, device=m.device, dtype=torch.int32)
    nv.check(nv.load().lip_link_mc(nv.ptr(m), nv.ptr(v), nv.ptr(Lf), B, K, int(num_samples), int(seed) & (2 ** 64 - 1),
                                   int(example_offset), nv.ptr(probs), nv.ptr(ent), nv.ptr(flags), nv.stream_ptr()),
             "lip_link_mc")
    _check_flags(flags, "a mean that is not finite, or a variance or factor that is negative or not finite")
    return probs, ent


def link_predictive(f_mean, f_cov=None, link: str = "probit", num_samples: int = 1000, seed: int = 0,
                    example_offset: int = 0, return_uncertainty: bool = False):
    """Class probabilities (B, K) of the Gaussian over the logits that a ``predict_lla_*`` returned: ``(f_mean, f_var)``
    or a ``MultivariateNormalFullCovariance``; ``link`` is one of :data:`LINKS` (module docstring).  ``num_samples``,
    ``seed`` and ``example_offset`` (the number of test points before this batch) are read by ``link="mc"`` alone, and so
    is ``return_uncertainty``: then -> (probs, {"total": H(probs), "aleatoric": mean_s H(p^s), "epistemic": their
    difference, the mutual information}), (B,) float64 each, in nats."""
    if link not in LINKS:
        raise ValueError(f"link must be one of {LINKS}, got {link!r}")
    if return_uncertainty and link != "mc":
        raise ValueError("the uncertainty split needs the draws: return_uncertainty is for link='mc'")
    mean, var, cov = _mean_and_cov(f_mean, f_cov)
    if link == "mc":
        if cov is not None:
            probs, ent = mc_predictive(mean, factor=cholesky_semidefinite(cov), num_samples=num_samples, seed=seed,
                                       example_offset=example_offset)
        else:
            probs, ent = mc_predictive(mean, f_var=var, num_samples=num_samples, seed=seed, example_offset=example_offset)
        if not return_uncertainty:
            return probs
        total = -torch.xlogy(probs, probs).sum(-1)
        return probs, {"total": total, "aleatoric": ent, "epistemic": total - ent}
    if var is None:
        var = torch.diagonal(cov, dim1=-2, dim2=-1)
    if link == "probit":
        from .lla import probit_predictive
        return probit_predictive(mean, var)
    return bridge_predictive(mean, var, normalise=link == "bridge_norm")
