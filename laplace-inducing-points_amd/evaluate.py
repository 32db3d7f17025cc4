"""Predictive evaluation harness — the reference's ``scale_experiments/evaluate.py:40-231`` ("next" row N3):
MC predictive NLL / accuracy (``batch_nll`` ``:98-154``), Brier (``:40-43``), ECE (``:45-63``), OOD-AUROC
(``:65-93``), ``eval_dataset`` (``:157-184``), ``eval_dataset_extended`` (``:187-231``).
Logit samples come from ``predict_lla_scalable`` (HIP engine); the metrics are plain reductions on the device.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch

from .lla import predict_lla_dense, predict_lla_scalable


def brier_score(probs: torch.Tensor, labels: torch.Tensor) -> float:
    """``:40-43`` multi-class Brier score."""
    one_hot = torch.nn.functional.one_hot(labels.long(), probs.shape[-1]).to(probs.dtype)
    return float(((probs - one_hot) ** 2).sum(1).mean())


def ece(probs: torch.Tensor, labels: torch.Tensor, n_bins: int = 15) -> float:
    """``:45-63`` expected calibration error, histogram binning on [lo, hi)."""
    conf, pred = probs.max(1)
    acc = (pred == labels.long()).to(probs.dtype)
    edges = torch.linspace(0.0, 1.0, n_bins + 1, device=probs.device, dtype=probs.dtype)
    val = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        mask = (conf >= lo) & (conf < hi)
        if not bool(mask.any()):
            continue
        val += float((conf[mask].mean() - acc[mask].mean()).abs() * mask.to(probs.dtype).mean())
    return val


def ood_scores(probs: torch.Tensor) -> torch.Tensor:
    """``:65-67``: higher = more in-distribution-like."""
    return -probs.max(1).values


def roc_auc(labels: torch.Tensor, scores: torch.Tensor) -> float:
    """Area under the ROC curve by the rank statistic (ties get average ranks), = sklearn.roc_auc_score."""
    scores = scores.double().cpu()
    labels = labels.double().cpu()
    order = torch.argsort(scores)
    s = scores[order]
    ranks = torch.empty_like(s)
    i, n = 0, s.numel()
    r = torch.arange(1, n + 1, dtype=torch.float64)
    # average ranks over ties
    uniq, inv, cnt = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    ends = torch.cumsum(cnt, 0).double()
    starts = ends - cnt.double() + 1
    ranks = ((starts + ends) / 2)[inv]
    full = torch.empty(n, dtype=torch.float64)
    full[order] = ranks
    pos = labels > 0.5
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    return float((full[pos].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


def batch_nll(state, x, y, Z, *, alpha, full_set_size, model_type, num_mc_samples, rng, scalable=True,
              return_mean=False):
    """``:98-154``: (NLL of the MC-averaged predictive, accuracy[, mean probabilities])."""
    if scalable == "marginals":
        # closed-form per-point predictive (lla.predict_lla_marginals): the metrics below only use per-point marginals,
        # so the S draws can be taken in the K-dimensional output space instead of through S tangent sweeps
        from .lla import predict_lla_marginals
        dist = predict_lla_marginals(state, x, Z, model_type=model_type, alpha=alpha, full_set_size=full_set_size)
        logit_samples = dist.sample(sample_shape=(num_mc_samples,), seed=rng).float()
    elif scalable:
        logit_samples = predict_lla_scalable(state, x, Z, model_type=model_type, alpha=alpha,
                                             full_set_size=full_set_size, num_samples=num_mc_samples, key=rng)
    else:
        dist = predict_lla_dense(state, x, Z, model_type=model_type, alpha=alpha, full_set_size=full_set_size)
        logit_samples = dist.sample(sample_shape=(num_mc_samples,), seed=rng).float()
    S = logit_samples.shape[0]
    log_probs = torch.log_softmax(logit_samples, dim=-1)                               # (S, B, C)
    y_int = y.reshape(-1).long().to(log_probs.device)
    log_p_true = torch.gather(log_probs, -1, y_int[None, :, None].expand(S, -1, 1)).squeeze(-1)   # (S, B)
    log_avg_prob = torch.logsumexp(log_p_true, dim=0) - math.log(S)
    nll = -log_avg_prob.mean()
    mean = torch.softmax(logit_samples, dim=-1).mean(0)                                # (B, C)
    acc = (mean.argmax(-1) == y_int).float().mean()
    if return_mean:
        return nll, acc, mean
    return nll, acc


def eval_dataset(state, dataloader: Iterable, Z, alpha, full_set_size, model_type, num_mc_samples, rng, scalable=True):
    """``:157-184``"""
    tot_nll = tot_correct = 0.0
    tot_N = 0
    for x_b, y_b in dataloader:
        rng = int(rng) + 1
        nll, acc = batch_nll(state, x_b, y_b, Z, alpha=alpha, full_set_size=full_set_size, model_type=model_type,
                             num_mc_samples=num_mc_samples, rng=rng, scalable=scalable)
        bs = x_b.shape[0]
        tot_nll += float(nll) * bs
        tot_correct += float(acc) * bs
        tot_N += bs
    return tot_nll / tot_N, tot_correct / tot_N


def eval_dataset_extended(state, dataloader: Iterable, Z, alpha, full_set_size, model_type, num_mc_samples, rng,
                          scalable=True):
    """``:187-231``: (NLL, accuracy, Brier, ECE, probs, labels)"""
    tot_nll = tot_correct = 0.0
    tot_N = 0
    all_probs, all_labels = [], []
    for x_b, y_b in dataloader:
        rng = int(rng) + 1
        nll, acc, mean = batch_nll(state, x_b, y_b, Z, alpha=alpha, full_set_size=full_set_size, model_type=model_type,
                                   num_mc_samples=num_mc_samples, rng=rng, scalable=scalable, return_mean=True)
        bs = x_b.shape[0]
        tot_nll += float(nll) * bs
        tot_correct += float(acc) * bs
        tot_N += bs
        all_probs.append(mean)
        all_labels.append(y_b.reshape(-1).to(mean.device))
    probs, labels = torch.cat(all_probs), torch.cat(all_labels)
    return tot_nll / tot_N, tot_correct / tot_N, brier_score(probs, labels), ece(probs, labels), probs, labels


def auroc_ood(state, id_probs: torch.Tensor, ood_loader: Iterable, Z, alpha, full_set_size, model_type,
              num_mc_samples, rng, scalable=True) -> float:
    """``:69-93``: AUROC of max-probability scores, in-distribution (label 0) vs OOD (label 1)."""
    ood = []
    for xb, yb in ood_loader:
        rng = int(rng) + 1
        dummy = torch.zeros(xb.shape[0], dtype=torch.long)
        _, _, mean = batch_nll(state, xb, dummy, Z, alpha=alpha, full_set_size=full_set_size, model_type=model_type,
                               num_mc_samples=num_mc_samples, rng=rng, scalable=scalable, return_mean=True)
        ood.append(mean)
    ood_probs = torch.cat(ood)
    scores = torch.cat([ood_scores(id_probs), ood_scores(ood_probs)])
    labels = torch.cat([torch.zeros(len(id_probs)), torch.ones(len(ood_probs))])
    return roc_auc(labels, scores)


def eval_dataset_probit(state, dataloader: Iterable, Z, alpha, full_set_size, model_type="classifier",
                        posterior: str = "diag", indices=None, rank=None, *, curvature=None, route=None):
    """:func:`eval_dataset_extended` without draws: the class probabilities are the probit predictive
    (``lla.probit_predictive``) of the closed-form output variances — ``posterior="diag"``: the diagonal Laplace
    posterior (``lla.predict_lla_diag``), ``"inducing"``: the inducing-point posterior (``lla.predict_lla_variances``),
    ``"last_layer"``: the dense last-layer posterior (``lla.predict_lla_last_layer``, fitted once for all batches),
    ``"last_layer_kron"``: its Kronecker-factored twin without the size cap (``lla.predict_lla_last_layer_kron``),
    ``"subnetwork"``: the dense posterior over the flat-parameter indices ``indices`` (``lla.predict_lla_subnetwork``,
    fitted once for all batches; ``indices`` is read by this value alone), ``"kfac"``: the Kronecker-factored posterior
    over all layers (``lla.predict_lla_kfac``, fitted once for all batches), ``"ekfac"``: its eigenvalue-corrected twin
    (``lla.predict_lla_ekfac``, fitted once for all batches), ``"lowrank"``: the low-rank posterior from the ``rank``
    leading eigenpairs of the GGN of Z (``lla.predict_lla_lowrank``, fitted once for all batches; ``rank`` is read by this
    value alone, ``None``: ``lowrank.DEFAULT_RANK``).  ``curvature``: a spec of ``fisher.py`` for the fit of
    ``posterior="diag"``, ``"kfac"`` and ``"ekfac"`` (whose second moments then come from the backward sweep,
    ``moments="sweep"``); the other posteriors refuse one.  ``route``: ``"rows"`` or ``"sweep"`` for the predictive of
    ``posterior="kfac"`` and ``"ekfac"`` (``kfac.predict_lla_kfac``; ``"sweep"`` forms no Jacobian row, so it runs at any
    D and K); the other posteriors refuse one.
    -> (NLL, accuracy, Brier, ECE, probs, labels)"""
    from .lla import (predict_lla_diag, predict_lla_ekfac, predict_lla_kfac, predict_lla_last_layer, predict_lla_last_layer_kron,
                      predict_lla_lowrank, predict_lla_subnetwork, predict_lla_variances, probit_predictive)
    rank_kw = {} if rank is None else {"rank": rank}
    curv_kw = {}
    if curvature is not None:
        if posterior not in ("diag", "kfac", "ekfac"):
            raise ValueError(f"curvature is taken by posterior='diag', 'kfac' and 'ekfac' only, not {posterior!r}")
        curv_kw = {"curvature": curvature}
    if route is not None:
        if posterior not in ("kfac", "ekfac"):
            raise ValueError(f"route is taken by posterior='kfac' and 'ekfac' only, not {posterior!r}")
        curv_kw = dict(curv_kw, route=route)
    if posterior == "subnetwork" and indices is None:
        raise ValueError("posterior='subnetwork' needs indices")
    predict = {"diag": predict_lla_diag, "inducing": predict_lla_variances,
               "last_layer": lambda *a, **kw: predict_lla_last_layer(*a, cov="diag", **kw),
               "last_layer_kron": lambda *a, **kw: predict_lla_last_layer_kron(*a, cov="diag", **kw),
               "kfac": lambda *a, **kw: predict_lla_kfac(*a, cov="diag", **kw),
               "ekfac": lambda *a, **kw: predict_lla_ekfac(*a, cov="diag", **kw),
               "lowrank": lambda *a, **kw: predict_lla_lowrank(*a, cov="diag", **rank_kw, **kw),
               "subnetwork": lambda *a, **kw: predict_lla_subnetwork(*a, indices, cov="diag", **kw)}[posterior]
    all_probs, all_labels = [], []
    for x_b, y_b in dataloader:
        probs = probit_predictive(*predict(state, x_b, Z, model_type, alpha, full_set_size=full_set_size, **curv_kw))
        all_probs.append(probs)
        all_labels.append(y_b.reshape(-1).long().to(probs.device))
    probs, labels = torch.cat(all_probs), torch.cat(all_labels)
    nll = -torch.log(torch.gather(probs, -1, labels[:, None]).squeeze(-1)).mean()
    acc = (probs.argmax(-1) == labels).to(probs.dtype).mean()
    return float(nll), float(acc), brier_score(probs, labels), ece(probs, labels), probs, labels


def _closed_form_predict(posterior: str, cov: str, indices=None, rank=None, curvature=None, route=None):
    """the predictive of :func:`eval_dataset_probit`'s ``posterior`` with its ``curvature`` / ``route`` / ``indices`` /
    ``rank`` forwarding, returning marginal variances (``cov="diag"``) or full covariances (``cov="full"``)"""
    from .lla import (predict_lla_diag, predict_lla_ekfac, predict_lla_kfac, predict_lla_last_layer, predict_lla_last_layer_kron,
                      predict_lla_lowrank, predict_lla_marginals, predict_lla_subnetwork, predict_lla_variances)
    if cov not in ("diag", "full"):
        raise ValueError("cov must be 'diag' or 'full'")
    rank_kw = {} if rank is None else {"rank": rank}
    curv_kw = {}
    if curvature is not None:
        if posterior not in ("diag", "kfac", "ekfac"):
            raise ValueError(f"curvature is taken by posterior='diag', 'kfac' and 'ekfac' only, not {posterior!r}")
        curv_kw = {"curvature": curvature}
    if route is not None:
        if posterior not in ("kfac", "ekfac"):
            raise ValueError(f"route is taken by posterior='kfac' and 'ekfac' only, not {posterior!r}")
        curv_kw = dict(curv_kw, route=route)
    if posterior == "subnetwork" and indices is None:
        raise ValueError("posterior='subnetwork' needs indices")
    table = {"diag": lambda *a, **kw: predict_lla_diag(*a, cov=cov, **kw),
             "inducing": predict_lla_variances if cov == "diag" else predict_lla_marginals,
             "last_layer": lambda *a, **kw: predict_lla_last_layer(*a, cov=cov, **kw),
             "last_layer_kron": lambda *a, **kw: predict_lla_last_layer_kron(*a, cov=cov, **kw),
             "kfac": lambda *a, **kw: predict_lla_kfac(*a, cov=cov, **kw),
             "ekfac": lambda *a, **kw: predict_lla_ekfac(*a, cov=cov, **kw),
             "lowrank": lambda *a, **kw: predict_lla_lowrank(*a, cov=cov, **rank_kw, **kw),
             "subnetwork": lambda *a, **kw: predict_lla_subnetwork(*a, indices, cov=cov, **kw)}
    if posterior not in table:
        raise ValueError(f"posterior must be one of {sorted(table)}, got {posterior!r}")
    predict = table[posterior]
    return lambda state, x, Z, model_type, alpha, full_set_size: predict(state, x, Z, model_type, alpha,
                                                                         full_set_size=full_set_size, **curv_kw)


def _closed_form_batches(state, dataloader, Z, alpha, full_set_size, model_type, predict, link, num_samples, seed, offset,
                         uncertainty=False):
    """per batch (link_predictive's result, labels); batch b is drawn with ``example_offset`` = ``offset`` + the number of
    points before it, so the draws of a point do not depend on the loader's batch size"""
    from .link import link_predictive
    for x_b, y_b in dataloader:
        out = predict(state, x_b, Z, model_type, alpha, full_set_size)
        out = out if isinstance(out, tuple) else (out,)
        yield link_predictive(*out, link=link, num_samples=num_samples, seed=seed, example_offset=offset,
                              return_uncertainty=uncertainty), y_b
        offset += int(x_b.shape[0])


def eval_dataset_closed_form(state, dataloader: Iterable, Z, alpha, full_set_size, model_type="classifier",
                             posterior: str = "diag", link: str = "probit", cov: str = "diag", num_samples: int = 1000,
                             seed: int = 0, indices=None, rank=None, *, curvature=None, route=None):
    """:func:`eval_dataset_probit` with the link a parameter (``link.link_predictive``): ``"probit"`` (then the tensors
    equal :func:`eval_dataset_probit`'s), ``"mc"`` (``num_samples`` draws per point from ``seed``, on the device),
    ``"bridge"`` or ``"bridge_norm"``.  ``cov="full"`` asks the posterior's predictive for (B, K, K) covariances, which
    only ``link="mc"`` uses beyond their diagonal (K <= 64; ``posterior="inducing"`` then takes
    ``lla.predict_lla_marginals``).  Same posteriors and ``curvature`` / ``route`` / ``indices`` / ``rank`` forwarding as
    :func:`eval_dataset_probit`.  The draws of a test point depend on ``seed`` and its position in the data set alone:
    the result does not depend on the loader's batch size.  -> (NLL, accuracy, Brier, ECE, probs, labels)"""
    predict = _closed_form_predict(posterior, cov, indices, rank, curvature, route)
    all_probs, all_labels = [], []
    for probs, y_b in _closed_form_batches(state, dataloader, Z, alpha, full_set_size, model_type, predict, link,
                                           num_samples, seed, 0):
        all_probs.append(probs)
        all_labels.append(y_b.reshape(-1).long().to(probs.device))
    probs, labels = torch.cat(all_probs), torch.cat(all_labels)
    nll = -torch.log(torch.gather(probs, -1, labels[:, None]).squeeze(-1)).mean()
    acc = (probs.argmax(-1) == labels).to(probs.dtype).mean()
    return float(nll), float(acc), brier_score(probs, labels), ece(probs, labels), probs, labels


def scaled_prior(alpha, s: float):
    """the prior s ``alpha``: a float for a scalar, a :class:`prior.GroupedPrior` with every value multiplied otherwise"""
    from .prior import is_grouped
    return alpha.with_values(alpha.values * float(s)) if is_grouped(alpha) else float(alpha) * float(s)


def _classifier_metrics(probs, labels):
    nll = -torch.log(torch.gather(probs, -1, labels[:, None]).squeeze(-1)).mean()
    acc = (probs.argmax(-1) == labels).to(probs.dtype).mean()
    return float(nll), float(acc), brier_score(probs, labels), ece(probs, labels)


def gaussian_nll(y, mean, var) -> float:
    """the mean negative log density of y under N(mean, var), float64"""
    y, mean, var = (torch.as_tensor(t).double().reshape(-1) for t in (y, mean, var))
    return float((0.5 * (torch.log(2.0 * math.pi * var) + (y - mean) ** 2 / var)).mean())


def eval_dataset_closed_form_grid(state, dataloader: Iterable, Z, alpha, scales, full_set_size, model_type="classifier",
                                  posterior: str = "kfac", link: str = "probit", num_samples: int = 1000, seed: int = 0,
                                  indices=None, rank=None, *, curvature=None, route=None):
    """:func:`eval_dataset_closed_form` (``cov="diag"``) at the priors s_g ``alpha`` for every s_g of ``scales``: a list
    of G tuples (NLL, accuracy, Brier, ECE).  ``posterior="kfac"`` / ``"ekfac"``: ONE pass over the loader and one fit
    at ``alpha``; per batch one grid predictive (``lla.predict_lla_kfac_grid`` / ``predict_lla_ekfac_grid``) and G calls
    of ``link.link_predictive`` on (f_mean, f_var[g]), batch b drawn with ``example_offset`` = the number of points
    before it, as :func:`eval_dataset_closed_form` draws.  Every other closed-form posterior loops that function at
    s_g ``alpha`` (a :class:`prior.GroupedPrior` scaled by ``with_values``), so ``dataloader`` must then be re-iterable.
    ``model_type="regressor"``: NLL is the Gaussian one at variance f_var + exp(logvar), the other three entries nan."""
    from .kfac import checked_scales
    from .link import link_predictive
    scales = checked_scales(scales)
    regressor = model_type == "regressor"
    if posterior not in ("kfac", "ekfac"):
        if regressor:
            raise ValueError("the regressor's Gaussian NLL on a grid is computed for posterior='kfac' and 'ekfac' only")
        return [eval_dataset_closed_form(state, dataloader, Z, scaled_prior(alpha, s), full_set_size, model_type, posterior,
                                         link, "diag", num_samples, seed, indices, rank, curvature=curvature,
                                         route=route)[:4] for s in scales]
    from .lla import predict_lla_ekfac_grid, predict_lla_kfac_grid
    predict = predict_lla_kfac_grid if posterior == "kfac" else predict_lla_ekfac_grid
    kw = {} if curvature is None else {"curvature": curvature}
    if route is not None:
        kw["route"] = route
    G = len(scales)
    parts, all_labels, offset = [[] for _ in range(G)], [], 0
    for x_b, y_b in dataloader:
        f_mean, f_var = predict(state, x_b, Z, model_type, alpha, scales, full_set_size=full_set_size, **kw)
        for g in range(G):
            if regressor:
                parts[g].append(torch.stack([f_mean.reshape(-1), f_var[g].reshape(-1)]))
            else:
                parts[g].append(link_predictive(f_mean, f_var[g], link=link, num_samples=num_samples, seed=seed,
                                                example_offset=offset))
        all_labels.append(y_b.reshape(-1).to(f_mean.device))
        offset += int(x_b.shape[0])
    labels = torch.cat(all_labels)
    if regressor:
        from .ggn import _logvar
        noise = math.exp(_logvar(state))
        out = []
        for g in range(G):
            mv = torch.cat(parts[g], dim=1)
            out.append((gaussian_nll(labels, mv[0], mv[1] + noise), float("nan"), float("nan"), float("nan")))
        return out
    return [_classifier_metrics(torch.cat(parts[g]), labels.long()) for g in range(G)]


OOD_SCORES = ("max_prob", "entropy", "mutual_information")


def auroc_ood_closed_form(state, id_loader: Iterable, ood_loader: Iterable, Z, alpha, full_set_size,
                          model_type="classifier", posterior: str = "diag", link: str = "probit", cov: str = "diag",
                          score: str = "max_prob", num_samples: int = 1000, seed: int = 0, indices=None, rank=None, *,
                          curvature=None, route=None) -> float:
    """:func:`auroc_ood` for the closed-form predictives: AUROC of in-distribution (label 0) against OOD (label 1) points
    under ``score`` = ``"max_prob"`` (:func:`ood_scores`), ``"entropy"`` (H of the predictive) or
    ``"mutual_information"`` (the epistemic part of the entropy, ``link="mc"`` only: it needs the draws).  Both loaders go
    through :func:`eval_dataset_closed_form`'s predictive and link; the OOD points are drawn after the in-distribution
    ones (``example_offset`` continues), so no two points share a stream."""
    if score not in OOD_SCORES:
        raise ValueError(f"score must be one of {OOD_SCORES}, got {score!r}")
    if score == "mutual_information" and link != "mc":
        raise ValueError("score='mutual_information' needs the draws of link='mc'")
    predict = _closed_form_predict(posterior, cov, indices, rank, curvature, route)
    want_mi = score == "mutual_information"
    scores, counts, offset = [], [], 0
    for loader in (id_loader, ood_loader):
        part = []
        for out, _ in _closed_form_batches(state, loader, Z, alpha, full_set_size, model_type, predict, link, num_samples,
                                           seed, offset, uncertainty=want_mi):
            if want_mi:
                part.append(out[1]["epistemic"])
            elif score == "entropy":
                part.append(-torch.xlogy(out, out).sum(-1))
            else:
                part.append(ood_scores(out))
        part = torch.cat(part)
        scores.append(part)
        counts.append(len(part))
        offset += len(part)
    labels = torch.cat([torch.zeros(counts[0]), torch.ones(counts[1])])
    return roc_auc(labels, torch.cat(scores))
