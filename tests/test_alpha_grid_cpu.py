"""CPU checks of the validation grid search of the prior precision: the schedule of ``train_alpha.grid_search_alpha``
against hand-worked cases, the rescaling identity behind the one-fit grid (``kfac.rescale_fit``) against the float64
helpers' dense covariances at the scaled prior, and the grid variance formula against the rescaled triples.

Identity: for a prior s a the whitened factor D A D only scales, so (V / sqrt(s), 1 / (Ev / s + 1), Ub) is the fit at
s a.  Everything is float64 on the host; the helper's alpha keeps the condition of every dense solve at most 1002, scales
>= 1 only lower it, and the bound 1e-11 max|ref| is that of tests/test_kfac_cpu.py for this comparison.
"""
import functools
import math

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import ekfac, evaluate, kfac, train_alpha
from lip_amd.distributions import KroneckerNormal
from lip_amd.prior import GroupedPrior

F64 = torch.float64
TOL = 1e-11
N_FULL = kf.N_FULL
SCALES = (1.0, 3.5, 12.0)
COARSE = [-3.0 + 5.0 * i / 6.0 for i in range(7)]           # -3, -2.1667, -1.3333, -0.5, 0.3333, 1.1667, 2


# ------------------------------------------------------------------------------------------------ the schedule
def _search(monkeypatch, t, **kw):
    """grid_search_alpha on the parabola (log10(alpha) - t)^2, with the alphas eval_dataset was asked for"""
    seen = []

    def fake(state, loader, Z, alpha, full_set_size, model_type, num_mc_samples, rng, scalable=True):
        seen.append((float(alpha), rng, num_mc_samples, scalable, full_set_size, model_type))
        return (math.log10(alpha) - t) ** 2, 0.0

    monkeypatch.setattr(evaluate, "eval_dataset", fake)
    out = train_alpha.grid_search_alpha("state", "Z0", [], 40, "classifier", verbose=False, rng_key=7, **kw)
    return out, seen


def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


@pytest.mark.parametrize("t,want,evals", [
    (-0.4, -0.5, [-0.5 - 5.0 / 12.0, -0.5, -0.5 + 5.0 / 12.0]),      # the tie at -0.5 goes to the coarse point
    (-0.1, -0.5 + 5.0 / 12.0, [-0.5 - 5.0 / 12.0, -0.5, -0.5 + 5.0 / 12.0]),   # the refinement improves on the coarse best
    (-5.0, -3.0, [-3.0 + 5.0 / 24.0, -3.0 + 5.0 / 12.0, -3.0 + 5.0 / 8.0]),    # left end: the end point and its neighbour
    (4.0, 2.0, [2.0 - 5.0 / 8.0, 2.0 - 5.0 / 12.0, 2.0 - 5.0 / 24.0]),         # right end
])
def test_schedule_is_the_reference_one(monkeypatch, t, want, evals):
    (alpha, history), seen = _search(monkeypatch, t, return_history=True)
    assert isinstance(alpha, float) and _close(alpha, 10.0 ** want)
    assert len(seen) == 10 and len(history) == 10                     # 7 coarse + 3 refined evaluations
    for (a, *_), lg in zip(seen, COARSE + evals):
        assert _close(a, 10.0 ** lg), (a, lg)
    # the history is in evaluation order and holds what the evaluation returned
    assert [a for a, _ in history] == [s[0] for s in seen]
    assert all(v == (math.log10(a) - t) ** 2 for a, v in history)
    # the first minimum over coarse-then-refined wins
    nlls = [v for _, v in history]
    assert alpha == history[nlls.index(min(nlls))][0]
    if t == -0.4 and history[8][1] == history[3][1]:                  # an exact tie in floating point too:
        assert alpha == history[3][0]                                 # the coarse point itself, not the refined twin
    # every evaluation got the search's own arguments, the rng included
    assert all(s[1:] == (7, 30, True, 40, "classifier") for s in seen)


def test_schedule_without_refinement_and_with_other_grids(monkeypatch):
    alpha, seen = _search(monkeypatch, -0.4, refine=False)
    assert len(seen) == 7 and _close(alpha, 10.0 ** -0.5)
    (alpha, history), seen = _search(monkeypatch, 0.2, log10_min=-1, log10_max=1, n_coarse=3, return_history=True)
    assert [round(math.log10(s[0]), 12) for s in seen] == [-1.0, 0.0, 1.0, -0.5, 0.0, 0.5]
    assert _close(alpha, 1.0) and alpha == history[1][0]
    from lip_amd import grid_search                                   # the reference's module name
    assert grid_search.grid_search_alpha is train_alpha.grid_search_alpha
    assert train_alpha.refinement_points([1e-3, 1e2], 0) == train_alpha.refinement_points([1e-3, 1e2], 1)
    with pytest.raises(ValueError, match="at least two"):
        train_alpha.refinement_points([1.0], 0)


def test_grouped_base_prior_is_scaled_as_a_whole(monkeypatch):
    base = GroupedPrior.from_table([("a", [(0, 3)]), ("b", [(3, 5)])], [0.5, 2.0], 8)
    seen = []

    def fake(state, loader, Z, alpha, full_set_size, model_type, num_mc_samples, rng, scalable=True):
        seen.append(alpha)
        return (math.log10(float(alpha.values[0]) / 0.5) + 0.4) ** 2, 0.0

    monkeypatch.setattr(evaluate, "eval_dataset", fake)
    out, history = train_alpha.grid_search_alpha("state", "Z0", [], 40, "classifier", verbose=False, alpha_base=base,
                                                 return_history=True)
    assert isinstance(out, GroupedPrior) and out.table == base.table and len(seen) == 10
    s = 10.0 ** -0.5
    assert torch.allclose(out.values, base.values * s, rtol=1e-12, atol=0.0)
    assert all(isinstance(a, GroupedPrior) for a, _ in history)
    assert evaluate.scaled_prior(2.0, 3.0) == 6.0 and torch.equal(evaluate.scaled_prior(base, 3.0).values, base.values * 3.0)


def test_scales_are_checked_before_anything_is_bound():
    state, Z, model_type = kf.make_case("xor_classifier")
    for bad in ([], [0.0], [-1.0], [float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="finite positive"):
            kfac.predict_lla_kfac_grid(state, Z[:2], Z, model_type, 1.0, bad)
        with pytest.raises(ValueError, match="finite positive"):
            ekfac.predict_lla_ekfac_grid(state, Z[:2], Z, model_type, 1.0, bad)
        with pytest.raises(ValueError, match="finite positive"):
            evaluate.eval_dataset_closed_form_grid(state, [], Z, 1.0, bad, N_FULL)
    with pytest.raises(ValueError, match="'rows' or 'sweep'"):
        kfac.predict_lla_kfac_grid(state, Z[:2], Z, model_type, 1.0, [1.0], route="columns")
    with pytest.raises(ValueError, match="finite positive"):
        kfac.rescale_fit([], [], (None, torch.ones(1), torch.ones(1)), 0.0)


# ------------------------------------------------------------------------------------------------ the identity
NETS = kf.DENSE_ONLY + ["resnet_tiny"]


@functools.lru_cache(maxsize=None)
def _helper(name):
    """the float64 helper's factors, rows and base alpha, built once per net and never written to"""
    state, Z, model_type = kf.make_case(name)
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    _, J, H = er.jacobian(state, Z, model_type)
    return dict(state=state, Z=Z, model_type=model_type, As=As, Ss=Ss, M=M, alpha=alpha, J=J, H=H,
                recal=ref.recal(state, M, model_type, N_FULL), diag=kf.ggn_diag_ref(state, Z, model_type, N_FULL),
                rem=kf.remainder_of(state))


def _base_fit(h, grouped):
    state, model_type, alpha = h["state"], h["model_type"], h["alpha"]
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    table = kfac.block_table(state)
    rows = [kfac.block_prior_rows(prior, b, a.numel()) for b in table]
    fits = kfac.fit_blocks(table, h["As"], h["Ss"], rows, h["recal"], h["M"], model_type != "regressor")
    return table, fits, a, (h["rem"], a[h["rem"]], h["diag"][h["rem"]])


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", NETS)
def test_rescaled_kfac_fit_is_the_dense_posterior_at_the_scaled_prior(name, grouped):
    h = _helper(name)
    table, fits, a, rem = _base_fit(h, grouped)
    Evs = kfac.block_eigenvalues(fits)
    worst = 0.0
    for s in SCALES:
        triples, rem_var = kfac.rescale_fit(fits, Evs, rem, s)
        cov_blocks, _ = kf.covariance_blocks(h["state"], h["As"], h["Ss"], h["M"], h["model_type"], s * a, N_FULL)
        for b, (V, R, Ub), (off, S) in zip(table, triples, cov_blocks):
            assert off == b.off and V.is_contiguous() and R.is_contiguous()
            worst = max(worst, _err(KroneckerNormal(torch.zeros(b.Mt * b.N, dtype=F64), V, R, Ub).covariance(), S))
        assert _err(rem_var, 1.0 / (s * a[h["rem"]] + h["diag"][h["rem"]])) <= 1e-15 if h["rem"].numel() else rem_var.numel() == 0
        if s == 1.0:                                                      # the fit itself, to the rounding of 1 / (Ev + 1)
            assert all(_err(t[1], f[1]) <= 1e-15 and torch.equal(t[0], f[0]) for t, f in zip(triples, fits))
    print(f"{name} {'grouped' if grouped else 'scalar'}: rescaled KFAC fit against the dense route {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", NETS)
def test_rescaled_ekfac_fit_is_the_helper_posterior_in_the_rescaled_basis(name, grouped):
    """Ev = recal Lam from the helper's rows in the base basis; the reference forms Lam_s from the rows in the basis
    (V / sqrt(s), Ub) itself and the dense covariance of ``ekfac_ref.dense_covariance``"""
    h = _helper(name)
    table, fits, a, rem = _base_fit(h, grouped)
    bases = [(f[0], f[2]) for f in fits]
    Lams = er.scales_ref(h["J"], h["H"], h["state"], bases)
    Evs = ekfac.block_eigenvalues(Lams, h["recal"])
    base = ekfac.corrected_fits(fits, Lams, h["recal"])
    worst = 0.0
    for s in SCALES:
        triples, _ = kfac.rescale_fit(base, Evs, rem, s)
        scaled = [(V / math.sqrt(s), Ub) for V, Ub in bases]
        want = er.covariance_blocks(h["state"], scaled, er.scales_ref(h["J"], h["H"], h["state"], scaled), h["recal"])
        for b, (V, R, Ub), (_, S) in zip(table, triples, want):
            worst = max(worst, _err(KroneckerNormal(torch.zeros(b.Mt * b.N, dtype=F64), V, R, Ub).covariance(), S))
        if s == 1.0:
            assert all(_err(t[1], f[1]) <= 1e-15 for t, f in zip(triples, base))
    print(f"{name} {'grouped' if grouped else 'scalar'}: rescaled EKFAC fit against the helper {worst:.2e}")
    assert worst <= TOL


def test_grid_variance_formula_is_the_predictive_of_the_rescaled_triples():
    """sum T^2 / (Ev + s) with T = V^T J Ub in the base basis is diag(J Sigma_s J^T) for the rescaled (V, R, Ub)"""
    g = torch.Generator().manual_seed(5)
    Mt, N, B = 7, 4, 6
    V = torch.randn(Mt, Mt, generator=g, dtype=F64)
    Ub = torch.randn(N, N, generator=g, dtype=F64)
    Ev = 5.0 * torch.rand(Mt, N, generator=g, dtype=F64)
    Ev[0] = 0.0
    J = torch.randn(B, Mt, N, generator=g, dtype=F64)
    idx = torch.arange(3)
    a_rem, h_rem = torch.rand(3, generator=g, dtype=F64) + 0.5, torch.rand(3, generator=g, dtype=F64)
    Jd = torch.randn(B, 3, generator=g, dtype=F64)
    T = V.T @ J @ Ub
    for s in (0.03, 1.0, 3.5, 40.0):
        got = (T * T / (Ev + s)).sum((1, 2)) + (Jd * Jd) @ (1.0 / (s * a_rem + h_rem))
        [(Vs, Rs, Us)], rem_var = kfac.rescale_fit([(V, None, Ub)], [Ev], (idx, a_rem, h_rem), s)
        Sigma = KroneckerNormal(torch.zeros(Mt * N, dtype=F64), Vs, Rs, Us).covariance()
        Jf = J.reshape(B, Mt * N)
        want = torch.einsum("bd,de,be->b", Jf, Sigma, Jf) + (Jd * Jd) @ rem_var
        assert _err(got, want) <= 1e-12
