"""CPU checks of the low-rank Laplace posterior: ``distributions.LowRankNormal`` on float64 CPU tensors against dense
inverses (scalar and two-group prior), the evidence of the truncated spectrum against ``slogdet`` of the truncated
precision, and the properties of the float64 helper (``tests/lowrank_ref.py``) that make it a yardstick for the GPU
tests: Ritz values below the exact ones, the prescribed-operator recovery, and the two conditions of ``check_case`` on
every net at the ranks the GPU tests use.
"""
import functools
import math

import pytest
import torch

import last_layer_kron_ref as kref
import last_layer_ref as ref
import lowrank_ref as lr
from lip_amd.distributions import LowRankNormal
from lip_amd.train_alpha import _lml_from_spectrum
from lip_amd.utils import flatten_nn_params

F64 = torch.float64
SMALL = ["sine_regressor", "xor_classifier", "flat_head"]          # D <= 354: dense D x D inverses are cheap
N_FULL = kref.N_FULL


@functools.lru_cache(maxsize=None)
def _case(name):
    state, Z, model_type = kref.make_case(name)
    W = lr.factor(state, Z, model_type)
    flat = flatten_nn_params(state.params)[0].detach().to(F64)
    lam_exact, _ = lr.exact_eigh(W)
    alpha = 1e-3 * (N_FULL / Z.shape[0]) * float(lam_exact[0])
    Xnew = kref.new_points(Z, 4, 7)
    _, J = ref.jac64(state, Xnew, model_type)
    return dict(state=state, Z=Z, model_type=model_type, W=W, flat=flat, lam_exact=lam_exact, alpha=alpha, J=J, D=W.shape[1])


def _fit(name, grouped):
    """(lam_t, U, prior vector or number) from the helper's subspace iteration at the net's configured rank"""
    c = _case(name)
    rank, _ = lr.CONFIG[name]
    nm = N_FULL / c["Z"].shape[0]
    if grouped:
        a = kref.split_prior(c["state"], c["alpha"]).vector("cpu", F64)
        lam, U, info = lr.subspace_iteration(lr.operator(c["W"], a.rsqrt()), lr.probes_for(name, c["D"]), rank)
        return lr.whiten(lam, nm), U, a
    lam, U, info = lr.subspace_iteration(lr.operator(c["W"]), lr.probes_for(name, c["D"]), rank)
    return lr.whiten(lam, nm, c["alpha"]), U, c["alpha"]


def _rel(v, r):
    return float((v - r).abs().max() / r.abs().max())


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_covariance_variance_and_products_match_the_dense_inverse(name, grouped):
    c = _case(name)
    lam_t, U, a = _fit(name, grouped)
    post = LowRankNormal(c["flat"], U, lam_t, a)
    Sigma = lr.sigma_dense(U, lam_t, a)
    D = c["D"]
    assert torch.equal(post.mean(), c["flat"]) and torch.equal(post.spectrum(), lam_t)
    assert _rel(post.cov_vp(torch.eye(D, dtype=F64)), Sigma) <= 1e-12
    assert _rel(lr.sigma_closed(U, lam_t, a), Sigma) <= 1e-12
    var = post.variance()
    assert var.dtype == F64 and var.shape == (D,)
    assert _rel(var, torch.diagonal(Sigma)) <= 1e-12
    assert _rel(post.stddev() ** 2, torch.diagonal(Sigma)) <= 1e-12
    g = torch.Generator().manual_seed(3)
    V = torch.randn(5, D, generator=g, dtype=F64)
    assert _rel(post.cov_vp(V), V @ Sigma) <= 1e-12
    assert _rel(post.cov_vp(V[0]), Sigma @ V[0]) <= 1e-12
    # truncation never under-states the variance: every direction left out keeps the prior's
    prior_var = 1.0 / lr.prior_vector(a, D)
    assert bool((var <= prior_var * (1 + 1e-12)).all()) and bool((var > 0).all())
    more = LowRankNormal(c["flat"], U[:-1], lam_t[:-1], a).variance()
    assert bool((more >= var * (1 - 1e-12)).all())


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_the_sample_map_has_the_posterior_covariance(name, grouped):
    c = _case(name)
    lam_t, U, a = _fit(name, grouped)
    post = LowRankNormal(c["flat"], U, lam_t, a)
    D = c["D"]
    Lt = post.sample_map(torch.eye(D, dtype=F64))            # row i = (L e_i)^T: the matrix L^T
    assert _rel(Lt.T @ Lt, lr.sigma_dense(U, lam_t, a)) <= 1e-12
    assert _rel(Lt, lr.sample_map_ref(torch.eye(D, dtype=F64), U, lam_t, a)) <= 1e-12
    x = post.sample((3, 2), seed=5)
    assert x.shape == (3, 2, D) and x.dtype == F64 and torch.equal(x, post.sample((3, 2), seed=5))
    eps = torch.randn(6, D, dtype=F64, generator=torch.Generator().manual_seed(5))
    assert _rel(x.reshape(6, D) - c["flat"], lr.sample_map_ref(eps, U, lam_t, a)) <= 1e-12


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_predictive_formula_matches_j_sigma_jt(name, grouped):
    """var_k = J A0^-1 J^T - sum_j s_j (J A0^(-1/2) ut_j)^2 is J Sigma J^T"""
    c = _case(name)
    lam_t, U, a = _fit(name, grouped)
    Sigma = lr.sigma_dense(U, lam_t, a)
    want = c["J"] @ Sigma @ c["J"].transpose(1, 2)
    assert _rel(lr.predict_ref(c["J"], U, lam_t, a), want) <= 1e-12
    post = LowRankNormal(c["flat"], U, lam_t, a)
    B, K, D = c["J"].shape
    got = (post.cov_vp(c["J"].reshape(B * K, D)).reshape(B, K, D) @ c["J"].transpose(1, 2))
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_evidence_is_the_slogdet_of_the_truncated_precision(name):
    c = _case(name)
    rank, _ = lr.CONFIG[name]
    lam, U, _ = lr.subspace_iteration(lr.operator(c["W"]), lr.probes_for(name, c["D"]), rank)
    nm = N_FULL / c["Z"].shape[0]
    theta2 = float((c["flat"] ** 2).sum())
    for alpha in (c["alpha"], 7.0 * c["alpha"]):
        lam_t = lr.whiten(lam, nm, alpha)
        sign, logdet = torch.linalg.slogdet(lr.precision_dense(U, lam_t, alpha))
        want = -0.5 * alpha * theta2 + 0.5 * c["D"] * math.log(alpha) - 0.5 * float(logdet)
        got, _ = _lml_from_spectrum(alpha, lam, c["D"], theta2, nm)
        assert float(sign) == 1.0 and abs(got - want) <= 1e-10 * abs(want)
        assert abs(lr.lml_ref(alpha, lam, c["D"], theta2, nm) - want) <= 1e-10 * abs(want)
        post = LowRankNormal(c["flat"], U, lam_t, alpha)
        assert abs(float(post.log_det_precision_ratio()) - (float(logdet) - c["D"] * math.log(alpha))) <= 1e-9 * abs(float(logdet))


def test_constructor_refusals():
    loc = torch.zeros(6, dtype=F64)
    U = torch.eye(6, dtype=F64)[:2]
    lam = torch.ones(2, dtype=F64)
    with pytest.raises(ValueError):
        LowRankNormal(loc, U[:, :5], lam, 1.0)
    with pytest.raises(ValueError):
        LowRankNormal(loc, U, lam[:1], 1.0)
    with pytest.raises(ValueError):
        LowRankNormal(loc, U, lam, torch.ones(5, dtype=F64))
    with pytest.raises(ValueError):
        LowRankNormal(loc, U, lam, 0.0)
    empty = LowRankNormal(loc, U[:0], lam[:0], 2.0)                    # no pairs: the prior
    assert torch.equal(empty.variance(), torch.full((6,), 0.5, dtype=F64))
    assert _rel(empty.cov_vp(torch.ones(6, dtype=F64)), torch.full((6,), 0.5, dtype=F64)) <= 1e-15


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("name", lr.NETS)
def test_helper_conditions_hold_at_the_configured_ranks(name):
    """(a) no row dropped, (b) a gap after the rank, for the scalar and the two-group prior; Ritz values never exceed
    the exact eigenvalues, and their sum never exceeds the trace"""
    c = _case(name)
    rank, over = lr.CONFIG[name]
    probes = lr.probes_for(name, c["D"])
    assert probes.shape == (rank + over, c["D"])
    a = kref.split_prior(c["state"], c["alpha"]).vector("cpu", F64)
    for isq in (None, a.rsqrt()):
        lam_exact, U_exact = lr.exact_eigh(c["W"], isq)
        lam, U, info = lr.subspace_iteration(lr.operator(c["W"], isq), probes, rank)
        ratio = lr.check_case(lam_exact, rank, info)
        print(f"{name}: gap ratio {ratio:.3f}, Ritz / exact {(lam / lam_exact[:rank]).tolist()}")
        assert info["passes"] == 3 and lam.shape == (rank,) and U.shape == (rank, c["D"])
        assert bool((lam[:-1] >= lam[1:]).all())
        assert bool((lam <= lam_exact[:rank] * (1 + 1e-12)).all())
        trace = float((c["W"] ** 2).sum()) if isq is None else float(((c["W"] * isq) ** 2).sum())
        assert float(lam.sum()) <= trace
        assert _rel(U @ U.T, torch.eye(rank, dtype=F64)) <= 1e-12
        assert float(info["residual"].max()) < 0.1
    if c["D"] <= 400:
        G = lr.dense(c["W"])
        assert _rel(torch.linalg.eigvalsh(G).flip(0)[:rank], lr.exact_eigh(c["W"])[0][:rank]) <= 1e-12
        V = torch.randn(3, c["D"], dtype=F64, generator=torch.Generator().manual_seed(1))
        assert _rel(lr.operator(c["W"])(V), V @ G) <= 1e-12


def prescribed_operator(N, lam, seed):
    """a dense symmetric N x N matrix with the eigenvalues ``lam`` on random orthonormal directions: (A, V (len, N))"""
    g = torch.Generator().manual_seed(seed)
    V = torch.linalg.qr(torch.randn(N, lam.numel(), generator=g, dtype=F64)).Q.T
    return V.T @ (lam[:, None] * V), V


def test_helper_recovers_a_rank_12_operator_without_power_iterations():
    """rank 12, a 3-decade spectrum, P = 16, power_iters = 0: the range of A Omega is the range of A, so the projection
    is exact; the four surplus rows are dropped"""
    N = 300
    lam = torch.logspace(0, -3, 12, dtype=F64)
    A, V = prescribed_operator(N, lam, 0)
    probes = torch.randn(16, N, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    got, U, info = lr.subspace_iteration(lambda X: X @ A, probes, 12, power_iters=0)
    assert info["dropped"] == [4] and info["passes"] == 2
    assert _rel(got, lam) <= 1e-10
    assert _rel(lr.projector(U), V.T @ V) <= 1e-10
    assert float(info["residual"].max()) <= 1e-10
    got0, U0, info0 = lr.subspace_iteration(lambda X: X @ torch.zeros(N, N, dtype=F64), probes, 12)
    assert got0.numel() == 0 and U0.shape == (0, N) and info0["passes"] == 1
