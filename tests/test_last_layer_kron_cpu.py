"""CPU checks of the Kronecker-factored last-layer posterior: the package's host algebra (``last_layer_kron.py``,
``distributions.KroneckerNormal``), fed the float64 helper's factors on the CPU, against the helper's dense route
(``tests/last_layer_kron_ref.py``: ``torch.kron`` and a dense solve), and the refusals.

Everything is float64 on the host.  alpha = 1e-3 c lam_max(A) mu_max(Bf) keeps the condition of the dense solve at most
1002 (asserted by the helper), so the bound 1e-11 max|ref| is 100 cond 2^-53; the worst figure seen over the cases below
was 1.1e-13 (the dense covariance of flat_head).
"""
import functools
import math

import pytest
import torch

import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import last_layer_kron as llk
from lip_amd.distributions import KroneckerNormal
from lip_amd.ggn import compute_ggn_last_layer
from lip_amd.last_layer import LAST_LAYER_MAX_DIM, last_layer_slice
from lip_amd.lla import posterior_lla_last_layer, posterior_lla_last_layer_kron, predict_lla_last_layer_kron
from lip_amd.netspec import NetSpec
from lip_amd.prior import GroupedPrior
from lip_amd.toymodels import create_state
from lip_amd.utils import flatten_nn_params

F64 = torch.float64
TOL = 1e-11


@functools.lru_cache(maxsize=None)
def _setup(name, grouped):
    """everything both routes need, built once: the helper's factors, the prior rows and the dense covariance"""
    state, Z, model_type = kref.make_case(name)
    off, F, K = last_layer_slice(state)
    A, Bf, M = kref.factors_ref(state, Z, model_type)
    c = kref.c_of(state, M, model_type, kref.N_FULL)
    alpha = kref.alpha_for(A, Bf, c)
    D = flatten_nn_params(state.params)[0].numel()
    prior = kref.split_prior(state, alpha) if grouped else alpha
    a_rows = llk.prior_rows(prior, off, F, K, D)
    if grouped:
        assert float(a_rows[0]) == alpha and bool((a_rows[1:] == 2.0 * alpha).all())
        assert torch.equal(a_rows.repeat_interleave(K), prior.vector("cpu", F64)[off:off + (F + 1) * K])
    S, logdet = kref.covariance_dense(A, Bf, c, a_rows, model_type)
    V, R, Ub, lam, mu = llk.factor_posterior(A, Bf, a_rows, c, model_type != "regressor")
    loc = torch.zeros((F + 1) * K, dtype=F64)
    return state, Z, model_type, (F, K), S, logdet, KroneckerNormal(loc, V, R, Ub, spectrum=(lam, mu, c))


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kref.NETS)
def test_factored_algebra_matches_the_dense_route(name, grouped):
    state, Z, model_type, (F, K), S, logdet, post = _setup(name, grouped)
    e_cov = _err(post.covariance(), S)
    e_var = _err(post.variance(), torch.diagonal(S))
    _, phit, _ = ref.features64(state, kref.new_points(Z, 5, 7))
    want = kref.predict_dense(phit, S, K)
    full = llk.predictive_cov(phit, post.V, post.R, post.Ub, diag=False)
    dg = llk.predictive_cov(phit, post.V, post.R, post.Ub, diag=True)
    e_full = _err(full, want)
    e_diag = _err(dg, torch.diagonal(want, dim1=1, dim2=2))
    got_ld = float(post.log_det_precision_ratio())
    e_ld = abs(got_ld - logdet) / abs(logdet)
    e_ld_r = abs(float(KroneckerNormal(post.loc, post.V, post.R, post.Ub).log_det_precision_ratio()) - logdet) / abs(logdet)
    print(f"{name} {'grouped' if grouped else 'scalar'}: cov {e_cov:.2e} var {e_var:.2e} predictive {e_full:.2e} "
          f"diag {e_diag:.2e} logdet {e_ld:.2e} (from R alone {e_ld_r:.2e})")
    assert post.covariance().shape == S.shape and post.variance().shape == (S.shape[0],)
    assert torch.equal(post.stddev(), torch.sqrt(post.variance()))
    assert max(e_cov, e_var, e_full, e_diag, e_ld, e_ld_r) <= TOL


@pytest.mark.parametrize("name,n", [("sine_regressor", None), ("xor_classifier", 1), ("mlp_ragged", 1)])
def test_kronecker_curvature_is_exact_for_the_gaussian_head_and_one_example(name, n):
    state, Z, model_type = kref.make_case(name)
    Z = Z if n is None else Z[:n]
    A, Bf, M = kref.factors_ref(state, Z, model_type)
    G = kref.c_of(state, M, model_type, kref.N_FULL) * torch.kron(A, Bf)
    G_ref = ref.ggn_last_layer_ref(state, Z, model_type, full_set_size=kref.N_FULL)
    assert _err(G, G_ref) <= 1e-12


def test_evidence_spectrum_is_the_outer_product_of_the_factor_spectra():
    """sum log1p over ``kron_spectrum`` equals the log-determinant of the dense route at N/M = 1"""
    state, Z, model_type, (F, K), S, logdet, post = _setup("xor_classifier", False)
    A, Bf, M = kref.factors_ref(state, Z, model_type)
    alpha = kref.alpha_for(A, Bf, kref.c_of(state, M, model_type, kref.N_FULL))
    spec = llk.kron_spectrum(torch.linalg.eigvalsh(A).clamp_min(0.0), torch.linalg.eigvalsh(llk.centre(Bf)).clamp_min(0.0), M)
    assert spec.shape == ((F + 1) * K,)
    from lip_amd.train_alpha import _lml_from_spectrum
    got = _lml_from_spectrum(alpha, spec, (F + 1) * K, 2.5, kref.N_FULL / M)[0]
    assert abs(got - (-0.5 * alpha * 2.5 - 0.5 * logdet)) <= TOL * abs(logdet)


def test_sample_moments_match_the_variance():
    """20 000 seeded draws: every component's mean within 5 sqrt(var / n) and second moment within 5 var sqrt(2 / n)"""
    *_, post = _setup("mlp_ragged", True)
    n = 20000
    x = post.sample((n,), seed=3)
    assert x.shape == (n, post.loc.numel()) and x.dtype == F64
    assert torch.equal(x, post.sample(n, seed=3))
    var = post.variance()
    z = x - post.mean()
    assert bool((z.mean(0).abs() <= 5.0 * torch.sqrt(var / n)).all())
    assert bool(((z * z).mean(0) - var).abs().le(5.0 * var * math.sqrt(2.0 / n)).all())
    # and one cross moment per row block: the draws carry the covariance, not the variances alone
    S = post.covariance()
    emp = z.T @ z / n
    se = torch.sqrt((S * S + var[:, None] * var[None, :]) / n)
    assert bool(((emp - S).abs() <= 5.5 * se).all())


def _oversize_state():
    net = NetSpec((6,))
    net.dense(net.dense(0, "Dense_0", 127, act="relu"), "Dense_1", 100)
    return create_state(net, 0, dtype=F64)


def test_prior_varying_along_k_is_refused():
    state, Z, model_type = kref.make_case("xor_classifier")
    off, F, K = last_layer_slice(state)
    D = flatten_nn_params(state.params)[0].numel()
    cut = off + K + 1                                              # inside kernel row 0
    table = [("a", [(0, cut)]), ("b", [(cut, D - cut)])]
    prior = GroupedPrior.from_table(table, [1.0, 2.0], D)
    with pytest.raises(ValueError, match="constant along"):
        llk.prior_rows(prior, off, F, K, D)
    with pytest.raises(ValueError, match="constant along"):       # before any engine is bound: runs without a GPU
        posterior_lla_last_layer_kron(state, Z, model_type, prior)
    same = GroupedPrior.from_table(table, [1.5, 1.5], D)           # the same cut with equal values does not vary
    assert bool((llk.prior_rows(same, off, F, K, D) == 1.5).all())
    tensor = GroupedPrior(state.params, 2.0, "tensor")
    assert bool((llk.prior_rows(tensor, off, F, K, D) == 2.0).all())


def test_cov_argument_is_checked():
    state, Z, model_type = kref.make_case("xor_classifier")
    with pytest.raises(ValueError, match="'diag' or 'full'"):
        predict_lla_last_layer_kron(state, Z[:2], Z, model_type, 1.0, cov="dense")


def test_dense_covariance_is_refused_above_the_cap():
    Ft, K = 91, 91
    assert Ft * K > LAST_LAYER_MAX_DIM
    post = KroneckerNormal(torch.zeros(Ft * K, dtype=F64), torch.eye(Ft, dtype=F64), torch.ones(Ft, K, dtype=F64),
                           torch.eye(K, dtype=F64))
    with pytest.raises(ValueError, match="LAST_LAYER_MAX_DIM"):
        post.covariance()
    assert post.variance().shape == (Ft * K,) and float(post.log_det_precision_ratio()) == 0.0


def test_dense_functions_still_refuse_an_oversize_layer():
    state = _oversize_state()
    Z = torch.randn(4, 6, dtype=F64)
    with pytest.raises(ValueError, match="Kronecker-factored"):
        last_layer_slice(state)
    with pytest.raises(ValueError, match="Kronecker-factored"):
        compute_ggn_last_layer(state, Z, "classifier")
    with pytest.raises(ValueError, match="Kronecker-factored"):
        posterior_lla_last_layer(state, Z, "classifier", 1.0)
    off, F, K = last_layer_slice(state, max_dim=None)
    assert (F, K) == (127, 100) and (F + 1) * K == 12800 > LAST_LAYER_MAX_DIM
    with pytest.raises(ValueError, match="Kronecker-factored"):
        last_layer_slice(state, max_dim=12799)
