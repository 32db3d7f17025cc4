"""GPU checks of the Kronecker-factored last-layer posterior: the kernels ``lip_ll_kron_factors`` /
``lip_ll_kron_predict`` on synthetic operands through ctypes, then the engine method and the public surface
(``last_layer_kron.py``) on the small nets of tests/test_last_layer.py.

Kernel level: the reference is a float64 einsum of the up-cast float32 operands, and the bound is the standard float64
summation bound on the absolute-sum twin of the reference, with a factor 4 for the reference's own rounding (the
convention of tests/test_last_layer.py): 4 (n + 8) 2^-53 for the factors (n-term sums), 4 (3 Ft + K + 8) 2^-53 for the
predictive (an Ft-term sum, squared, an Ft-term sum, a K-term sum).  Both hold for any summation order.

Engine level: the features come from the float32 primal pass, so no bound is derivable; every bound there is 4 x the
worst error measured on MI355X against the float64 helper (``tests/last_layer_kron_ref.py``), with the measured figure
next to it.
"""
import ctypes
import functools

import pytest
import torch

import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import last_layer_kron as llk
from lip_amd.distributions import KroneckerNormal
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache, compute_ggn_last_layer, compute_kron_factors_last_layer, get_engine
from lip_amd.last_layer import LAST_LAYER_MAX_DIM, last_layer_slice
from lip_amd.lla import (posterior_lla_last_layer_kron, predict_lla_last_layer, predict_lla_last_layer_kron,
                         predict_lla_last_layer_kron_scalable)
from lip_amd.netspec import NetSpec
from lip_amd.toymodels import create_state
from lip_amd.train_alpha import fit_alpha_last_layer_kron, log_marginal_likelihood_last_layer_kron
from lip_amd.utils import flatten_nn_params

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -53
DEV = "cuda"
N_FULL = kref.N_FULL


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
def _operands(n, F, K, softmax, seed=0, ldphi=None):
    g = torch.Generator().manual_seed(seed)
    Phi = torch.randn(n, ldphi or F, generator=g, dtype=F32).to(DEV)
    Pr = torch.softmax(torch.randn(n, K, generator=g, dtype=F32), dim=1).to(DEV) if softmax else None
    return Phi, Pr


def _phit(Phi, F):
    return torch.cat([torch.ones(Phi.shape[0], 1, device=Phi.device, dtype=F64), Phi[:, :F].double()], dim=1)


def _factors_reference(Phi, Pr, F, K):
    """(A, |A| twin, Bf, |Bf| twin): float64 einsums of the up-cast operands; the twins are sum_i |phit_f phit_g| and
    sum_i (delta_kl p_k + p_k p_l)"""
    pt = _phit(Phi, F)
    n = Phi.shape[0]
    A, Aabs = pt.T @ pt, pt.abs().T @ pt.abs()
    if Pr is None:
        Bf = Babs = n * torch.eye(K, device=Phi.device, dtype=F64)
    else:
        p = Pr.double()
        Bf = torch.diag(p.sum(0)) - p.T @ p
        Babs = torch.diag(p.sum(0)) + p.T @ p
    return A, Aabs, Bf, Babs


def _scratch(query, n, F, K):
    d = ctypes.c_int64(0)
    nv.check(getattr(nv.load(), query)(n, F, K, ctypes.byref(d)), query)
    return torch.empty(max(1, d.value), device=DEV, dtype=F64)


def _run_factors(Phi, Pr, F, K, A=None, Bf=None, n=None, row0=0):
    lib = nv.load()
    n = Phi.shape[0] - row0 if n is None else n
    A = torch.zeros(F + 1, F + 1, device=DEV, dtype=F64) if A is None else A
    Bf = torch.zeros(K, K, device=DEV, dtype=F64) if Bf is None else Bf
    scratch = _scratch("lip_ll_kron_factors_scratch", n, F, K)
    phi = Phi[row0:]
    pr = None if Pr is None else Pr[row0:]
    nv.check(lib.lip_ll_kron_factors(phi.data_ptr(), Phi.stride(0), 0 if pr is None else pr.data_ptr(), n, F, K,
                                     A.data_ptr(), Bf.data_ptr(), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_ll_kron_factors")
    torch.cuda.synchronize()
    return A, Bf


# (n, F, K, softmax, ldphi)
FACTOR_SHAPES = [
    (1, 1, 1, False, None),            # smallest case, Gaussian head
    (9, 5, 3, True, None),
    (33, 24, 5, True, 27),             # no tile multiple; ldphi = F + 3
    (257, 7, 33, True, None),          # K + 1 above one 32-tile
    (4099, 63, 10, True, None),        # Ft = 64: two tiles per edge, many example ranges
    (4099, 63, 1, False, None),        # many example ranges, Gaussian head
    (1, 4, 33, True, None),            # one example
    (130, 128, 65, True, None),        # Ft and K one past a tile multiple
]


@pytest.mark.parametrize("n,F,K,softmax,ldphi", FACTOR_SHAPES)
def test_kron_factors_against_float64_einsum(n, F, K, softmax, ldphi):
    Phi, Pr = _operands(n, F, K, softmax, seed=n + F + K, ldphi=ldphi)
    A_ref, Aabs, B_ref, Babs = _factors_reference(Phi, Pr, F, K)
    bA, bB = 4 * (n + 8) * U * Aabs, 4 * (n + 8) * U * Babs
    A, Bf = _run_factors(Phi, Pr, F, K)
    eA, eB = (A - A_ref).abs(), (Bf - B_ref).abs()
    print(f"kron factors n={n} F={F} K={K}: max err / bound  A {(eA / bA.clamp_min(1e-300)).max().item():.3f}  "
          f"Bf {(eB / bB.clamp_min(1e-300)).max().item():.3f}")
    assert bool((eA <= bA).all()) and bool((eB <= bB).all())
    assert torch.equal(A, A.T) and torch.equal(Bf, Bf.T)                       # exactly symmetric
    A2, B2 = _run_factors(Phi, Pr, F, K)
    assert torch.equal(A, A2) and torch.equal(Bf, B2)                          # bitwise reproducible
    # pre-filled factors are added to, not overwritten
    g = torch.Generator().manual_seed(1)
    A0 = torch.randn(A.shape, generator=g, dtype=F64).to(DEV)
    B0 = torch.randn(Bf.shape, generator=g, dtype=F64).to(DEV)
    A1, B1 = _run_factors(Phi, Pr, F, K, A=A0.clone(), Bf=B0.clone())
    assert bool(((A1 - A0 - A_ref).abs() <= bA + 4 * U * (A0.abs() + A_ref.abs())).all())
    assert bool(((B1 - B0 - B_ref).abs() <= bB + 4 * U * (B0.abs() + B_ref.abs())).all())
    # two calls on the two halves of the examples add into one pair within the bound
    if n >= 2:
        h = n // 2
        Ah, Bh = _run_factors(Phi, Pr, F, K, n=h)
        Ah, Bh = _run_factors(Phi, Pr, F, K, A=Ah, Bf=Bh, n=n - h, row0=h)
        assert bool(((Ah - A_ref).abs() <= bA).all()) and bool(((Bh - B_ref).abs() <= bB).all())
        assert torch.equal(Ah, Ah.T) and torch.equal(Bh, Bh.T)


def test_kron_factors_status_codes_leave_the_factors_untouched():
    lib = nv.load()
    n, F, K = 9, 5, 3
    Phi, Pr = _operands(n, F, K, True)
    A0 = torch.full((F + 1, F + 1), 7.0, device=DEV, dtype=F64)
    B0 = torch.full((K, K), 5.0, device=DEV, dtype=F64)
    A, Bf = A0.clone(), B0.clone()
    scratch = _scratch("lip_ll_kron_factors_scratch", n, F, K)
    assert scratch.numel() > 1
    good = [Phi.data_ptr(), F, Pr.data_ptr(), n, F, K, A.data_ptr(), Bf.data_ptr(), scratch.data_ptr(), scratch.numel(),
            nv.stream_ptr()]
    for i, v in [(0, 0), (6, 0), (7, 0), (8, 0), (1, F - 1), (9, scratch.numel() - 1), (3, 0), (4, 0), (5, 0), (3, -1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_ll_kron_factors(*args) == 1, (i, v)              # LIP_ERR_ARG
        assert lib.lip_last_error()
        torch.cuda.synchronize()
        assert torch.equal(A, A0) and torch.equal(Bf, B0), (i, v)
    d = ctypes.c_int64(0)
    assert lib.lip_ll_kron_factors_scratch(0, F, K, ctypes.byref(d)) == 1
    assert lib.lip_ll_kron_factors_scratch(n, F, K, None) == 1
    assert lib.lip_ll_kron_factors(*good) == 0


def _spd_factors(F, K, seed):
    """(V, R, Ub) of a random posterior: eigenvectors of two seeded SPD matrices, a random positive row scaling"""
    g = torch.Generator().manual_seed(seed)
    Ft = F + 1
    Ga, Gb = torch.randn(Ft, Ft, generator=g, dtype=F64), torch.randn(K, K, generator=g, dtype=F64)
    lam, Ut = torch.linalg.eigh(Ga @ Ga.T / Ft + torch.eye(Ft, dtype=F64))
    mu, Ub = torch.linalg.eigh(Gb @ Gb.T / K + torch.eye(K, dtype=F64))
    d = 0.5 + torch.rand(Ft, generator=g, dtype=F64)
    R = 1.0 / (torch.outer(lam, mu) + 1.0)
    return (d[:, None] * Ut).contiguous().to(DEV), R.contiguous().to(DEV), Ub.contiguous().to(DEV)


def _run_predict(Phi, F, K, V, R, Ub, diag):
    lib = nv.load()
    B = Phi.shape[0]
    out = torch.full((B, K) if diag else (B, K, K), float("nan"), device=DEV, dtype=F64)
    scratch = _scratch("lip_ll_kron_predict_scratch", B, F, K)
    assert scratch.numel() == B * (F + 1 + K)
    nv.check(lib.lip_ll_kron_predict(Phi.data_ptr(), Phi.stride(0), B, F, K, V.data_ptr(), R.data_ptr(), Ub.data_ptr(),
                                     out.data_ptr(), int(diag), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_ll_kron_predict")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 9, 257])
@pytest.mark.parametrize("F,K,ldphi", [(1, 1, None), (5, 3, None), (24, 5, 27), (7, 33, None), (63, 10, None), (63, 1, None),
                                       (128, 65, None)])
def test_kron_predict_against_float64_einsum(B, F, K, ldphi):
    Phi, _ = _operands(B, F, K, False, seed=B + F + K, ldphi=ldphi)
    V, R, Ub = _spd_factors(F, K, 5)
    pt = _phit(Phi, F)
    cov_ref = torch.einsum("kl,bl,ml->bkm", Ub, (pt @ V) ** 2 @ R, Ub)
    T = torch.einsum("kl,bl,ml->bkm", Ub.abs(), (pt.abs() @ V.abs()) ** 2 @ R, Ub.abs())
    bound = 4 * (3 * (F + 1) + K + 8) * U * T
    full = _run_predict(Phi, F, K, V, R, Ub, diag=False)
    dg = _run_predict(Phi, F, K, V, R, Ub, diag=True)
    err = (full - cov_ref).abs()
    print(f"kron predict B={B} F={F} K={K}: max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(full, full.transpose(1, 2))                  # exactly symmetric in (k, m)
    assert torch.equal(dg, torch.diagonal(full, dim1=1, dim2=2))    # the same code on m = k: bitwise the diagonal


def test_kron_predict_status_codes_leave_out_untouched():
    lib = nv.load()
    B, F, K = 9, 5, 3
    Phi, _ = _operands(B, F, K, False)
    V, R, Ub = _spd_factors(F, K, 5)
    out0 = torch.full((B, K, K), 7.0, device=DEV, dtype=F64)
    out = out0.clone()
    scratch = _scratch("lip_ll_kron_predict_scratch", B, F, K)
    good = [Phi.data_ptr(), F, B, F, K, V.data_ptr(), R.data_ptr(), Ub.data_ptr(), out.data_ptr(), 0, scratch.data_ptr(),
            scratch.numel(), nv.stream_ptr()]
    for i, v in [(0, 0), (5, 0), (6, 0), (7, 0), (8, 0), (10, 0), (1, F - 1), (2, 0), (3, 0), (4, 0), (11, scratch.numel() - 1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_ll_kron_predict(*args) == 1, (i, v)          # LIP_ERR_ARG
        assert lib.lip_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, out0), (i, v)
    d = ctypes.c_int64(0)
    assert lib.lip_ll_kron_predict_scratch(0, F, K, ctypes.byref(d)) == 1
    assert lib.lip_ll_kron_predict_scratch(B, F, K, None) == 1
    assert lib.lip_ll_kron_predict(*good) == 0


# ------------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _case(name):
    """(state, Z, model_type, (offset, F, K)); built once per net and never written to"""
    state, Z, model_type = kref.make_case(name)
    return state, Z, model_type, last_layer_slice(state)


@functools.lru_cache(maxsize=None)
def _helper(name):
    """(A, Bf, M, c, alpha) of the float64 helper at full_set_size = N_FULL, alpha = 1e-3 c lam_max(A) mu_max(Bf)"""
    state, Z, model_type, _ = _case(name)
    A, Bf, M = kref.factors_ref(state, Z, model_type)
    c = kref.c_of(state, M, model_type, N_FULL)
    return A, Bf, M, c, kref.alpha_for(A, Bf, c)


def _rel(v, r):
    r = r.to(v.device)
    return ((v.double() - r).abs().max() / r.abs().max()).item()


# measured on MI355X, max|A - ref| / max|ref| and max|Bf - ref| / max|ref| against the float64 helper:
#   sine_regressor 3.25e-8 / 0, xor_classifier 2.47e-8 / 4.21e-9, mlp_ragged 3.86e-8 / 1.45e-8,
#   resnet_tiny 3.39e-8 / 4.44e-8, resnet50_tiny 1.83e-7 / 6.67e-8, flat_head 1.77e-8 / 1.23e-8
FACTOR_A_TOL = 7.4e-7
FACTOR_B_TOL = 2.7e-7


@pytest.mark.parametrize("name", kref.NETS)
def test_factors_match_the_float64_helper(name):
    state, Z, model_type, (off, F, K) = _case(name)
    A_ref, B_ref, M, _, _ = _helper(name)
    A, Bf, m = compute_kron_factors_last_layer(state, Z, model_type)
    torch.cuda.synchronize()
    assert m == M == Z.shape[0]
    assert A.shape == (F + 1, F + 1) and Bf.shape == (K, K) and A.dtype == Bf.dtype == F64 and A.is_cuda and Bf.is_cuda
    assert torch.equal(A, A.T) and torch.equal(Bf, Bf.T)
    e_a, e_b = _rel(A, A_ref), _rel(Bf, B_ref)
    print(f"{name}: Ft={F + 1} K={K} A {e_a:.2e}  Bf {e_b:.2e}")
    if model_type == "regressor":
        assert torch.equal(Bf.cpu(), B_ref)                        # M I exactly
    assert e_a <= FACTOR_A_TOL and e_b <= FACTOR_B_TOL


def test_engine_method_checks_its_outputs():
    state, Z, model_type, (off, F, K) = _case("xor_classifier")
    eng = get_engine(state, Z, model_type)
    A = torch.zeros(F + 1, F + 1, device=DEV, dtype=F64)
    Bf = torch.zeros(K, K, device=DEV, dtype=F64)
    for bad_a, bad_b in [(A.float(), Bf), (A, Bf.cpu()), (A[:, :F], Bf), (A, torch.zeros(K + 1, K, device=DEV, dtype=F64))]:
        with pytest.raises(ValueError, match="contiguous float64 device matrix"):
            eng.last_layer_kron_factors(bad_a, bad_b)
    eng.last_layer_kron_factors(A, Bf)
    assert "lip_ll_kron_factors_scratch" in eng._scratches          # the scratch is cached on the binding
    assert float(A[0, 0]) == Z.shape[0]                             # sum_i 1 * 1


def test_example_chunks_add_into_one_pair():
    """n = 9 in chunks of 4 (a ragged last chunk): the same float64 operands in another grouping"""
    state, Z, model_type, _ = _case("mlp_ragged")
    A, Bf, M = compute_kron_factors_last_layer(state, Z, model_type)
    Ac, Bc, Mc = compute_kron_factors_last_layer(state, Z, model_type, example_chunk=4)
    assert M == Mc == 9
    assert (A - Ac).abs().max() <= 1e-12 * A.abs().max() and (Bf - Bc).abs().max() <= 1e-12 * Bf.abs().max()
    assert torch.equal(Ac, Ac.T) and torch.equal(Bc, Bc.T)


# measured on MI355X, max|. - ref| / max|ref| of the posterior variance / predictive covariance / mean, scalar prior
# (two-group prior); the dense covariance, where it differs from its diagonal, in brackets:
#   sine_regressor 2.86e-8 [4.17e-8] / 6.00e-8 / 3.20e-7 (2.92e-8 [3.81e-8] / 3.92e-8 / 3.20e-7)
#   xor_classifier 8.72e-8 / 6.33e-8 / 1.01e-7 (5.58e-8 / 5.31e-8 / 1.01e-7)
#   mlp_ragged     1.27e-7 [1.33e-7] / 4.86e-8 / 2.18e-7 (1.10e-7 [1.18e-7] / 4.84e-8 / 2.18e-7)
#   flat_head      8.83e-8 / 1.00e-7 / 1.72e-7 (7.03e-8 / 7.99e-8 / 1.72e-7)
# (the dense posterior of tests/test_last_layer.py measured 1e-6 .. 6e-6 on the classifiers here: its G carries the
# float32 probabilities' leak into the null directions x (x) 1_K, which the centring of Bf removes)
POSTERIOR_TOL = 5.4e-7
PREDICT_TOL = 4.1e-7
MEAN_TOL = 1.3e-6


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kref.SMALL)
def test_posterior_and_predictive_match_the_float64_helper(name, grouped):
    state, Z, model_type, (off, F, K) = _case(name)
    A_ref, B_ref, M, c, alpha = _helper(name)
    DL = (F + 1) * K
    prior = kref.split_prior(state, alpha) if grouped else alpha
    a_rows = torch.tensor([alpha] + [2.0 * alpha if grouped else alpha] * F, dtype=F64)
    S_ref, _ = kref.covariance_dense(A_ref, B_ref, c, a_rows, model_type)
    post = posterior_lla_last_layer_kron(state, Z, model_type, prior, full_set_size=N_FULL)
    assert isinstance(post, KroneckerNormal)
    theta = flatten_nn_params(state.params)[0]
    assert post.mean().dtype == F64 and torch.equal(post.mean().cpu(), theta[off:off + DL].double())
    e_var = _rel(post.variance(), torch.diagonal(S_ref))
    e_post = _rel(post.covariance(), S_ref)
    Xnew = kref.new_points(Z, 5, 7)
    f_ref, phit, _ = ref.features64(state, Xnew)
    cov_ref = kref.predict_dense(phit, S_ref, K)
    full = predict_lla_last_layer_kron(state, Xnew, Z, model_type, prior, full_set_size=N_FULL, cov="full", batch=3)
    mean, var = predict_lla_last_layer_kron(state, Xnew, Z, model_type, prior, full_set_size=N_FULL, cov="diag", batch=3)
    if model_type == "regressor":
        assert full.mean().shape == (5,) and full.covariance().shape == (5, 5) and mean.shape == var.shape == (5,)
        assert torch.equal(full.covariance(), torch.diag(torch.diagonal(full.covariance())))
        cov = torch.diagonal(full.covariance())[:, None, None]
        var_full = torch.diagonal(full.covariance())
    else:
        assert full.mean().shape == (5, K) and full.covariance().shape == (5, K, K) and mean.shape == var.shape == (5, K)
        cov = full.covariance()
        var_full = torch.diagonal(cov, dim1=1, dim2=2)
    assert torch.equal(var, var_full)                                # cov="diag" is bitwise the diagonal of cov="full"
    assert torch.equal(mean.reshape(-1), full.mean().reshape(-1))
    e_cov = _rel(cov, cov_ref)
    e_mean = _rel(mean.reshape(5, K), f_ref)
    print(f"{name} {'grouped' if grouped else 'scalar'}: variance {e_var:.2e} covariance {e_post:.2e} predictive {e_cov:.2e} "
          f"mean {e_mean:.2e}")
    assert e_var <= POSTERIOR_TOL and e_post <= POSTERIOR_TOL and e_cov <= PREDICT_TOL and e_mean <= MEAN_TOL


def test_regressor_predictive_equals_the_dense_last_layer_posterior():
    """the Gaussian head's Kronecker curvature is the dense last-layer GGN exactly, so the two posteriors agree"""
    state, Z, model_type, _ = _case("sine_regressor")
    _, _, _, _, alpha = _helper("sine_regressor")
    Xnew = kref.new_points(Z, 5, 7)
    mean_k, var_k = predict_lla_last_layer_kron(state, Xnew, Z, model_type, alpha, full_set_size=N_FULL, cov="diag")
    mean_d, var_d = predict_lla_last_layer(state, Xnew, Z, model_type, alpha, full_set_size=N_FULL, cov="diag")
    e = _rel(var_k, var_d)
    print(f"sine_regressor: Kronecker against dense predictive variance {e:.2e}")           # measured on MI355X: 1.63e-15
    assert torch.equal(mean_k, mean_d) and e <= PREDICT_TOL


def test_scalable_draws_are_the_linear_head_applied_to_posterior_draws():
    state, Z, model_type, (off, F, K) = _case("xor_classifier")
    alpha = _helper("xor_classifier")[4]
    Xnew = kref.new_points(Z, 6, 9)
    out = predict_lla_last_layer_kron_scalable(state, Xnew, Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=4)
    assert out.shape == (4, 6, K) and out.is_cuda and out.dtype == F32
    one = predict_lla_last_layer_kron_scalable(state, Xnew, Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=1)
    post = posterior_lla_last_layer_kron(state, Z, model_type, alpha, full_set_size=N_FULL)
    dW = (post.sample((1,), seed=5) - post.mean()).reshape(1, F + 1, K)
    eng = get_engine(state, Xnew, model_type)
    phit = torch.cat([torch.ones(6, 1, device=DEV, dtype=F64), eng.features().double()], dim=1)
    expect = eng.outputs().double()[None] + phit @ dW
    assert one.shape == (1, 6, K)
    # the same draw through the same float64 algebra, rounded once to float32
    assert (one.double() - expect).abs().max() <= 2.0 ** -23 * expect.abs().max()


def test_log_marginal_likelihood_matches_the_helper_spectrum():
    """Measured on MI355X: got -14.0922666232, want -14.0922665908, 2.30e-9 relative (xor_classifier)."""
    state, Z, model_type, (off, F, K) = _case("xor_classifier")
    A_ref, B_ref, M, _, alpha = _helper("xor_classifier")
    DL = (F + 1) * K
    lam = torch.linalg.eigvalsh(A_ref).clamp_min(0.0)
    mu = torch.linalg.eigvalsh(kref.centre(B_ref)).clamp_min(0.0)
    spec = (torch.outer(lam, mu) / M).reshape(-1)                   # N/M = 1
    theta2 = float((flatten_nn_params(state.params)[0][off:off + DL].double() ** 2).sum())
    want = ref.lml_ref(alpha, spec, DL, theta2, N_FULL / M)
    got = log_marginal_likelihood_last_layer_kron(alpha, Z, state, model_type, full_set_size=N_FULL)
    print(f"lml last layer kron: got {got:.12g} want {want:.12g} rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-8 * abs(want)
    post = posterior_lla_last_layer_kron(state, Z, model_type, alpha, full_set_size=N_FULL)
    logdet = float(post.log_det_precision_ratio())
    assert abs((-0.5 * alpha * theta2 - 0.5 * logdet) - want) <= 1e-8 * abs(want)
    a_fit, hist = fit_alpha_last_layer_kron(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=5)
    assert len(hist) == 5 and abs(hist[0][0] - alpha) <= 1e-14 * alpha and abs(hist[0][1] - want) <= 1e-8 * abs(want) and a_fit > 0


def test_eval_dataset_probit_fits_the_posterior_once(monkeypatch):
    state, Z, model_type, _ = _case("xor_classifier")
    alpha = _helper("xor_classifier")[4]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    calls = []
    inner = llk.compute_kron_factors_last_layer
    monkeypatch.setattr(llk, "compute_kron_factors_last_layer", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N_FULL,
                                                               model_type, posterior="last_layer_kron")
    assert len(calls) == 1                                          # one fit for both batches
    assert probs.shape == (16, 2) and labels.shape == (16,)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), (nll, acc, brier, ece_)))
    assert bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1).abs() < 1e-9).all())
    assert llk._FIT_CACHE
    clear_engine_cache()
    assert not llk._FIT_CACHE                                       # clear_engine_cache drops the fitted factors


# measured on MI355X: max|. - ref| / max|ref| of the (5, 100) predictive variances against the helper's factored route
# 5.56e-8, of the mean 2.82e-7
OVERSIZE_TOL = 2.3e-7
OVERSIZE_MEAN_TOL = 1.2e-6


def test_oversize_last_layer_gets_a_posterior():
    """DL = 128 * 100 = 12 800 is above LAST_LAYER_MAX_DIM: the dense functions refuse, the factored posterior answers."""
    net = NetSpec((6,))
    net.dense(net.dense(0, "Dense_0", 127, act="relu"), "Dense_1", 100)
    state = create_state(net, 0, dtype=F64)
    g = torch.Generator().manual_seed(4)
    Z = torch.randn(12, 6, dtype=F64, generator=g)
    Xnew = torch.randn(5, 6, dtype=F64, generator=g)
    off, F, K = last_layer_slice(state, max_dim=None)
    assert (F + 1) * K == 12800 > LAST_LAYER_MAX_DIM
    with pytest.raises(ValueError, match="Kronecker-factored"):
        compute_ggn_last_layer(state, Z, "classifier")
    A, Bf, M = kref.factors_ref(state, Z, "classifier")
    c = kref.c_of(state, M, "classifier", N_FULL)
    alpha = kref.alpha_for(A, Bf, c)
    V, R, Ub, _, _ = kref.factored(A, Bf, c, alpha, "classifier")
    f_ref, phit, _ = ref.features64(state, Xnew)
    var_ref = torch.diagonal(kref.predict_factored(phit, V, R, Ub), dim1=1, dim2=2)
    mean, var = predict_lla_last_layer_kron(state, Xnew, Z, "classifier", alpha, full_set_size=N_FULL, cov="diag")
    assert mean.shape == var.shape == (5, 100) and var.dtype == F64
    assert bool(torch.isfinite(var).all()) and bool((var > 0).all())
    e_var, e_mean = _rel(var, var_ref), _rel(mean, f_ref)
    print(f"oversize: predictive variance {e_var:.2e} mean {e_mean:.2e}")
    assert e_var <= OVERSIZE_TOL and e_mean <= OVERSIZE_MEAN_TOL
    post = posterior_lla_last_layer_kron(state, Z, "classifier", alpha, full_set_size=N_FULL)
    assert post.variance().shape == (12800,)
    with pytest.raises(ValueError, match="LAST_LAYER_MAX_DIM"):
        post.covariance()
