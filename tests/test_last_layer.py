"""GPU checks of the last-layer Laplace posterior: the kernels ``lip_ll_ggn`` / ``lip_ll_predict`` on synthetic operands
through ctypes, then the engine methods and the public surface (``last_layer.py``) on small nets.

Kernel level: the reference is a float64 einsum of the up-cast float32 operands, and the bound is the standard float64
summation bound on the absolute-sum twin A of the reference, with a factor 4 for the reference's own rounding:
|G - ref| <= 4 (n + 8) 2^-53 A for the fit, 4 ((F + 1)^2 + 8) 2^-53 A for the quadratic form.  It holds for any summation
order, so it does not depend on how the kernel splits the work.

Engine level: the features come from the float32 primal pass, so no bound is derivable; every bound there is 4 x the
worst error measured on MI355X (the convention of tests/test_krylov_ops.py and tests/test_wnorm.py), with the measured
figure next to it.
"""
import ctypes
import functools

import pytest
import torch

import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import last_layer as ll
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache, compute_ggn_last_layer, get_engine, materialize_factor
from lip_amd.lla import (posterior_lla_last_layer, predict_lla_dense, predict_lla_last_layer,
                         predict_lla_last_layer_scalable)
from lip_amd.netspec import NetSpec
from lip_amd.prior import GroupedPrior
from lip_amd.scalemodels import LargeClassifier, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from lip_amd.utils import flatten_nn_params
from lip_amd.train_alpha import fit_alpha_last_layer, log_marginal_likelihood_last_layer
from oracle.ggn import compute_ggn_dense

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -53
DEV = "cuda"


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
def _operands(n, F, K, softmax, seed=0, ldphi=None, logit_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ld = ldphi or F
    Phi = torch.randn(n, ld, generator=g, dtype=F32).to(DEV)
    Pr = torch.softmax(logit_scale * torch.randn(n, K, generator=g, dtype=F32), dim=1).to(DEV) if softmax else None
    return Phi, Pr


def _phit(Phi, F):
    return torch.cat([torch.ones(Phi.shape[0], 1, device=Phi.device, dtype=F64), Phi[:, :F].double()], dim=1)


def _ggn_reference(Phi, Pr, F, K):
    """(ref, A): the float64 einsum of the up-cast operands and its absolute-sum twin
    A[(f,k),(g,l)] = sum_i |phit_f phit_g| (delta_kl p_k + p_k p_l)"""
    pt = _phit(Phi, F)
    DL = (F + 1) * K
    if Pr is None:
        H = torch.eye(K, device=Phi.device, dtype=F64).expand(Phi.shape[0], K, K)
        Habs = H
    else:
        p = Pr.double()
        H = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
        Habs = torch.diag_embed(p) + p[:, :, None] * p[:, None, :]
    G = torch.einsum("if,ig,ikl->fkgl", pt, pt, H).reshape(DL, DL)
    A = torch.einsum("if,ig,ikl->fkgl", pt.abs(), pt.abs(), Habs).reshape(DL, DL)
    return G, A


def _scratch(n, F, K):
    lib = nv.load()
    d = ctypes.c_int64(0)
    nv.check(lib.lip_ll_ggn_scratch(n, F, K, ctypes.byref(d)), "lip_ll_ggn_scratch")
    return torch.empty(max(1, d.value), device=DEV, dtype=F64)


def _run_ggn(Phi, Pr, F, K, G=None, n=None, row0=0):
    lib = nv.load()
    n = Phi.shape[0] - row0 if n is None else n
    DL = (F + 1) * K
    if G is None:
        G = torch.zeros(DL, DL, device=DEV, dtype=F64)
    scratch = _scratch(n, F, K)
    phi = Phi[row0:]
    pr = None if Pr is None else Pr[row0:]
    nv.check(lib.lip_ll_ggn(phi.data_ptr(), Phi.stride(0), 0 if pr is None else pr.data_ptr(), n, F, K, G.data_ptr(),
                            scratch.data_ptr(), scratch.numel(), nv.stream_ptr()), "lip_ll_ggn")
    torch.cuda.synchronize()
    return G


# (n, F, K, softmax, ldphi)
GGN_SHAPES = [
    (1, 1, 1, False, None),            # smallest case, Gaussian head
    (9, 5, 3, True, None),             # DL = 18
    (33, 24, 5, True, 27),             # DL = 125, no tile multiple; ldphi = F + 3
    (50, 72, 10, True, None),          # DL = 730
    (257, 7, 33, True, None),          # K above any 16 / 32 tile
    (4099, 63, 10, True, None),        # DL = 640, many row blocks
    (4099, 63, 1, False, None),        # many row blocks, Gaussian head
    (1, 4, 33, True, None),            # n = 0-adjacent guard: one example, K = 33
]


@pytest.mark.parametrize("n,F,K,softmax,ldphi", GGN_SHAPES)
def test_ll_ggn_against_float64_einsum(n, F, K, softmax, ldphi):
    Phi, Pr = _operands(n, F, K, softmax, seed=n + F + K, ldphi=ldphi)
    G_ref, A = _ggn_reference(Phi, Pr, F, K)
    bound = 4 * (n + 8) * U * A
    G = _run_ggn(Phi, Pr, F, K)
    err = (G - G_ref).abs()
    print(f"ll_ggn n={n} F={F} K={K}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(G, G.T)                                     # exactly symmetric
    assert torch.equal(G, _run_ggn(Phi, Pr, F, K))                 # bitwise reproducible
    # a pre-filled G is added to, not overwritten
    g = torch.Generator().manual_seed(1)
    G0 = torch.randn(G.shape, generator=g, dtype=F64).to(DEV)
    G1 = _run_ggn(Phi, Pr, F, K, G=G0.clone())
    assert bool(((G1 - G0 - G_ref).abs() <= bound + 4 * U * (G0.abs() + G_ref.abs())).all())
    # two calls on the two halves of the examples, added into one G, equal one call on all examples within the bound
    if n >= 2:
        h = n // 2
        Gh = _run_ggn(Phi, Pr, F, K, n=h)
        Gh = _run_ggn(Phi, Pr, F, K, G=Gh, n=n - h, row0=h)
        assert bool(((Gh - G_ref).abs() <= bound).all())
        assert torch.equal(Gh, Gh.T)


def test_ll_ggn_float32_softmax_of_scaled_logits():
    """the plain float32 softmax of logits x 50 (rows may sum to 1 + 6e-8) under the elementwise bound"""
    n, F, K = 33, 24, 5
    Phi, Pr = _operands(n, F, K, True, seed=11, logit_scale=50.0)
    assert float(Pr.max()) > 0.999
    G_ref, A = _ggn_reference(Phi, Pr, F, K)
    G = _run_ggn(Phi, Pr, F, K)
    assert bool(((G - G_ref).abs() <= 4 * (n + 8) * U * A).all())
    assert torch.equal(G, G.T)


def test_ll_ggn_near_one_hot_probabilities_stay_psd():
    """logits x 50: the probabilities are one-hot to rounding and diag(p) - p p^T cancels almost completely.
    diag(p) - p p^T is positive semi-definite exactly when sum_k p_k <= 1, and a float32 softmax row can sum to
    1 + 6e-8, which alone puts lambda_min at -4e-8 lambda_max in exact arithmetic.  The rows here are a float64 softmax
    scaled by 1 - 2^-22 before rounding to float32, so every row sums to less than 1 and whatever negative eigenvalue
    appears is the kernel's rounding."""
    n, F, K = 33, 24, 5
    g = torch.Generator().manual_seed(11)
    Phi = torch.randn(n, F, generator=g, dtype=F32).to(DEV)
    p64 = torch.softmax(50.0 * torch.randn(n, K, generator=g, dtype=F64), dim=1)
    Pr = (p64 * (1.0 - 2.0 ** -22)).float()
    assert float(Pr.double().sum(1).max()) < 1.0 and float(Pr.max()) > 0.999
    Pr = Pr.to(DEV)
    G_ref, A = _ggn_reference(Phi, Pr, F, K)
    G = _run_ggn(Phi, Pr, F, K)
    assert bool(((G - G_ref).abs() <= 4 * (n + 8) * U * A).all())
    lam = torch.linalg.eigvalsh(G)
    print(f"near-one-hot: lambda_min / lambda_max = {(lam.min() / lam.max()).item():.2e}")
    assert lam.min() >= -1e-12 * lam.max()


def test_ll_ggn_status_codes_leave_g_untouched():
    lib = nv.load()
    n, F, K = 9, 5, 3
    Phi, Pr = _operands(n, F, K, True)
    DL = (F + 1) * K
    G0 = torch.full((DL, DL), 7.0, device=DEV, dtype=F64)
    G = G0.clone()
    scratch = _scratch(n, F, K)
    st = nv.stream_ptr()
    good = [Phi.data_ptr(), F, Pr.data_ptr(), n, F, K, G.data_ptr(), scratch.data_ptr(), scratch.numel(), st]

    def call(**kw):
        args = list(good)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return lib.lip_ll_ggn(*args)

    bad = [dict(a0=0), dict(a6=0), dict(a7=0), dict(a1=F - 1), dict(a8=scratch.numel() - 1 if scratch.numel() > 1 else 0),
           dict(a3=0), dict(a4=0), dict(a5=0)]
    for kw in bad:
        assert call(**kw) == 1, kw                                  # LIP_ERR_ARG
        assert lib.lip_last_error()
        torch.cuda.synchronize()
        assert torch.equal(G, G0), kw
    d = ctypes.c_int64(0)
    assert lib.lip_ll_ggn_scratch(0, F, K, ctypes.byref(d)) == 1
    assert lib.lip_ll_ggn_scratch(n, F, K, None) == 1
    assert call() == 0


def _run_predict(Phi, F, K, S, diag):
    lib = nv.load()
    B = Phi.shape[0]
    out = torch.full((B, K) if diag else (B, K, K), float("nan"), device=DEV, dtype=F64)
    nv.check(lib.lip_ll_predict(Phi.data_ptr(), Phi.stride(0), B, F, K, S.data_ptr(), out.data_ptr(), int(diag),
                                nv.stream_ptr()), "lip_ll_predict")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 9, 257])
@pytest.mark.parametrize("F,K,ldphi", [(1, 1, None), (5, 3, None), (24, 5, 27), (72, 10, None), (7, 33, None), (63, 10, None),
                                       (63, 1, None)])
def test_ll_predict_against_float64_einsum(B, F, K, ldphi):
    Phi, _ = _operands(B, F, K, False, seed=B + F + K, ldphi=ldphi)
    DL = (F + 1) * K
    g = torch.Generator().manual_seed(5)
    R = torch.randn(DL, DL, generator=g, dtype=F64)
    S = (R @ R.T / DL + torch.eye(DL, dtype=F64)).to(DEV)           # random SPD
    pt = _phit(Phi, F)
    S4 = S.reshape(F + 1, K, F + 1, K)
    cov_ref = torch.einsum("bf,bg,fkgl->bkl", pt, pt, S4)
    bound = 4 * ((F + 1) ** 2 + 8) * U * torch.einsum("bf,bg,fkgl->bkl", pt.abs(), pt.abs(), S4.abs())
    full = _run_predict(Phi, F, K, S, diag=False)
    dg = _run_predict(Phi, F, K, S, diag=True)
    assert bool(((full - cov_ref).abs() <= bound).all())
    assert torch.equal(full, full.transpose(1, 2))                  # exactly symmetric in (k, l)
    # the diag form runs the l = k column of the full form through the same code: bitwise its diagonal
    assert torch.equal(dg, torch.diagonal(full, dim1=1, dim2=2))


def test_ll_predict_status_codes_leave_out_untouched():
    lib = nv.load()
    B, F, K = 9, 5, 3
    Phi, _ = _operands(B, F, K, False)
    DL = (F + 1) * K
    S = torch.eye(DL, device=DEV, dtype=F64)
    out0 = torch.full((B, K, K), 7.0, device=DEV, dtype=F64)
    out = out0.clone()
    st = nv.stream_ptr()
    good = [Phi.data_ptr(), F, B, F, K, S.data_ptr(), out.data_ptr(), 0, st]
    for i, v in [(0, 0), (5, 0), (6, 0), (1, F - 1), (2, 0), (3, 0), (4, 0)]:
        args = list(good)
        args[i] = v
        assert lib.lip_ll_predict(*args) == 1, (i, v)               # LIP_ERR_ARG
        assert lib.lip_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, out0), (i, v)
    assert lib.lip_ll_predict(*good) == 0


# ------------------------------------------------------------------------------------------------ engine level
def _flat_head_net():
    """a final Dense directly on a 3 x 3 x 4 feature map (the ``flat_kernel`` path)"""
    net = NetSpec((3, 3, 2))
    c = net.conv(0, "Conv_0", 4, 3, act="relu", use_bias=True)
    net.dense(c, "Dense_0", 3)
    return net


def _cases():
    """the nets of tests/test_wnorm.py::_cases that are small enough for the oracle's dense GGN, and the flat-head net"""
    g = torch.Generator().manual_seed(0)
    return {
        "sine_regressor": (SimpleRegressor(8, 4), torch.randn(16, 1, dtype=F64, generator=g), "regressor"),
        "xor_classifier": (SimpleClassifier(16, 2, 2), torch.randn(32, 2, dtype=F64, generator=g), "classifier"),
        "mlp_ragged": (LargeClassifier((6, 6, 1), [40, 24], 2, 5), torch.rand(9, 6, 6, 1, dtype=F64, generator=g),
                       "classifier"),
        "resnet_tiny": (ResNet1M(4, input_shape=(8, 8, 3), widths=(4, 8, 12), blocks_per_stage=2),
                        torch.rand(3, 8, 8, 3, dtype=F64, generator=g), "classifier"),
        "resnet50_tiny": (ResNet50(6, input_shape=(20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
                          torch.rand(2, 20, 20, 3, dtype=F64, generator=g), "classifier"),
        "flat_head": (_flat_head_net(), torch.rand(7, 3, 3, 2, dtype=F64, generator=g), "classifier"),
    }


NETS = list(_cases())
SMALL = ["sine_regressor", "xor_classifier", "mlp_ragged", "flat_head"]
N_FULL = 40


@functools.lru_cache(maxsize=None)
def _case(name):
    """(state, Z, model_type, (offset, F, K)); built once per net and never written to"""
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    return state, Z, model_type, ll.last_layer_slice(state)


@functools.lru_cache(maxsize=None)
def _oracle_slice(name):
    """the oracle's dense GGN restricted to theta_L (float64, CPU), full_set_size = N_FULL"""
    state, Z, model_type, (off, F, K) = _case(name)
    sl = slice(off, off + (F + 1) * K)
    return compute_ggn_dense(state, Z, model_type, full_set_size=N_FULL)[0][sl, sl].contiguous()


@functools.lru_cache(maxsize=None)
def _helper(name):
    """(G_ref, alpha) of the float64 helper at full_set_size = N_FULL, alpha = 1e-3 lambda_max(G_ref)"""
    state, Z, model_type, _ = _case(name)
    G = ref.ggn_last_layer_ref(state, Z, model_type, full_set_size=N_FULL)
    lam = torch.linalg.eigvalsh(G)
    alpha = 1e-3 * float(lam.max())
    assert (float(lam.max()) + alpha) / (max(float(lam.min()), 0.0) + alpha) <= 1001.0 * (1 + 1e-12)
    return G, alpha


def _new_points(Z, B, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B,) + tuple(Z.shape[1:])
    return torch.randn(shape, dtype=F64, generator=g) if Z.dim() == 2 else torch.rand(shape, dtype=F64, generator=g)


def _rel(v, r):
    r = r.to(v.device)
    return ((v.double() - r).abs().max() / r.abs().max()).item()


# measured on MI355X, max|features - ref| / max|ref| and max|G - ref| / max|ref| against the oracle's dense GGN slice:
#   sine_regressor 1.75e-7 / 3.25e-8, xor_classifier 1.25e-7 / 2.56e-8, mlp_ragged 2.07e-7 / 3.79e-8,
#   resnet_tiny 7.28e-8 / 4.44e-8, resnet50_tiny 1.24e-7 / 1.97e-7, flat_head 7.18e-8 / 1.83e-8
FEATURE_TOL = 8.3e-7
GGN_TOL = 7.9e-7


@pytest.mark.parametrize("name", NETS)
def test_features_and_ggn_match_the_oracle_slice(name):
    state, Z, model_type, (off, F, K) = _case(name)
    eng = get_engine(state, Z, model_type)
    assert eng.last_layer() == (off, F, K)
    _, phit, _ = ref.features64(state, Z)
    phi = eng.features()
    assert phi.shape == (Z.shape[0], F) and phi.dtype == F32 and phi.is_cuda
    e_phi = _rel(phi, phit[:, 1:])
    G = compute_ggn_last_layer(state, Z, model_type, full_set_size=N_FULL)
    torch.cuda.synchronize()
    DL = (F + 1) * K
    assert G.shape == (DL, DL) and G.dtype == F64 and G.is_cuda
    e_g = _rel(G, _oracle_slice(name))
    print(f"{name}: DL={DL} features {e_phi:.2e}  G {e_g:.2e}")
    assert torch.equal(G, G.T)
    assert e_phi <= FEATURE_TOL and e_g <= GGN_TOL


def test_example_chunks_add_into_one_g():
    """n = 9 in chunks of 4 (a ragged last chunk): the same float64 operands in another grouping"""
    state, Z, model_type, _ = _case("mlp_ragged")
    G = compute_ggn_last_layer(state, Z, model_type, full_set_size=N_FULL)
    Gc = compute_ggn_last_layer(state, Z, model_type, full_set_size=N_FULL, example_chunk=4)
    assert (G - Gc).abs().max() <= 1e-12 * G.abs().max()
    assert torch.equal(Gc, Gc.T)


# measured on MI355X: max|G - Wl^T Wl| / max = 3.84e-8
FACTOR_TOL = 1.6e-7


def test_ggn_matches_the_materialised_factor_route():
    state, Z, model_type, (off, F, K) = _case("resnet_tiny")
    eng = get_engine(state, Z, model_type)
    Wl = materialize_factor(eng)[:, off:off + (F + 1) * K].double()
    G = compute_ggn_last_layer(state, Z, model_type)
    e = _rel(G, Wl.T @ Wl)
    print(f"resnet_tiny: last-layer G against the factor route {e:.2e}")
    assert e <= FACTOR_TOL


def test_oversize_last_layer_is_refused_before_allocation():
    net = NetSpec((6,))
    net.dense(net.dense(0, "Dense_0", 100, act="relu"), "Dense_1", 100)
    state = create_state(net, 0, dtype=F64)
    with pytest.raises(ValueError, match="Kronecker-factored"):
        compute_ggn_last_layer(state, torch.randn(4, 6, dtype=F64), "classifier")


def _split_prior(state, alpha):
    """two groups cutting theta_L between the final bias and the final kernel"""
    kernel = state.net.units[-1].kernel
    return GroupedPrior(state.params, [alpha, 2.0 * alpha], lambda path: "head_kernel" if path == kernel else "rest")


# measured on MI355X, max|. - ref| / max|ref| of the posterior covariance / predictive covariance / mean, scalar prior
# (two-group prior):
#   sine_regressor 4.17e-8 / 6.00e-8 / 3.20e-7 (3.81e-8 / 3.92e-8 / 3.20e-7)
#   xor_classifier 8.62e-7 / 5.68e-6 / 1.01e-7 (9.62e-7 / 3.67e-6 / 1.01e-7)
#   mlp_ragged     7.02e-7 / 4.63e-6 / 2.18e-7 (1.31e-6 / 3.30e-6 / 2.18e-7)
#   flat_head      1.07e-6 / 5.73e-6 / 1.72e-7 (1.96e-6 / 4.24e-6 / 1.72e-7)
POSTERIOR_TOL = 7.9e-6
PREDICT_TOL = 2.3e-5
MEAN_TOL = 1.3e-6


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", SMALL)
def test_posterior_and_predictive_match_the_float64_helper(name, grouped):
    state, Z, model_type, (off, F, K) = _case(name)
    G_ref, alpha = _helper(name)
    DL = (F + 1) * K
    if grouped:
        prior = _split_prior(state, alpha)
        a = prior.vector("cpu", F64)[off:off + DL]
        assert float(a[K - 1]) == alpha and float(a[K]) == 2.0 * alpha          # the cut lies between bias and kernel
        lam = torch.linalg.eigvalsh(G_ref + torch.diag(a))
        assert float(lam.max() / lam.min()) <= 1002.0
    else:
        prior, a = alpha, alpha
    S_ref = ref.covariance_ref(G_ref, a)
    post = posterior_lla_last_layer(state, Z, model_type, prior, full_set_size=N_FULL)
    theta = flatten_nn_params(state.params)[0]
    assert post.mean().dtype == F64 and torch.equal(post.mean().cpu(), theta[off:off + DL].double())
    e_post = _rel(post.covariance(), S_ref)
    Xnew = _new_points(Z, 5, 7)
    f_ref, cov_ref = ref.predict_ref(state, Xnew, S_ref)
    full = predict_lla_last_layer(state, Xnew, Z, model_type, prior, full_set_size=N_FULL, cov="full", batch=3)
    mean, var = predict_lla_last_layer(state, Xnew, Z, model_type, prior, full_set_size=N_FULL, cov="diag", batch=3)
    if model_type == "regressor":
        dense = predict_lla_dense(state, Xnew, Z, model_type, alpha, full_set_size=N_FULL)
        assert full.mean().shape == dense.mean().shape == (5,)
        assert full.covariance().shape == dense.covariance().shape == (5, 5)
        assert mean.shape == var.shape == (5,)
        cov = torch.diagonal(full.covariance())[:, None, None]
        assert torch.equal(full.covariance(), torch.diag(torch.diagonal(full.covariance())))
        var_full = torch.diagonal(full.covariance())
    else:
        assert full.mean().shape == (5, K) and full.covariance().shape == (5, K, K)
        assert mean.shape == var.shape == (5, K)
        cov = full.covariance()
        var_full = torch.diagonal(cov, dim1=1, dim2=2)
    assert torch.equal(var, var_full)                                # cov="diag" is the diagonal of cov="full"
    assert torch.equal(mean.reshape(-1), full.mean().reshape(-1))
    e_cov = _rel(cov, cov_ref)
    e_mean = _rel(mean.reshape(5, K), f_ref)
    print(f"{name} {'grouped' if grouped else 'scalar'}: posterior {e_post:.2e} predictive {e_cov:.2e} mean {e_mean:.2e}")
    assert e_post <= POSTERIOR_TOL and e_cov <= PREDICT_TOL and e_mean <= MEAN_TOL


def test_scalable_draws_are_the_linear_head_applied_to_posterior_draws():
    state, Z, model_type, (off, F, K) = _case("xor_classifier")
    _, alpha = _helper("xor_classifier")
    Xnew = _new_points(Z, 6, 9)
    out = predict_lla_last_layer_scalable(state, Xnew, Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=4)
    assert out.shape == (4, 6, K) and out.is_cuda
    one = predict_lla_last_layer_scalable(state, Xnew, Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=1)
    post = posterior_lla_last_layer(state, Z, model_type, alpha, full_set_size=N_FULL)
    dW = (post.sample((1,), seed=5) - post.mean()).reshape(1, F + 1, K)
    eng = get_engine(state, Xnew, model_type)
    phit = torch.cat([torch.ones(6, 1, device=DEV, dtype=F64), eng.features().double()], dim=1)
    expect = eng.outputs().double()[None] + phit @ dW
    assert one.shape == (1, 6, K)
    # the same draw through the same float64 algebra, rounded once to float32
    assert (one.double() - expect).abs().max() <= 2.0 ** -23 * expect.abs().max()


def test_log_marginal_likelihood_matches_the_helper_spectrum():
    """Measured on MI355X: got -13.9722631425, want -13.9722630835, 4.22e-9 relative (xor_classifier, alpha = 1e-3
    lambda_max).  Without the projection of G onto the complement of the directions x (x) 1_K in
    ``last_layer._spectrum_last_layer`` the same case gave 1.08e-7: float32 probabilities sum to 1 +- 6e-8, which lifts
    the exactly-zero eigenvalues of the classifier's G, and log1p(r lambda / alpha) magnifies them by lambda_max / alpha
    = 1000."""
    state, Z, model_type, (off, F, K) = _case("xor_classifier")
    _, alpha = _helper("xor_classifier")
    DL = (F + 1) * K
    G1 = ref.ggn_last_layer_ref(state, Z, model_type)               # N/M = 1
    lam = torch.linalg.eigvalsh(G1).clamp_min(0.0)
    theta2 = float((flatten_nn_params(state.params)[0][off:off + DL].double() ** 2).sum())
    want = ref.lml_ref(alpha, lam, DL, theta2, N_FULL / Z.shape[0])
    got = log_marginal_likelihood_last_layer(alpha, Z, state, model_type, full_set_size=N_FULL)
    print(f"lml last layer: got {got:.12g} want {want:.12g} rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-8 * abs(want)
    a_fit, hist = fit_alpha_last_layer(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=5)
    assert len(hist) == 5 and abs(hist[0][0] - alpha) <= 1e-14 * alpha and abs(hist[0][1] - want) <= 1e-8 * abs(want) and a_fit > 0


def test_eval_dataset_probit_fits_the_posterior_once(monkeypatch):
    state, Z, model_type, _ = _case("xor_classifier")
    _, alpha = _helper("xor_classifier")
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    calls = []
    inner = ll.compute_ggn_last_layer
    monkeypatch.setattr(ll, "compute_ggn_last_layer", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N_FULL,
                                                               model_type, posterior="last_layer")
    assert len(calls) == 1                                          # one fit for both batches
    assert probs.shape == (16, 2) and labels.shape == (16,)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), (nll, acc, brier, ece_)))
    assert bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1).abs() < 1e-9).all())
    clear_engine_cache()
    assert not ll._COV_CACHE                                        # clear_engine_cache drops the fitted covariance
