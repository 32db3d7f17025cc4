"""GPU checks of the Kronecker-factored posterior over all layers: the kernels ``lip_kfac_input_gram`` /
``lip_kfac_predict`` on synthetic operands through ctypes, then the engine methods and the public surface (``kfac.py``)
on the small nets of tests/last_layer_kron_ref.py and a net on a non-square map.

Kernel level: the reference is a float64 einsum of the up-cast float32 operands, and the bound is the standard float64
summation bound on the absolute-value twin of the reference, with a factor 4 for the reference's own rounding (the
convention of tests/test_last_layer.py): 4 (terms + 8) 2^-53, terms = n OH OW for the input Gram and
2 (Mt + N) + Mt N for the predictive.  Both hold for any summation order.

Engine level: the activations and cotangents come from the float32 passes, so no bound is derivable; every bound there
is 4 x the worst error measured on MI355X against the float64 helper (``tests/kfac_ref.py``), with the measured figure
next to it.
"""
import ctypes
import functools
import types

import pytest
import torch

import kfac_ref as kf
import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import kfac
from lip_amd.distributions import KFACNormal, MultivariateNormalFullCovariance
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache, compute_kfac_factors, compute_kron_factors_last_layer, get_engine
from lip_amd.lla import posterior_lla_kfac, predict_lla_kfac, predict_lla_kfac_scalable
from lip_amd.train_alpha import fit_alpha_kfac, log_marginal_likelihood_kfac
from lip_amd.utils import flatten_nn_params

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -53
DEV = "cuda"
N_FULL = kf.N_FULL


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
# (n, IH, IW, C, KH, KW, stride, pad_h, pad_w, OH, OW, bias)
GRAM_GEOMETRIES = {
    "1x1_c1": (1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0),                  # smallest
    "1x1_c1_bias": (1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1),
    "3x3_5x4x3": (2, 5, 4, 3, 3, 3, 1, 1, 1, 5, 4, 1),               # Mt = 28, non-square, all four borders masked
    "3x3s2_same_7x6x4": (3, 7, 6, 4, 3, 3, 2, 1, 0, 4, 3, 1),        # high-side padding, Mt = 37 crosses a tile
    "1x1s2_6x6x33": (2, 6, 6, 33, 1, 1, 2, 0, 0, 3, 3, 0),
    "valid_3x3x4": (4, 3, 3, 4, 3, 3, 1, 0, 0, 1, 1, 1),             # flat head, one position
    "3x3_8x8x16": (2, 8, 8, 16, 3, 3, 1, 1, 1, 8, 8, 1),             # Mt = 145, five tiles per edge
    "3x3_32x32x4_n5": (5, 32, 32, 4, 3, 3, 1, 1, 1, 32, 32, 0),      # 5120 rows, many row ranges
}


def _run_gram(X, geom, A=None, n=None, img0=0):
    lib = nv.load()
    n = geom[0] - img0 if n is None else n
    g = (n,) + tuple(geom[1:])
    Mt = geom[3] * geom[4] * geom[5] + geom[11]
    A = torch.zeros(Mt, Mt, device=DEV, dtype=F64) if A is None else A
    d = ctypes.c_int64(0)
    nv.check(lib.lip_kfac_input_gram_scratch(*g, ctypes.byref(d)), "lip_kfac_input_gram_scratch")
    scratch = torch.empty(max(1, d.value), device=DEV, dtype=F64)
    nv.check(lib.lip_kfac_input_gram(X[img0:].data_ptr(), *g, A.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                     nv.stream_ptr()), "lip_kfac_input_gram")
    torch.cuda.synchronize()
    return A


@pytest.mark.parametrize("name", list(GRAM_GEOMETRIES))
def test_input_gram_against_float64_einsum(name):
    geom = GRAM_GEOMETRIES[name]
    n, IH, IW, Cc, KH, KW, stride, ph, pw, OH, OW, bias = geom
    g = torch.Generator().manual_seed(sum(geom))
    X = torch.randn(n, IH, IW, Cc, generator=g, dtype=F32)
    unit = types.SimpleNamespace(kh=KH, kw=KW, stride=stride, pad_h=ph, pad_w=pw)
    P = kf.patches(X.double(), unit, OH, OW, bool(bias)).reshape(n * OH * OW, -1)
    A_ref, A_abs = (P.T @ P).to(DEV), (P.abs().T @ P.abs()).to(DEV)
    bound = 4 * (n * OH * OW + 8) * U * A_abs
    Xd = X.to(DEV)
    A = _run_gram(Xd, geom)
    err = (A - A_ref).abs()
    print(f"input gram {name}: Mt={A.shape[0]} max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(A, A.T)                                                 # exactly symmetric
    assert torch.equal(A, _run_gram(Xd, geom))                                 # bitwise reproducible
    if n >= 2:                                                                 # two halves of the images add into one A
        h = n // 2
        Ah = _run_gram(Xd, geom, n=h)
        Ah = _run_gram(Xd, geom, A=Ah, n=n - h, img0=h)
        assert bool(((Ah - A_ref).abs() <= bound).all()) and torch.equal(Ah, Ah.T)


def test_input_gram_status_codes_leave_the_factor_untouched():
    lib = nv.load()
    geom = GRAM_GEOMETRIES["3x3_5x4x3"]
    X = torch.randn(geom[0], 5, 4, 3, dtype=F32).to(DEV)
    A0 = torch.full((28, 28), 7.0, device=DEV, dtype=F64)
    A = A0.clone()
    scratch = torch.empty(1 << 16, device=DEV, dtype=F64)
    good = [X.data_ptr(), *geom, A.data_ptr(), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()]
    for i, v in [(0, 0), (13, 0), (14, 0), (1, 0), (4, 0), (7, 0), (15, 1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_input_gram(*args) == 1, (i, v)
    # 2^31 or more elements are refused before any launch (nothing of that size exists)
    big = [X.data_ptr(), 1 << 20, 64, 64, 1, 1, 1, 1, 0, 0, 64, 64, 0, A.data_ptr(), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()]
    assert lib.lip_kfac_input_gram(*big) == 1 and b"2^31" in lib.lip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(A, A0)


PREDICT_BLOCKS = [(1, 1), (9, 3), (37, 5), (33, 33), (145, 16)]


def _run_predict(Jr, ldj, B, Kc, off, Mt, N, V, Ub, R, diag, scratch_doubles=None):
    lib = nv.load()
    d = ctypes.c_int64(0)
    nv.check(lib.lip_kfac_predict_scratch(B, Kc, Mt, N, ctypes.byref(d)), "lip_kfac_predict_scratch")
    assert d.value == 2 * B * Kc * Mt * N
    scratch = torch.empty(d.value if scratch_doubles is None else scratch_doubles, device=DEV, dtype=F64)
    out = torch.zeros((B, Kc) if diag else (B, Kc, Kc), device=DEV, dtype=F64)
    nv.check(lib.lip_kfac_predict(Jr.data_ptr(), ldj, B, Kc, off, Mt, N, V.data_ptr(), Ub.data_ptr(), R.data_ptr(),
                                  out.data_ptr(), int(diag), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_kfac_predict")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Mt,N", PREDICT_BLOCKS)
def test_predict_against_float64_einsum(Mt, N):
    g = torch.Generator().manual_seed(Mt * 100 + N)
    off = 5
    ldj = off + Mt * N + 3
    V = torch.randn(Mt, Mt, generator=g, dtype=F64).to(DEV)
    Ub = torch.randn(N, N, generator=g, dtype=F64).to(DEV)
    R = torch.rand(Mt, N, generator=g, dtype=F64).to(DEV)
    for B, Kc in [(1, 1), (1, 3), (5, 1), (5, 3)]:
        Jr = torch.randn(Kc * B, ldj, generator=g, dtype=F32).to(DEV)
        J = Jr[:, off:off + Mt * N].double().reshape(Kc, B, Mt, N)
        T = V.T @ J @ Ub
        want = torch.einsum("jl,kbjl,mbjl->bkm", R, T, T)
        Ta = V.abs().T @ J.abs() @ Ub.abs()
        bound = 4 * (2 * (Mt + N) + Mt * N + 8) * U * torch.einsum("jl,kbjl,mbjl->bkm", R, Ta, Ta)
        full = _run_predict(Jr, ldj, B, Kc, off, Mt, N, V, Ub, R, False)
        dg = _run_predict(Jr, ldj, B, Kc, off, Mt, N, V, Ub, R, True)
        err = (full - want).abs()
        print(f"predict Mt={Mt} N={N} B={B} Kc={Kc}: max err / bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all())
        assert torch.equal(full, full.transpose(1, 2))                        # exactly symmetric
        assert torch.equal(dg, torch.diagonal(full, dim1=1, dim2=2))          # diag is bitwise the diagonal of full
        if B > 1:                                                             # a scratch for two points: three chunks
            small = _run_predict(Jr, ldj, B, Kc, off, Mt, N, V, Ub, R, False, scratch_doubles=2 * 2 * Kc * Mt * N)
            assert torch.equal(small, full)


def test_predict_status_codes_leave_the_output_untouched():
    lib = nv.load()
    B, Kc, off, Mt, N = 2, 3, 4, 9, 3
    ldj = off + Mt * N
    Jr = torch.randn(Kc * B, ldj, dtype=F32).to(DEV)
    V, Ub, R = (torch.randn(s, dtype=F64).to(DEV) for s in ((Mt, Mt), (N, N), (Mt, N)))
    out0 = torch.full((B, Kc, Kc), 3.0, device=DEV, dtype=F64)
    out = out0.clone()
    scratch = torch.empty(2 * B * Kc * Mt * N, device=DEV, dtype=F64)
    good = [Jr.data_ptr(), ldj, B, Kc, off, Mt, N, V.data_ptr(), Ub.data_ptr(), R.data_ptr(), out.data_ptr(), 0,
            scratch.data_ptr(), scratch.numel(), nv.stream_ptr()]
    for i, v in [(0, 0), (7, 0), (8, 0), (9, 0), (10, 0), (12, 0), (1, ldj - 1), (2, 0), (3, 0), (5, 0), (6, 0), (4, -1),
                 (13, 2 * Kc * Mt * N - 1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_predict(*args) == 1, (i, v)
    torch.cuda.synchronize()
    assert torch.equal(out, out0)


# ------------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _helper(name):
    """everything of the float64 helper, built once per net and never written to"""
    state, Z, model_type = kf.make_case(name)
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    Xnew = kref.new_points(Z, 5, 7)
    f_new, J_new = ref.jac64(state, Xnew, model_type)
    return dict(state=state, Z=Z, model_type=model_type, As=As, Ss=Ss, M=M, alpha=alpha, Xnew=Xnew, f_new=f_new, J_new=J_new,
                diag=kf.ggn_diag_ref(state, Z, model_type, N_FULL), rem=kf.remainder_of(state))


def _rel(v, r):
    r = r.to(v.device)
    return ((v.double() - r).abs().max() / r.abs().max()).item()


# measured on MI355X, worst over the blocks of a net of max|A_l - ref| / max|ref| and max|S_l - ref| / max|ref| against
# the float64 helper, and [the final block's S against lip_ll_kron_factors' Bf; its A agrees bitwise]:
#   sine_regressor 5.80e-8 / 2.67e-7 [0]        xor_classifier 2.47e-8 / 4.79e-8 [1.27e-8]
#   mlp_ragged     4.06e-8 / 3.46e-8 [2.83e-8]  resnet_tiny    2.05e-7 / 2.10e-7 [3.84e-8]
#   resnet50_tiny  3.88e-7 / 2.50e-7 [4.36e-8]  flat_head      1.77e-8 / 4.44e-8 [4.02e-8]
#   stem_net       1.21e-7 / 2.06e-7
FACTOR_A_TOL = 1.6e-6          # 4 x 3.88e-7
FACTOR_S_TOL = 1.1e-6          # 4 x 2.67e-7
FINAL_S_TOL = 1.8e-7           # 4 x 4.36e-8


@pytest.mark.parametrize("name", kf.NETS)
def test_factors_match_the_float64_helper(name):
    h = _helper(name)
    blocks, As, Ss, M = compute_kfac_factors(h["state"], h["Z"], h["model_type"])
    assert M == h["M"] and len(blocks) == len(As) == len(Ss) == len(h["As"])
    e_a = max(_rel(A, Ar) for A, Ar in zip(As, h["As"]))
    e_s = max(_rel(S, Sr) for S, Sr in zip(Ss, h["Ss"]))
    print(f"{name}: A {e_a:.2e}  S {e_s:.2e}")
    for b, A, S in zip(blocks, As, Ss):
        assert A.dtype == S.dtype == F64 and A.shape == (b.Mt, b.Mt) and S.shape == (b.N, b.N)
        assert torch.equal(A, A.T) and torch.equal(S, S.T)
    assert e_a <= FACTOR_A_TOL and e_s <= FACTOR_S_TOL
    if name in kref.NETS:                                          # the final Dense block reproduces last_layer_kron.py
        A, Bf, _ = compute_kron_factors_last_layer(h["state"], h["Z"], h["model_type"])
        e_fa, e_fb = _rel(As[-1], A), _rel(Ss[-1], Bf)
        print(f"{name}: final block against lip_ll_kron_factors  A {e_fa:.2e}  S {e_fb:.2e}")
        assert e_fa <= 1e-13 and e_fb <= FINAL_S_TOL                # A: the same float64 Gram in another order (measured: 0)


# The float32 patches and cotangent rows of an example do not depend on how the examples and classes are chunked, so a
# chunked fit is the same float64 products in another grouping: at most (n T K + 8) 2^-53 < 1e-12 of the absolute-value
# sums (the bound tests/test_last_layer_kron.py asks of its example chunks).  Measured on MI355X, worst block, A / S:
# sine_regressor 2.22e-16 / 1.13e-16, xor_classifier 0 / 1.18e-16, mlp_ragged 4.93e-17 / 2.61e-16, resnet_tiny
# 7.11e-17 / 2.08e-16, resnet50_tiny 1.99e-16 / 2.86e-16, flat_head 5.64e-17 / 1.44e-16, stem_net 2.58e-16 / 2.25e-16
SPLIT_TOL = 1e-12


@pytest.mark.parametrize("name", kf.NETS)
def test_example_and_class_chunks_agree_with_the_unsplit_fit(name):
    """examples in two chunks or more (a ragged last one where M is odd), classes in chunks of about K / 2"""
    h = _helper(name)
    M, K = h["M"], h["f_new"].shape[1]
    _, As, Ss, _ = compute_kfac_factors(h["state"], h["Z"], h["model_type"])
    _, Ae, Se, _ = compute_kfac_factors(h["state"], h["Z"], h["model_type"], example_chunk=max(1, M // 2))
    _, Ac, Sc, _ = kfac.compute_kfac_factors(h["state"], h["Z"], h["model_type"], class_chunk=max(1, K // 2))
    e_a = max(max(_rel(a, r) for a, r in zip(Ae, As)), max(_rel(a, r) for a, r in zip(Ac, As)))
    e_s = max(max(_rel(s, r) for s, r in zip(Se, Ss)), max(_rel(s, r) for s, r in zip(Sc, Ss)))
    print(f"{name}: chunked against unsplit  A {e_a:.2e}  S {e_s:.2e}")
    assert all(torch.equal(a, r) for a, r in zip(Ac, As))          # the input Grams do not see the class chunks
    assert e_a <= SPLIT_TOL and e_s <= SPLIT_TOL


# measured on MI355X, max|. - ref| / max|ref| of the posterior variance / predictive covariance / mean, scalar prior
# (two-group prior):
#   sine_regressor 1.24e-7 / 3.66e-7 / 3.20e-7 (1.24e-7 / 3.67e-7 / 3.20e-7)
#   xor_classifier 8.34e-8 / 6.26e-8 / 1.01e-7 (8.34e-8 / 7.45e-8 / 1.01e-7)
#   mlp_ragged     9.61e-8 / 1.22e-7 / 2.18e-7 (4.14e-8 / 1.32e-7 / 2.18e-7)
#   resnet_tiny    1.54e-7 / 5.62e-8 / 1.14e-7 (1.54e-7 / 5.62e-8 / 1.14e-7)
#   resnet50_tiny  2.80e-7 / 1.44e-7 / 2.47e-7 (2.80e-7 / 1.61e-7 / 2.47e-7)
#   flat_head      8.78e-8 / 8.60e-8 / 1.72e-7 (4.28e-8 / 6.32e-8 / 1.72e-7)
#   stem_net       8.79e-8 / 2.65e-8 / 2.06e-7 (8.79e-8 / 2.57e-8 / 2.06e-7)
VARIANCE_TOL = 1.2e-6          # 4 x 2.80e-7
PREDICT_TOL = 1.5e-6           # 4 x 3.67e-7
MEAN_TOL = 1.3e-6              # 4 x 3.20e-7


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kf.NETS)
def test_posterior_and_predictive_match_the_float64_helper(name, grouped):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    cov_blocks, _ = kf.covariance_blocks(state, h["As"], h["Ss"], h["M"], model_type, a, N_FULL)
    rem = h["rem"]
    rem_var = 1.0 / (a[rem] + h["diag"][rem])
    post = posterior_lla_kfac(state, Z, model_type, prior, full_set_size=N_FULL)
    assert isinstance(post, KFACNormal)
    theta = flatten_nn_params(state.params)[0]
    assert post.mean().dtype == F64 and torch.equal(post.mean().cpu(), theta.double())
    e_var = _rel(post.variance(), kf.variance_ref(state, cov_blocks, rem, rem_var))
    K = h["f_new"].shape[1]
    cov_ref = kf.predict_dense(h["J_new"], cov_blocks, rem, rem_var)
    full = predict_lla_kfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="full", batch=3)
    mean, var = predict_lla_kfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="diag", batch=3)
    assert isinstance(full, MultivariateNormalFullCovariance)
    if model_type == "regressor":
        assert full.mean().shape == (5,) and full.covariance().shape == (5, 5) and mean.shape == var.shape == (5,)
        cov = torch.diagonal(full.covariance())[:, None, None]
        var_full = torch.diagonal(full.covariance())
    else:
        assert full.mean().shape == (5, K) and full.covariance().shape == (5, K, K) and mean.shape == var.shape == (5, K)
        cov = full.covariance()
        var_full = torch.diagonal(cov, dim1=1, dim2=2)
        assert torch.equal(cov, cov.transpose(1, 2))
    # cov="diag" is the diagonal of cov="full" bitwise when both read the same rows: the kernel-level test, and below on
    # one set of rows with the remainder's term.  Here each call runs its own backward sweep, whose BN reductions may go
    # through float atomics: its rows can differ in the last bits from run to run, so the diag form gets the bound of the
    # full form (the rule of tests/test_subnetwork.py)
    assert var.shape == var_full.shape
    var_ref = torch.diagonal(cov_ref, dim1=1, dim2=2).to(DEV)
    assert ((var.reshape(5, K) - var_ref).abs().max() / cov_ref.abs().max()).item() <= PREDICT_TOL
    eng = get_engine(state, h["Xnew"], model_type)
    rows = eng._one_hot_rows(0, K, "raw")
    _, fits, rem_idx, rem_v, _ = kfac._cached_fit(state, Z, model_type, prior, N_FULL, None)
    triples = [f[:3] for f in fits]
    o_full = torch.zeros(5, K, K, device=DEV, dtype=F64)
    o_diag = torch.zeros(5, K, device=DEV, dtype=F64)
    eng._kfac_predict_rows(rows, 5, K, triples, (rem_idx, rem_v), o_full, False)
    eng._kfac_predict_rows(rows, 5, K, triples, (rem_idx, rem_v), o_diag, True)
    assert torch.equal(o_diag, torch.diagonal(o_full, dim1=1, dim2=2)) and torch.equal(o_full, o_full.transpose(1, 2))
    e_cov = _rel(cov, cov_ref)
    e_mean = _rel(mean.reshape(5, K), h["f_new"])
    print(f"{name} {'grouped' if grouped else 'scalar'}: variance {e_var:.2e} predictive {e_cov:.2e} mean {e_mean:.2e}")
    assert e_var <= VARIANCE_TOL and e_cov <= PREDICT_TOL and e_mean <= MEAN_TOL


# measured on MI355X: max|. - ref| / max|ref| of the draws f + J dtheta against the helper's, same seeded dtheta:
# sine_regressor 7.80e-7, xor_classifier 2.40e-7, mlp_ragged 4.91e-7, resnet_tiny 2.80e-7, resnet50_tiny 2.85e-7,
# flat_head 2.47e-7, stem_net 1.49e-7
SCALABLE_TOL = 3.2e-6          # 4 x 7.80e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_scalable_draws_match_the_helper_for_the_same_seeded_draws(name):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    out = predict_lla_kfac_scalable(state, h["Xnew"], Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=4)
    K = h["f_new"].shape[1]
    assert out.shape == (4, 5, K) and out.is_cuda and out.dtype == F32
    post = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N_FULL)
    d_theta = (post.sample((4,), seed=5, dtype=F64) - post.mean()).cpu()
    want = h["f_new"][None] + torch.einsum("bkd,sd->sbk", h["J_new"], d_theta)
    e = _rel(out, want)
    print(f"{name}: scalable draws {e:.2e}")
    assert e <= SCALABLE_TOL


# measured on MI355X: |got - want| / |want| of the evidence against the helper's spectrum: sine_regressor 2.26e-8
# (-41.0362870809 against -41.0362861552), xor_classifier 6.31e-9 (-50.8082035545 against -50.808203234), mlp_ragged
# 3.13e-8 (-176.38836165 against -176.388356135), resnet_tiny 3.08e-8 (-434.922471428 against -434.922484815),
# resnet50_tiny 2.59e-8 (-230.076718685 against -230.076724633), flat_head 1.04e-8 (-74.2200164191 against
# -74.2200171928), stem_net 3.36e-9 (-45.0688764351 against -45.0688765866)
LML_TOL = 1.3e-7               # 4 x 3.13e-8


@pytest.mark.parametrize("name", kf.NETS)
def test_evidence_matches_the_helper_spectrum_and_the_fit_does_not_lose_evidence(name):
    h = _helper(name)
    state, Z, model_type, alpha, M = h["state"], h["Z"], h["model_type"], h["alpha"], h["M"]
    spec = kf.spectrum_ref(state, h["As"], h["Ss"], M, model_type, kf.ggn_diag_ref(state, Z, model_type, None))
    theta = flatten_nn_params(state.params)[0].double()
    want = ref.lml_ref(alpha, spec, theta.numel(), float((theta ** 2).sum()), N_FULL / M)
    got = log_marginal_likelihood_kfac(alpha, Z, state, model_type, full_set_size=N_FULL)
    e = abs(got - want) / abs(want)
    print(f"{name}: evidence got {got:.12g} want {want:.12g} rel {e:.2e}")
    assert e <= LML_TOL
    a_fit, hist = fit_alpha_kfac(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=20)
    assert len(hist) == 20 and abs(hist[0][0] - alpha) <= 1e-14 * alpha and abs(hist[0][1] - got) <= 1e-12 * abs(got)
    assert a_fit > 0 and a_fit == a_fit and a_fit != float("inf")
    assert log_marginal_likelihood_kfac(a_fit, Z, state, model_type, full_set_size=N_FULL) >= hist[0][1]


def test_eval_dataset_probit_fits_the_posterior_once(monkeypatch):
    h = _helper("xor_classifier")
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    calls = []
    inner = kfac.compute_kfac_factors
    monkeypatch.setattr(kfac, "compute_kfac_factors", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N_FULL,
                                                               model_type, posterior="kfac")
    assert len(calls) == 1                                          # one fit for both batches
    assert probs.shape == (16, 2) and labels.shape == (16,)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), (nll, acc, brier, ece_)))
    assert bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1).abs() < 1e-9).all())
    assert kfac._FIT_CACHE
    clear_engine_cache()
    assert not kfac._FIT_CACHE                                      # clear_engine_cache drops the fitted factors


def test_engine_methods_check_their_operands():
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    blocks = eng.kfac_blocks()
    assert [(b.off, b.Mt, b.N, b.T) for b in blocks] == [(0, 19, 4, 9), (76, 37, 3, 1)] and blocks[1].final
    As = [torch.zeros(b.Mt, b.Mt, device=DEV, dtype=F64) for b in blocks]
    Ss = [torch.zeros(b.N, b.N, device=DEV, dtype=F64) for b in blocks]
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_factors(As[:1], Ss)
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_factors([As[0].float(), As[1]], Ss)
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_factors(As, [Ss[0].cpu(), Ss[1]])
    eng.kfac_factors(As, Ss)
    assert float(As[1][0, 0]) == h["Z"].shape[0] and float(As[0][0, 0]) == 9 * h["Z"].shape[0]       # sum of 1 * 1


def _conv_head_engine(n, hw, classes, max_chunk):
    """a 4-channel 3 x 3 conv on an hw x hw map and a Dense head, bound with at most ``max_chunk`` probes per pass"""
    from lip_amd.engine import LinearizedNet
    from lip_amd.netspec import NetSpec
    from lip_amd.toymodels import create_state
    net = NetSpec((hw, hw, 3))
    net.dense(net.conv(0, "Conv_0", 4, 3, act="relu", use_bias=True), "Dense_0", classes)
    state = create_state(net, 1, dtype=F32)
    Z = torch.rand(n, hw, hw, 3, generator=torch.Generator().manual_seed(n))
    return LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 30, max_chunk=max_chunk)


def _kron_scratch(eng, P):
    d = ctypes.c_int64(0)
    nv.check(eng.lib.lip_vjp_kron_scratch(eng.h, P, ctypes.byref(d)), "lip_vjp_kron_scratch")
    return d.value


def test_kron_scratch_query_covers_a_shorter_last_pass():
    """The partial tiles of a panel Gram are not monotone in its rows: with 800 spans per probe and one tile, a pass of 7
    probes needs more ranges than one of 8.  P = 15 on 8 probes per pass runs 8 + 7: the query covers both, a scratch one
    double short is refused before anything is added, and the result is that of the two passes as two calls."""
    eng = _conv_head_engine(50, 32, 3, 8)                           # 50 * 32 * 32 = 51 200 rows = 800 spans per probe
    assert eng.chunk == 8
    need = _kron_scratch(eng, 15)
    # one tile: 915 ranges for the pass of 8 probes, 934 for the pass of 7; the query answers for every pass size up to 8
    assert need >= 934 * 1024 and need == _kron_scratch(eng, 8) >= _kron_scratch(eng, 7)
    cap = 4
    koff, ooff, Ns = (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int32 * cap)()
    count, total = ctypes.c_int32(0), ctypes.c_int64(0)
    nv.check(eng.lib.lip_vjp_kron_layout(eng.h, cap, koff, ooff, Ns, ctypes.byref(count), ctypes.byref(total)), "layout")
    assert count.value == 2 and total.value == 4 * 4 + 3 * 3
    g = torch.Generator().manual_seed(0)
    U = torch.randn(15, eng.n, eng.K, generator=g, dtype=F32).to(DEV)
    scratch = torch.empty(need, device=DEV, dtype=F64)

    def run(Ublock, S, doubles):
        return eng.lib.lip_vjp_kron(eng.h, Ublock.data_ptr(), S.data_ptr(), Ublock.shape[0], nv.HEAD_IN, 1.0,
                                    scratch.data_ptr(), doubles, nv.stream_ptr())

    S0 = torch.full((total.value,), 2.0, device=DEV, dtype=F64)
    S = S0.clone()
    assert run(U, S, need - 1) == 1 and b"scratch" in eng.lib.lip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(S, S0)                                      # refused before the first launch
    S = torch.zeros(total.value, device=DEV, dtype=F64)
    assert run(U, S, need) == 0
    S2 = torch.zeros(total.value, device=DEV, dtype=F64)
    assert run(U[:8].contiguous(), S2, need) == 0 and run(U[8:].contiguous(), S2, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(S, S2) and bool((S.abs().sum() > 0).item())


def test_factors_on_a_binding_whose_probe_chunk_exceeds_the_classes():
    """25 probes per pass, K = 10 classes, 6400 rows per probe: the sweep's scratch is sized for the 10 probes it passes"""
    eng = _conv_head_engine(25, 16, 10, 25)
    assert eng.chunk == 25 and 1000 * 1024 <= _kron_scratch(eng, 10) <= _kron_scratch(eng, 25)      # 10 probes: 1000 ranges
    blocks = eng.kfac_blocks()
    As = [torch.zeros(b.Mt, b.Mt, device=DEV, dtype=F64) for b in blocks]
    Ss = [torch.zeros(b.N, b.N, device=DEV, dtype=F64) for b in blocks]
    eng.kfac_factors(As, Ss)
    assert all(bool(torch.isfinite(S).all()) and float(S.diagonal().min()) >= 0 and torch.equal(S, S.T) for S in Ss)
    assert float(Ss[0].diagonal().sum()) > 0
