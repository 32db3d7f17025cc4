"""GPU checks of the layer-wise prior (``GroupedPrior``): the two new entry points (``lip_bdot_w``, ``lip_ggn_vp_diag``),
the per-group Grams, the layer-wise evidence and its fit, the whitened sampler and the predictives.

The float64 reference everywhere is the dense precision ``diag(a) + GGN`` with the oracle's dense GGN (N/M and
exp(-logvar) included) and autograd Jacobians; it is built once per net and shared.  Priors draw one precision per
group log-uniformly from [0.05, 20] (seeded), under both the "tensor" and the "layer" grouping.  Nets and the Jacobian
helper are those of tests/test_wnorm.py.  Bounds: the ones the scalar-alpha tests of this repository apply to the same
quantity (named at each test).  The predictive variances / marginals cancel; they are bounded at 4 x the worst error
measured on MI355X, the convention of tests/test_wnorm.py, with the measured figures next to the bound (test 8).
"""
import ctypes
import functools
import math

import pytest
import torch
from torch.func import jacrev

from lip_amd import _native as nv
from lip_amd import krylov
from lip_amd.engine import LinearizedNet
from lip_amd.ggn import clear_engine_cache, gram_from_factor, grouped_grams, materialize_factor
from lip_amd.lla import (compute_curvature_approx, predict_lla_diag, predict_lla_diag_scalable, predict_lla_marginals,
                         predict_lla_scalable, predict_lla_variances)
from lip_amd.prior import GroupedPrior
from lip_amd.sample import inv_matsqrt_vp, range_deflation, sample, sample_lanczos
from lip_amd.scalemodels import LargeClassifier, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from lip_amd.train_alpha import fit_alpha_layerwise, log_marginal_likelihood_layerwise
from lip_amd.utils import flatten_nn_params
from oracle.ggn import compute_ggn_dense
from oracle.lla import _flat_apply

pytestmark = pytest.mark.gpu
F64 = torch.float64
GROUPINGS = ["tensor", "layer"]
GGN_VP_TOL = 2e-4                                           # max|err| <= 2e-4 max|ref|: tests/test_hip_engine.py, test_golden.py
WNORM_TOL = 1e-5                                            # TOL of tests/test_wnorm.py


def _cases():
    """the small nets of tests/test_wnorm.py::_cases"""
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
    }


SMALL = ["sine_regressor", "xor_classifier", "mlp_ragged", "resnet_tiny", "resnet50_tiny"]
DENSE_D = ["sine_regressor", "xor_classifier", "mlp_ragged"]          # D small enough for D x D inverses


def _jac64(state, X, model_type):
    """(f (n, K), J (n, K, D)) in float64 by autograd (tests/test_wnorm.py::_jac64)"""
    flat, unravel = flatten_nn_params(state.params)
    fn = _flat_apply(state, unravel, model_type)
    n = X.shape[0]
    f = fn(flat, X).reshape(n, -1)
    J = torch.stack([jacrev(lambda fp: fn(fp, X[i:i + 1]).reshape(-1))(flat) for i in range(n)])
    return f.detach(), J.detach()


def _new_points(Z, B, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B,) + tuple(Z.shape[1:])
    return torch.randn(shape, dtype=F64, generator=g) if Z.dim() == 2 else torch.rand(shape, dtype=F64, generator=g)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(state, Z, model_type, N, dense float64 GGN on the device), built once per net and never written to"""
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    N = 7 * Z.shape[0] + 5
    G, _, _ = compute_ggn_dense(state, Z, model_type, full_set_size=N)
    return state, Z, model_type, N, G.detach().cuda()


@functools.lru_cache(maxsize=None)
def _new_jac(name):
    """(f (5, K), J (5, K, D)) float64 on the device at B = 5 new points, and the points"""
    state, Z, model_type, _, _ = _ref(name)
    Xnew = _new_points(Z, 5, 21)
    f, J = _jac64(state, Xnew, model_type)
    return Xnew, f.cuda(), J.cuda()


def _prior(state, groups, seed=17):
    """per-group precisions log-uniform in [0.05, 20]: a mean, the first value or a wrong group fail visibly"""
    G = GroupedPrior(state.params, 1.0, groups).G
    u = torch.rand(G, dtype=F64, generator=torch.Generator().manual_seed(seed))
    return GroupedPrior(state.params, torch.exp(math.log(0.05) + u * (math.log(20.0) - math.log(0.05))), groups)


def _scale(state, Z, model_type, N):
    return N / Z.shape[0] * (math.exp(-float(state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0)


def _err(v, ref):
    """max |v - ref| / max |ref| (ref float64)"""
    ref = ref.to(v.device)
    return ((v.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ---- 1. lip_bdot_w against float64 torch; the bound of tests/test_hip_krylov.py::test_bdot_axpby on lip_bdot
def _offset_block(P, N, seed, off):
    """a (P, N) block whose first element sits `off` floats past a 16-byte boundary"""
    buf = torch.empty(P * N + 4, device="cuda")
    X = buf[off:off + P * N].view(P, N)
    X.copy_(torch.randn(P, N, generator=torch.Generator().manual_seed(seed)))
    assert X.data_ptr() % 16 == 4 * off and X.is_contiguous()
    return X


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("P,N", [(1, 1), (3, 5), (3, 1027), (2, 4099)])
def test_bdot_w(P, N, off):
    X, Y = _offset_block(P, N, 1, off), _offset_block(P, N, 2, off)
    w = _offset_block(1, N, 3, off)[0]
    u = torch.rand(N, generator=torch.Generator().manual_seed(4))
    w.copy_(torch.exp(math.log(0.05) + u * (math.log(20.0) - math.log(0.05))))
    out = krylov.bdot_w(X, Y, w)
    torch.cuda.synchronize()
    ref = (w.double() * X.double() * Y.double()).sum(1)
    assert out.shape == (P,) and out.dtype == torch.float32
    print(f"bdot_w P={P} N={N} off={off}: max |out - ref| = {(out.double() - ref).abs().max().item():.3e}")
    assert torch.allclose(out.double(), ref, rtol=2e-5, atol=1e-3 * (N ** 0.5) * 1e-2)
    # w offset alone (the rows of an odd-N block meet w at every relative alignment anyway)
    w1 = _offset_block(1, N, 3, 1 - off)[0].copy_(w)
    out1 = krylov.bdot_w(X, Y, w1)
    torch.cuda.synchronize()
    assert torch.allclose(out1.double(), ref, rtol=2e-5, atol=1e-3 * (N ** 0.5) * 1e-2)
    lib = nv.load()
    assert lib.lip_bdot_w(nv.ptr(X), nv.ptr(Y), None, nv.ptr(out), P, N, nv.stream_ptr()) == 1     # LIP_ERR_ARG


# ---- 2. ggn_vp_diag against the dense float64 precision; the bound scalar-alpha lip_ggn_vp is held to on these nets
@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", SMALL)
def test_ggn_vp_diag_matches_dense_float64(name, groups):
    state, Z, model_type, N, G = _ref(name)
    prior = _prior(state, groups)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    a = prior.vector("cuda")
    V = torch.randn(3, eng.D, generator=torch.Generator().manual_seed(1)).cuda()
    V0 = V.clone()
    Y = eng.ggn_vp_diag(V, _scale(state, Z, model_type, N), a)
    torch.cuda.synchronize()
    ref = V.double() @ G + prior.vector("cuda", F64) * V.double()
    assert Y.shape == ref.shape and Y.dtype == torch.float32 and Y.is_cuda
    assert torch.equal(V, V0), "V was written to"
    err = _err(Y, ref)
    print(f"{name}/{groups}: D={eng.D} G={prior.G} max|Y - ref| / max|ref| = {err:.2e}")
    assert err <= GGN_VP_TOL, f"{name}/{groups}: {err:.2e}"


@pytest.mark.parametrize("groups", GROUPINGS)
def test_ggn_vp_diag_over_two_probe_chunks(groups):
    state, Z, model_type, N, G = _ref("xor_classifier")
    prior = _prior(state, groups)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 28, max_chunk=3)
    assert eng.chunk == 3
    V = torch.randn(5, eng.D, generator=torch.Generator().manual_seed(2)).cuda()       # passes of 3 and 2 probes
    out = torch.full_like(V, float("nan"))
    Y = eng.ggn_vp_diag(V, _scale(state, Z, model_type, N), prior.vector("cuda"), out=out)
    torch.cuda.synchronize()
    assert Y is out
    ref = V.double() @ G + prior.vector("cuda", F64) * V.double()
    err = _err(Y, ref)
    print(f"xor/{groups}: two chunks, max|Y - ref| / max|ref| = {err:.2e}")
    assert err <= GGN_VP_TOL


def test_ggn_vp_diag_status_codes():
    state, Z, model_type, N, _ = _ref("xor_classifier")
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 28)
    lib, st = eng.lib, nv.stream_ptr()
    V = torch.randn(2, eng.D, device="cuda")
    a = _prior(state, "layer").vector("cuda")
    Y = torch.full_like(V, 3.0)
    assert lib.lip_ggn_vp_diag(eng.h, nv.ptr(V), nv.ptr(Y), 2, 1.0, None, st) == 1            # LIP_ERR_ARG
    assert b"bad argument" in lib.lip_last_error()
    assert lib.lip_ggn_vp_diag(eng.h, None, nv.ptr(Y), 2, 1.0, nv.ptr(a), st) == 1
    assert lib.lip_ggn_vp_diag(eng.h, nv.ptr(V), None, 2, 1.0, nv.ptr(a), st) == 1
    h = ctypes.c_void_p()
    assert lib.lip_engine_create(ctypes.byref(h), eng.D, eng.n, eng.K) == 0
    assert lib.lip_ggn_vp_diag(h, nv.ptr(V), nv.ptr(Y), 2, 1.0, nv.ptr(a), st) == 3           # LIP_ERR_STATE
    assert b"not bound" in lib.lip_last_error()
    assert lib.lip_engine_destroy(h) == 0
    torch.cuda.synchronize()
    assert torch.equal(Y, torch.full_like(Y, 3.0)), "a refused call touched Y"
    with pytest.raises(ValueError):
        eng.ggn_vp_diag(V, 1.0, a[:-1])


# ---- 3. the operator's quadratic forms: v^T (GGN + diag a) v by the tangent sweep and lip_bdot_w against <v, op(v)> in
#         float64 and against the dense reference; the lip_bdot bound
@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", SMALL)
def test_quadratic_forms_match_products(name, groups):
    state, Z, model_type, N, G = _ref(name)
    prior = _prior(state, groups)
    op = compute_curvature_approx(state, Z, model_type, prior, full_set_size=N)
    D = op.engine.D
    V = torch.randn(4, D, generator=torch.Generator().manual_seed(3)).cuda()
    q = op.quadratic_forms(V)
    ref = (V.double() * op(V).double()).sum(1)
    dense = (V.double() * (V.double() @ G + prior.vector("cuda", F64) * V.double())).sum(1)
    torch.cuda.synchronize()
    assert q.shape == (4,) and q.dtype == F64
    print(f"{name}/{groups}: quadratic forms, max rel. to <v, op v> {((q - ref).abs() / ref).max().item():.2e}, "
          f"to dense {((q - dense).abs() / dense).max().item():.2e}")
    atol = 1e-3 * (D ** 0.5) * 1e-2
    assert torch.allclose(q, ref, rtol=2e-5, atol=atol)
    assert torch.allclose(q, dense, rtol=2e-5, atol=atol)
    assert torch.allclose(op(V[0]), op(V)[0], rtol=1e-4, atol=1e-5)      # a plain (D,) vector


# ---- 4. per-group Grams: every f32 x f32 product is exact in float64, so 1e-12 of max|G|
def _biases(path):
    return path[-1] == "bias"


@pytest.mark.parametrize("groups", GROUPINGS + ["biases"])
@pytest.mark.parametrize("name", SMALL)
def test_grouped_grams(name, groups):
    state, Z, model_type, _, _ = _ref(name)
    prior = GroupedPrior(state.params, 1.0, _biases) if groups == "biases" else _prior(state, groups)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    Wm = materialize_factor(eng, 0.9)
    grams = grouped_grams(Wm, prior)
    total = gram_from_factor(Wm)
    torch.cuda.synchronize()
    d = eng.n * eng.K
    assert grams.shape == (prior.G, d, d) and grams.dtype == F64
    tol = 1e-12 * total.abs().max().item()
    assert (grams.sum(0) - total).abs().max().item() <= tol
    assert torch.equal(grams, grams.transpose(1, 2))
    W64 = Wm.double()
    for g in range(prior.G):
        cols = torch.cat([W64[:, o:o + n] for o, n in prior.segments(g)], 1)
        assert (grams[g] - cols @ cols.T).abs().max().item() <= tol, (name, groups, g)


# ---- 5. the layer-wise evidence against the dense float64 determinant; the bound tests/test_next_rows.py applies to the
#         scalar evidence: |v - ref| <= 2e-4 max(1, |ref|)
@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", SMALL)
def test_layerwise_evidence_matches_dense_slogdet(name, groups):
    state, Z, model_type, N, G = _ref(name)
    prior = _prior(state, groups)
    v = log_marginal_likelihood_layerwise(prior, Z, state, model_type, full_set_size=N)
    a = prior.vector("cuda", F64)
    flat, _ = flatten_nn_params(state.params)
    logdet = torch.linalg.slogdet(torch.diag(a) + G)[1].item()
    ref = -0.5 * float((a * flat.cuda().double() ** 2).sum()) - 0.5 * (logdet - float((prior.sizes.double() * torch.log(prior.values)).sum()))
    shared = prior.with_values(torch.full((prior.G,), float(prior.values.mean()), dtype=F64))
    v_shared = log_marginal_likelihood_layerwise(shared, Z, state, model_type, full_set_size=N)
    print(f"{name}/{groups}: evidence {v:.9g} ref {ref:.9g} |diff| {abs(v - ref):.2e} (shared mean precision: {v_shared:.6g})")
    assert abs(v - ref) <= 2e-4 * max(1.0, abs(ref)), (v, ref)
    assert abs(v_shared - ref) > 2e-4 * max(1.0, abs(ref))              # the bound tells the precisions apart


# ---- 6. the fit: the evidence goes up, and the network is visited once
def test_fit_alpha_layerwise_builds_the_grams_once(monkeypatch):
    state, Z, model_type, N, _ = _ref("xor_classifier")
    calls = []
    real = krylov.dot_nt
    monkeypatch.setattr(krylov, "dot_nt", lambda A, B: (calls.append(A.shape), real(A, B))[1])
    prior, hist = fit_alpha_layerwise(Z, state, model_type, full_set_size=N, groups="layer", alpha0=1.0, steps=50)
    torch.cuda.synchronize()
    segments = sum(len(prior.segments(g)) for g in range(prior.G))
    assert len(calls) == segments == 3, calls                              # one pass over the factor for 50 steps
    monkeypatch.undo()
    assert len(hist) == 50 and prior.G == 3
    start = GroupedPrior(state.params, 1.0, "layer")
    v0 = log_marginal_likelihood_layerwise(start, Z, state, model_type, full_set_size=N)
    v1 = log_marginal_likelihood_layerwise(prior, Z, state, model_type, full_set_size=N)
    print(f"xor layer-wise fit: evidence {v0:.6g} -> {v1:.6g}, precisions {prior.values.tolist()}")
    assert abs(hist[0][1] - v0) <= 1e-9 * max(1.0, abs(v0))
    assert v1 > v0
    assert len(set(round(x, 6) for x in prior.values.tolist())) == 3        # the groups moved apart


# ---- 7. the sampler: T T^T against the dense float64 covariance; tests/test_sample.py holds the scalar map to
#         allclose(rtol, atol = rtol * max|ref|) with rtol = 3e-3 on the regressor and 5e-3 on the classifier; 3e-3 here
@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", DENSE_D)
def test_sampler_covariance_matches_dense_inverse(name, groups):
    state, Z, model_type, N, G = _ref(name)
    prior = _prior(state, groups)
    D = G.shape[0]
    fun = inv_matsqrt_vp(state, Z, D, prior, model_type, full_set_size=N)
    Tt = fun(torch.eye(D, device="cuda")).double()                          # row p = T e_p
    cov = Tt.T @ Tt
    ref = torch.linalg.inv(torch.diag(prior.vector("cuda", F64)) + G)
    torch.cuda.synchronize()
    print(f"{name}/{groups}: D={D} max|T T^T - S| / max|S| = {_err(cov, ref):.2e}")
    assert torch.allclose(cov, ref, rtol=3e-3, atol=3e-3 * ref.abs().max().item())
    scalar = torch.linalg.inv(float(prior.values.mean()) * torch.eye(D, device="cuda", dtype=F64) + G)
    assert not torch.allclose(scalar, ref, rtol=3e-3, atol=3e-3 * ref.abs().max().item())
    s1 = sample(state, Z, D, prior, 5, model_type, num_samples=6, full_set_size=N)
    s2 = sample(state, Z, D, prior, 6, model_type, num_samples=6, full_set_size=N)
    torch.cuda.synchronize()
    assert s1.shape == (6, D) and s1.dtype == torch.float32 and s1.is_cuda and bool(torch.isfinite(s1).all())
    assert not torch.equal(s1, s2)
    assert torch.equal(s1, sample(state, Z, D, prior, 5, model_type, num_samples=6, full_set_size=N))
    # another prior on the same binding gets parts of its own
    other = inv_matsqrt_vp(state, Z, D, prior.with_values(prior.values.flip(0)), model_type, full_set_size=N)
    assert other.parts is not fun.parts
    assert inv_matsqrt_vp(state, Z, D, prior, model_type, full_set_size=N).parts is fun.parts
    draws = predict_lla_scalable(state, _new_jac(name)[0], Z, model_type, prior, key=3, full_set_size=N, num_samples=4)
    assert draws.shape[:2] == (4, 5) and bool(torch.isfinite(draws).all())


# ---- 8. predictives at B = 5 new points against J S J^T with the dense float64 S = (diag(a) + GGN)^-1.  The inducing-
#         point variances and covariances are differences (var = jj - quad: jj the A^-1 metric norm of the Jacobian row,
#         quad the range part), so, as in tests/test_wnorm.py and tests/test_krylov_ops.py, the bound is 4 x the worst
#         error measured on MI355X against the float64 reference; the margin is for run-to-run variation in the f32
#         reductions of the Jacobian rows.  Measured on MI355X (tensor / layer grouping; two runs gave the same digits):
#           variances, max|v - ref| / max ref:
#             sine_regressor 1.49e-4 / 2.87e-5    xor_classifier 2.35e-5 / 5.46e-6    mlp_ragged 1.11e-6 / 6.29e-7
#           marginals, max|C - ref| / max|ref|:
#             sine_regressor 1.93e-5 / 5.56e-6    xor_classifier 2.37e-5 / 5.62e-6    mlp_ragged 1.49e-7 / 1.17e-7
#         The worst of the two groupings per net is held below; the bounds are 4 x these (variances 5.96e-4, 9.40e-5,
#         4.44e-6; marginals 7.72e-5, 9.48e-5, 5.96e-7).  The error follows the cancellation of the net (largest on
#         sine_regressor with one group per tensor) times the f32 rounding of the engine's rows: the variances carry the f32 tangent-
#         forward block J A^-1 Wm^T, the marginals only the f32 Jacobian rows (their products accumulate in float64).
#         The float64 reference with every precision replaced by the mean precision lies 3.28e-1 to 9.07e-1 of max|ref|
#         away on these cases, three orders above the widest bound: the test asserts that too.
VARIANCES_WORST = {"sine_regressor": 1.49e-4, "xor_classifier": 2.35e-5, "mlp_ragged": 1.11e-6}
MARGINALS_WORST = {"sine_regressor": 1.93e-5, "xor_classifier": 2.37e-5, "mlp_ragged": 1.49e-7}


def _dense_cov(name, prior):
    _, _, _, _, G = _ref(name)
    _, f, J = _new_jac(name)
    S = torch.linalg.inv(torch.diag(prior.vector("cuda", F64)) + G)
    return f, J @ S @ J.transpose(-1, -2)                                   # (B, K), (B, K, K)


@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", DENSE_D)
def test_predict_lla_variances_and_marginals(name, groups):
    state, Z, model_type, N, _ = _ref(name)
    prior = _prior(state, groups)
    Xnew = _new_jac(name)[0]
    f, ref = _dense_cov(name, prior)
    ref_var = torch.diagonal(ref, dim1=-2, dim2=-1)
    mean, var = predict_lla_variances(state, Xnew, Z, model_type, prior, full_set_size=N)
    dist = predict_lla_marginals(state, Xnew, Z, model_type, prior, full_set_size=N)
    torch.cuda.synchronize()
    cov = dist.covariance_matrix
    if model_type == "regressor":
        assert mean.shape == (5,) and var.shape == (5,) and cov.shape == (5, 5)
        mean, var, cov = mean[:, None], var[:, None], torch.diagonal(cov)[:, None, None]
    assert var.shape == ref_var.shape and var.dtype == F64 and cov.shape == ref.shape and cov.dtype == F64
    assert _err(mean, f) <= 1e-4                                            # an f32 forward pass
    assert bool((var > 0).all())
    e_var, e_cov = _err(var, ref_var), _err(cov, ref)
    _, ref_mean = _dense_cov(name, prior.with_values(torch.full((prior.G,), float(prior.values.mean()), dtype=F64)))
    e_mean = _err(ref_mean, ref)
    print(f"{name}/{groups}: variances max|v - ref| / max ref = {e_var:.2e}; marginals max|C - ref| / max|ref| = "
          f"{e_cov:.2e}; the mean precision in the float64 reference: {e_mean:.2e}")
    b_var, b_cov = 4 * VARIANCES_WORST[name], 4 * MARGINALS_WORST[name]
    assert e_mean > max(b_var, b_cov)                                       # either bound refuses the mean precision
    assert e_var <= b_var, f"{name}/{groups}: {e_var:.2e} > {b_var:.2e}"
    assert e_cov <= b_cov, f"{name}/{groups}: {e_cov:.2e} > {b_cov:.2e}"


@pytest.mark.parametrize("groups", GROUPINGS)
@pytest.mark.parametrize("name", SMALL)
def test_predict_lla_diag_with_a_grouped_prior(name, groups):
    state, Z, model_type, N, G = _ref(name)
    prior = _prior(state, groups)
    Xnew, f, J = _new_jac(name)
    ref = (J ** 2 / (prior.vector("cuda", F64) + torch.diagonal(G))).sum(-1)            # (B, K)
    mean, var = predict_lla_diag(state, Xnew, Z, model_type, prior, full_set_size=N)
    torch.cuda.synchronize()
    if model_type == "regressor":
        mean, var = mean[:, None], var[:, None]
    err = _err(var, ref)
    print(f"{name}/{groups}: diagonal-posterior variances max|v - ref| / max ref = {err:.2e}")
    assert var.shape == ref.shape and err <= WNORM_TOL, f"{name}/{groups}: {err:.2e}"
    assert _err(mean, f) <= 1e-4
    draws = predict_lla_diag_scalable(state, Xnew, Z, model_type, prior, key=5, full_set_size=N, num_samples=3)
    assert draws.shape[:2] == (3, 5) and bool(torch.isfinite(draws).all())


# ---- 9. what refuses a grouped prior says so
def test_refusals_name_the_limitation():
    state, Z, model_type, N, G = _ref("xor_classifier")
    prior = _prior(state, "layer")
    D = G.shape[0]
    with pytest.raises(ValueError, match="eigh"):
        inv_matsqrt_vp(state, Z, D, prior, model_type, full_set_size=N, method="lanczos")
    with pytest.raises(ValueError, match="eigh"):
        sample(state, Z, D, prior, 0, model_type, full_set_size=N, reference_compat=True)
    with pytest.raises(ValueError, match="clip_min"):
        inv_matsqrt_vp(state, Z, D, prior, model_type, full_set_size=N, clip_min=1.0)
    with pytest.raises(ValueError, match="scalar alpha"):
        sample_lanczos(state, Z, D, prior, 0, model_type, full_set_size=N)
    with pytest.raises(ValueError, match="scalar alpha"):
        range_deflation(state, Z, D, prior, model_type, full_set_size=N)
    import lip_amd.sample as smp
    limit = smp.FACTOR_BYTES_LIMIT
    try:
        smp.FACTOR_BYTES_LIMIT = 16
        with pytest.raises(ValueError, match="matrix-free"):
            inv_matsqrt_vp(state, Z, D, prior.with_values(prior.values * 2), model_type, full_set_size=N)
    finally:
        smp.FACTOR_BYTES_LIMIT = limit
    small = GroupedPrior.from_table([("all", [(0, D - 1)])], 1.0, D - 1)
    with pytest.raises(ValueError, match="parameters"):
        compute_curvature_approx(state, Z, model_type, small, full_set_size=N)
