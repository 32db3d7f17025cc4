"""GPU checks of the weighted-norm backward sweep (``lip_vjp_wnorm``) and the closed-form predictives built on it
(``predict_lla_diag``, ``predict_lla_variances``, ``probit_predictive``).

References: float64 Jacobians by autograd through ``oracle.lla._flat_apply`` and the oracle's dense GGN on nets small
enough for a D x D matrix; at full size the per-example rows (``vjp_rows``) weighted and summed in float64.  The
kernels are f32 MFMA with f32 accumulation of non-negative squares, so the bound on the norms is the one of the GGN
diagonal (tests/test_ggn_diag.py): elementwise |v - ref| <= 1e-5 * max(ref).  Quantities that cancel (polarisation, the
inducing-point variances, probit against Monte Carlo) are bounded at 4 x the worst error measured on MI355X, the
convention of tests/test_krylov_ops.py; the measured figures stand next to each bound.
"""
import ctypes
import math

import pytest
import torch
from torch.func import jacrev

from lip_amd import _native as nv
from lip_amd.engine import LinearizedNet
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache
from lip_amd.lla import (POLARISATION_MAX_K, predict_lla_diag, predict_lla_diag_scalable, predict_lla_marginals,
                         predict_lla_variances, probit_predictive)
from lip_amd.scalemodels import LargeClassifier, LeNet5, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from oracle.ggn import compute_ggn_dense
from oracle.lla import _flat_apply

pytestmark = pytest.mark.gpu
F64 = torch.float64
TOL = 1e-5                                                   # |v - ref| <= TOL * max(ref): squared f32 sums


def _cases():
    """the nets of tests/test_ggn_diag.py::_cases"""
    g = torch.Generator().manual_seed(0)
    return {
        "sine_regressor": (SimpleRegressor(8, 4), torch.randn(16, 1, dtype=F64, generator=g), "regressor"),
        "xor_classifier": (SimpleClassifier(16, 2, 2), torch.randn(32, 2, dtype=F64, generator=g), "classifier"),
        "mlp_ragged": (LargeClassifier((6, 6, 1), [40, 24], 2, 5), torch.rand(9, 6, 6, 1, dtype=F64, generator=g),
                       "classifier"),
        "mlp_wide": (LargeClassifier((12, 12, 1), [200, 136, 72], 3, 10), torch.rand(50, 12, 12, 1, dtype=F64, generator=g),
                     "classifier"),
        "resnet_tiny": (ResNet1M(4, input_shape=(8, 8, 3), widths=(4, 8, 12), blocks_per_stage=2),
                        torch.rand(3, 8, 8, 3, dtype=F64, generator=g), "classifier"),
        "resnet_small": (ResNet1M(10, input_shape=(16, 16, 3), widths=(32, 64, 128), blocks_per_stage=1),
                         torch.rand(6, 16, 16, 3, dtype=F64, generator=g), "classifier"),
        "resnet50_tiny": (ResNet50(6, input_shape=(20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
                          torch.rand(2, 20, 20, 3, dtype=F64, generator=g), "classifier"),
    }


SMALL = ["sine_regressor", "xor_classifier", "mlp_ragged", "resnet_tiny", "resnet50_tiny"]
SMALL_CLASSIFIERS = SMALL[1:]


def _new_points(Z, B, seed):
    """B test points of the shape (and range) of the examples Z"""
    g = torch.Generator().manual_seed(seed)
    shape = (B,) + tuple(Z.shape[1:])
    return torch.randn(shape, dtype=F64, generator=g) if Z.dim() == 2 else torch.rand(shape, dtype=F64, generator=g)


def _jac64(state, X, model_type):
    """(f (n, K), J (n, K, D)) in float64 by autograd; the nets run in inference mode, so example i's outputs depend on
    example i only"""
    from lip_amd.utils import flatten_nn_params
    flat, unravel = flatten_nn_params(state.params)
    fn = _flat_apply(state, unravel, model_type)
    n = X.shape[0]
    f = fn(flat, X).reshape(n, -1)
    J = torch.stack([jacrev(lambda fp: fn(fp, X[i:i + 1]).reshape(-1))(flat) for i in range(n)])
    return f.detach(), J.detach()


def _onehots(eng):
    return torch.eye(eng.K, device=eng.device)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()


def _err(v, ref):
    """max |v - ref| / max ref (ref float64)"""
    ref = ref.to(v.device)
    return ((v.double() - ref).abs().max() / ref.abs().max()).item()


def _wnorm_census(lib):
    n = lib.lip_debug_wnorm_route_count()
    counts, names = (ctypes.c_int64 * n)(), (ctypes.c_char_p * n)()
    nv.check(lib.lip_debug_wnorm_routes(counts, n, names), "lip_debug_wnorm_routes")
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# 1a. vjp_wnorm with arbitrary cotangents against float64 Jacobians.  Measured on MI355X (max|v - ref| / max ref,
#     weighted / w=None): sine_regressor 1.3e-7 / 1.4e-7, xor_classifier 9.1e-8 / 7.4e-8,
#     mlp_ragged 1.2e-7 / 1.1e-7, resnet_tiny 1.6e-7 / 1.4e-7, resnet50_tiny 8.7e-8 / 7.7e-8
@pytest.mark.parametrize("name", SMALL)
def test_wnorm_matches_float64_jacobians(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    _, J = _jac64(state, Z, model_type)                      # (n, K, D)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    g = torch.Generator().manual_seed(4)
    U = torch.randn(3, eng.n, eng.K, dtype=F64, generator=g)
    w = torch.rand(eng.D, dtype=F64, generator=g) + 0.05
    rows = torch.einsum("pik,ikd->pid", U, J)
    errs = []
    for wt in (w, None):
        ref = (rows ** 2 * (wt if wt is not None else 1.0)).sum(-1)
        v = eng.vjp_wnorm(U, wt, "raw")
        torch.cuda.synchronize()
        assert v.shape == ref.shape and v.dtype == torch.float32 and v.is_cuda
        errs.append(_err(v, ref))
    print(f"{name}: D={eng.D} max|v - ref| / max ref = {errs[0]:.2e} (weighted) {errs[1]:.2e} (w=None)")
    assert max(errs) <= TOL, f"{name}: {errs}"


# 1b. predict_lla_diag against J diag(1 / (alpha + diag G)) J^T with the oracle's dense float64 GGN.  Measured
#     (variances; means |f - ref| / max|ref|): sine_regressor 8.9e-8; 2.6e-7, xor_classifier 1.1e-7; 1.1e-7,
#     mlp_ragged 9.7e-8; 2.3e-7, resnet_tiny 1.2e-7; 3.1e-7, resnet50_tiny 3.8e-7; 2.3e-7
@pytest.mark.parametrize("name", SMALL)
def test_predict_lla_diag_matches_float64_oracle(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    alpha, N = 0.5, 7 * Z.shape[0] + 5
    Xnew = _new_points(Z, 5, 21)
    G, _, _ = compute_ggn_dense(state, Z, model_type, full_set_size=N)
    s2 = 1.0 / (alpha + torch.diagonal(G))
    f, J = _jac64(state, Xnew, model_type)
    ref = (J ** 2 * s2).sum(-1)                              # (B, K)
    mean, var = predict_lla_diag(state, Xnew, Z, model_type, alpha, full_set_size=N)
    torch.cuda.synchronize()
    if model_type == "regressor":
        assert mean.shape == (5,) and var.shape == (5,)
        mean, var = mean[:, None], var[:, None]
    assert var.shape == ref.shape and var.dtype == F64 and mean.shape == f.shape
    err, merr = _err(var, ref), _err(mean, f)
    print(f"{name}: variances max|v - ref| / max ref = {err:.2e}; means {merr:.2e}")
    assert err <= TOL, f"{name}: {err:.2e}"
    assert merr <= 1e-4, f"{name}: mean {merr:.2e}"         # an f32 forward pass (the bound of the smoke run)
    assert bool((var > 0).all())


# 2. full size, against the rows route: vjp_rows weighted and summed in float64.  Measured (weighted / w=None):
#    resnet1m_cifar 3.0e-7 / 2.8e-7, lenet5 1.5e-7 / 1.2e-7, mlp_wide 9.9e-8 / 1.2e-7
def _full_cases():
    g = torch.Generator().manual_seed(11)
    return {
        "resnet1m_cifar": (ResNet1M(10), torch.rand(50, 32, 32, 3, generator=g)),
        "lenet5": (LeNet5(10), torch.rand(20, 28, 28, 1, generator=g)),
        "mlp_wide": (_cases()["mlp_wide"][0], _cases()["mlp_wide"][1].float()),
    }


@pytest.mark.parametrize("name", ["resnet1m_cifar", "lenet5", "mlp_wide"])
def test_wnorm_matches_weighted_rows_full_size(name):
    net, X = _full_cases()[name]
    state = create_state(net, 1231231234, dtype=torch.float32)
    eng = LinearizedNet(state, X.cuda(), "classifier", workspace_bytes=4 << 30)
    E = _onehots(eng)
    w = (torch.rand(eng.D, generator=torch.Generator().manual_seed(12)) + 0.05).cuda()
    ref_w = torch.zeros(eng.K, eng.n, device="cuda", dtype=F64)
    ref_1 = torch.zeros_like(ref_w)
    for k in range(eng.K):
        r2 = eng.vjp_rows(E[k:k + 1], "raw")[0].double() ** 2           # (n, D)
        ref_w[k] = r2 @ w.double()
        ref_1[k] = r2.sum(-1)
        del r2
    e_w = _err(eng.vjp_wnorm(E, w, "raw"), ref_w)
    e_1 = _err(eng.vjp_wnorm(E, None, "raw"), ref_1)
    torch.cuda.synchronize()
    print(f"{name}: D={eng.D} max|v - ref| / max ref = {e_w:.2e} (weighted) {e_1:.2e} (w=None)")
    assert max(e_w, e_1) <= TOL, f"{name}: {e_w:.2e} {e_1:.2e}"


# 3. cov="full" by polarisation against the float64 J S J^T, S = diag(1 / (alpha + diag G)).  The off-diagonal entries
#    are differences of three norms, so the error is bounded at 4 x the worst measured.  Measured max|C - ref| / max|ref|
#    on MI355X: xor_classifier 3.03e-7, mlp_ragged 1.20e-7, resnet_tiny 5.58e-7,
#    resnet50_tiny 3.21e-7; worst 5.58e-7, bound 4 x = 2.23e-6
FULL_COV_WORST = 5.58e-7
FULL_COV_BOUND = 4 * FULL_COV_WORST


@pytest.mark.parametrize("name", SMALL_CLASSIFIERS)
def test_full_covariance_by_polarisation(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64)
    alpha, N = 0.5, 7 * Z.shape[0] + 5
    Xnew = _new_points(Z, 5, 22)
    G, _, _ = compute_ggn_dense(state, Z, model_type, full_set_size=N)
    s2 = 1.0 / (alpha + torch.diagonal(G))
    f, J = _jac64(state, Xnew, model_type)
    ref = (J * s2) @ J.transpose(-1, -2)                     # (B, K, K)
    dist = predict_lla_diag(state, Xnew, Z, model_type, alpha, full_set_size=N, cov="full")
    torch.cuda.synchronize()
    C = dist.covariance_matrix
    assert C.shape == ref.shape and C.dtype == F64
    assert torch.equal(C, C.transpose(-1, -2)), "the covariances are not symmetric"
    assert _err(dist.loc, f) <= 1e-4
    _, var = predict_lla_diag(state, Xnew, Z, model_type, alpha, full_set_size=N)
    assert _err(torch.diagonal(C, dim1=-2, dim2=-1), var) <= 2e-6       # (2 e_k against e_k: the same tiles, scaled)
    err = _err(C, ref)
    print(f"{name}: K={C.shape[-1]} max|C - ref| / max|ref| = {err:.2e}")
    assert err <= FULL_COV_BOUND, f"{name}: {err:.2e} > {FULL_COV_BOUND:.2e}"


def test_full_covariance_refuses_many_outputs():
    K = POLARISATION_MAX_K + 1
    net = LargeClassifier((4, 4, 1), [12], 1, K)
    state = create_state(net, 3, dtype=F64)
    g = torch.Generator().manual_seed(0)
    Z, Xnew = torch.rand(4, 4, 4, 1, dtype=F64, generator=g), torch.rand(2, 4, 4, 1, dtype=F64, generator=g)
    with pytest.raises(ValueError, match="refused"):
        predict_lla_diag(state, Xnew, Z, "classifier", 0.5, cov="full")
    mean, var = predict_lla_diag(state, Xnew, Z, "classifier", 0.5)    # the variances have no such limit
    assert mean.shape == (2, K) and var.shape == (2, K)


# 4. predict_lla_variances against the diagonal of predict_lla_marginals (float64 products on the materialised rows).
#    var = (||J_k||^2 - (J W)_k C (J W)_k^T) / alpha cancels more the smaller alpha is, so the bound is 4 x the worst
#    relative error max |v - ref| / ref measured on MI355X, per alpha:
#      xor    alpha 0.5: 3.06e-7    alpha 0.005: 1.36e-6
#      resnet alpha 0.5: 1.90e-5    alpha 0.005: 2.22e-5
#    worst per alpha 1.90e-5 and 2.22e-5 (bounds 7.6e-5 and 8.9e-5).  The ResNet error is the same at both alphas: it is
#    the f32 tangent-forward J W against the float64-accumulated products of the rows route, not the cancellation;
#    alpha = 0.005 keeps more than four digits (the finish kernel adds the tile partials in float64 in any case).
VARIANCES_WORST = {0.5: 1.90e-5, 0.005: 2.22e-5}


def _variance_cases():
    g = torch.Generator().manual_seed(31)
    xor, Zx, _ = _cases()["xor_classifier"]
    return {
        "xor": (xor, Zx.float(), torch.randn(16, 2, generator=g), 100, 3),
        # ResNet1M at 32 x 32 with 50 inducing images (the CIFAR config of tests/test_sampler_fullsize.py)
        "resnet1m": (ResNet1M(10), torch.rand(50, 32, 32, 3, generator=g), torch.rand(16, 32, 32, 3, generator=g), 49000,
                     1231231234),
    }


@pytest.mark.parametrize("alpha", [0.5, 0.005])
@pytest.mark.parametrize("name", ["xor", "resnet1m"])
def test_variances_match_marginals_diagonal(name, alpha):
    net, Z, Xnew, N, seed = _variance_cases()[name]
    state = create_state(net, seed, dtype=torch.float32)
    Z, Xnew = Z.cuda(), Xnew.cuda()
    dist = predict_lla_marginals(state, Xnew, Z, "classifier", alpha, full_set_size=N)
    ref = torch.diagonal(dist.covariance_matrix, dim1=-2, dim2=-1)      # (B, K)
    mean, var = predict_lla_variances(state, Xnew, Z, "classifier", alpha, full_set_size=N)
    torch.cuda.synchronize()
    assert var.shape == ref.shape and var.dtype == F64
    assert torch.equal(mean, dist.loc.reshape(mean.shape))
    assert bool((ref > 0).all())
    rel = ((var - ref).abs() / ref).max().item()
    print(f"{name} alpha={alpha}: max |v - ref| / ref = {rel:.2e} (variances in [{ref.min().item():.3e}, {ref.max().item():.3e}])")
    bound = 4 * VARIANCES_WORST[alpha]
    assert rel <= bound, f"{name} alpha={alpha}: {rel:.2e} > {bound:.2e}"


# 5. mechanics
# probe chunking: K = 10 probes on a 3-probe workspace (passes of 3, 3, 3, 1) against a single pass
@pytest.mark.parametrize("name", ["mlp_wide", "resnet_small"])
def test_probe_chunks_agree(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64)
    big = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30, max_chunk=16)
    small = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30, max_chunk=3)
    assert small.chunk == 3 and big.chunk >= big.K == 10
    w = (torch.rand(big.D, generator=torch.Generator().manual_seed(5)) + 0.05).cuda()
    a = big.vjp_wnorm(_onehots(big), w, "raw")
    b = small.vjp_wnorm(_onehots(small), w, "raw")
    torch.cuda.synchronize()
    assert ((a - b).abs().max() / a.abs().max()).item() <= 1e-6


# the 'l' head with a scale, against the rows; out= is added into; two runs are bitwise equal; refusals leave out alone
def test_l_head_out_accumulates_bitwise_reproducible_and_refusals():
    net, Z, model_type = _cases()["resnet_small"]
    state = create_state(net, 3, dtype=F64)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    g = torch.Generator().manual_seed(6)
    U = torch.randn(3, eng.n, eng.K, generator=g).cuda()
    w = (torch.rand(eng.D, generator=g) + 0.05).cuda()
    a = eng.vjp_wnorm(U, w, "l", 0.7)
    ref = (eng.vjp_rows(U, "l", 0.7).double() ** 2) @ w.double()
    torch.cuda.synchronize()
    assert _err(a, ref) <= TOL
    b = eng.vjp_wnorm(U, w, "l", 0.7)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "lip_vjp_wnorm is not bitwise reproducible"
    y = a.clone()
    eng.vjp_wnorm(U, w, "l", 0.7, out=y)
    torch.cuda.synchronize()
    assert torch.allclose(y, 2 * a, rtol=1e-6, atol=0)

    lib, P = eng.lib, 3
    floats = ctypes.c_int64(0)
    assert lib.lip_vjp_wnorm_scratch(eng.h, P, ctypes.byref(floats)) == 0
    assert floats.value > 0
    scratch = torch.empty(floats.value, device="cuda")
    out = torch.full((P, eng.n), 3.0, device="cuda")
    st = nv.stream_ptr()
    rc = lib.lip_vjp_wnorm(eng.h, nv.ptr(U), nv.ptr(w), nv.ptr(out), P, nv.HEAD_GGN, 1.0, nv.ptr(scratch), floats.value, st)
    assert rc == 1 and b"bad argument" in lib.lip_last_error()
    rc = lib.lip_vjp_wnorm(eng.h, nv.ptr(U), nv.ptr(w), nv.ptr(out), P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value - 1, st)
    assert rc == 1 and b"scratch" in lib.lip_last_error()
    assert lib.lip_vjp_wnorm(eng.h, nv.ptr(U), nv.ptr(w), None, P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value, st) == 1
    assert lib.lip_vjp_wnorm(eng.h, None, nv.ptr(w), nv.ptr(out), P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value, st) == 1
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 3.0))
    # the exact size is enough
    out.zero_()
    assert lib.lip_vjp_wnorm(eng.h, nv.ptr(U), nv.ptr(w), nv.ptr(out), P, nv.HEAD_L, 0.7, nv.ptr(scratch), floats.value, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, a)


# every tile variant of the dispatcher, the dense form and the reduce form in the census of the new kernels: the two
# nets of tests/test_kernel_routes.py (SQSUM_NETS) — the dispatcher picks its tiles as launch_wgrad_sqsum does
def _net_a():
    """tiles <2,2,1,2>, <4,1,1,2>, <2,2,2,2>, <4,1,1,1>, the dense form and the bias reduce"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((6, 6, 3))
    x = net.conv(0, "Conv_0", 72, 3, 1, padding=1, act="relu", use_bias=True)       # M = 27, N = 72
    x = net.conv(x, "Conv_1", 40, 3, 1, padding=1, act="relu")                      # M = 648, N = 40
    x = net.conv(x, "Conv_2", 80, 3, 1, padding=1, act="relu")                      # M = 360, N = 80
    x = net.conv(x, "Conv_3", 20, 3, 1, padding=1, act="relu")                      # M = 720, N = 20
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 5)
    net.model_type = "classifier"
    return net


def _net_b():
    """tiles <4,1,1,1>, <2,2,1,1>, <2,1,1,1>, the dense form and the bias reduce"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((8, 8, 32))
    x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, act="relu", use_bias=True)       # M = 288, N = 32
    x = net.conv(x, "Conv_1", 48, 1, 1, padding=0, act="relu")                      # M = 32, N = 48
    x = net.conv(x, "Conv_2", 16, 1, 1, padding=0, act="relu")                      # M = 48, N = 16
    x = net.meanpool(x)
    x = net.dense(x, "Dense_0", 40, act="relu")
    net.dense(x, "Dense_1", 5)
    net.model_type = "classifier"
    return net


WNORM_NETS = {"a": {"wgrad_wnorm<2,2,1,2>", "wgrad_wnorm<4,1,1,2>", "wgrad_wnorm<2,2,2,2>", "wgrad_wnorm<4,1,1,1>",
                    "wgrad_wnorm_dense", "reduce_wnorm", "wnorm_finish"},
              "b": {"wgrad_wnorm<4,1,1,1>", "wgrad_wnorm<2,2,1,1>", "wgrad_wnorm<2,1,1,1>", "wgrad_wnorm_dense",
                    "reduce_wnorm", "wnorm_finish"}}
# non-square inputs (aniso_nets.per_example_nets): between them every tile and the dense form
WNORM_NETS["c"] = set(WNORM_NETS["a"])
WNORM_NETS["d"] = set(WNORM_NETS["b"])


def _net_of(which):
    if which in ("c", "d"):
        from aniso_nets import per_example_nets
        return per_example_nets()[which]
    return _net_a() if which == "a" else _net_b()


@pytest.mark.parametrize("which", ["c", "d"])
def test_non_square_nets_match_float64_rows_of_the_emulator(which):
    """every variant on non-square maps, element by element against the float64 weighted norms of the tape emulator's
    per-example rows (not the engine's own rows)"""
    from test_kernel_routes import _bind
    n, P = 3, 2
    eng, tm, _ = _bind(_net_of(which), n, 7, P)
    g = torch.Generator().manual_seed(3)
    U = torch.randn(P, n, eng.K, dtype=F64, generator=g)
    w = (torch.rand(eng.D, dtype=F64, generator=g) + 0.05).float().double()
    rows = torch.zeros(P, n, eng.D, dtype=F64)
    for i in range(n):
        Ui = torch.zeros_like(U)
        Ui[:, i] = U[:, i]
        rows[:, i] = tm.vjp(Ui, nv.HEAD_L, 0.7)
    _wnorm_census(eng.lib)                                   # clear
    for wt in (w.float().cuda(), None):
        v = eng.vjp_wnorm(U.float().cuda(), wt, "l", 0.7)
        torch.cuda.synchronize()
        census = _wnorm_census(eng.lib)
        assert WNORM_NETS[which] <= set(census), f"{sorted(WNORM_NETS[which] - set(census))} not launched ({census})"
        ref = (rows ** 2) @ (wt.double().cpu() if wt is not None else torch.ones(eng.D, dtype=F64))
        e = _err(v.reshape(ref.shape), ref)
        print(f"non-square net {which}, w {'given' if wt is not None else 'None'}: max|v - ref| / max ref = {e:.3g}")
        assert e <= TOL, e


@pytest.mark.parametrize("which", ["a", "b"])
def test_several_pairs_per_group_last_group_short(which):
    """517 pairs: every tile, the dense form and the reduce walk 2, 4 or 7 pairs per block and end on a short group
    (tests/test_kernel_routes.py works the groups out and shares the float64 rows of the tape emulator)"""
    from test_kernel_routes import MANY_N, MANY_P, assert_several_pairs_per_group, many_pairs
    assert_several_pairs_per_group(_net_of(which), MANY_P * MANY_N)
    eng, _, U, rows = many_pairs(which)
    w = (torch.rand(eng.D, dtype=F64, generator=torch.Generator().manual_seed(4)) + 0.05).float().double()
    _wnorm_census(eng.lib)                                   # clear
    for wt in (w.float().cuda(), None):
        v = eng.vjp_wnorm(U.float().cuda(), wt, "l", 0.7)
        torch.cuda.synchronize()
        census = _wnorm_census(eng.lib)
        assert WNORM_NETS[which] <= set(census), f"{sorted(WNORM_NETS[which] - set(census))} not launched ({census})"
        ref = (rows ** 2) @ (wt.double().cpu() if wt is not None else torch.ones(eng.D, dtype=F64))
        e = _err(v.reshape(ref.shape), ref)
        print(f"net {which}, 517 pairs, w {'given' if wt is not None else 'None'}: max|v - ref| / max ref = {e:.3g}")
        assert e <= TOL, e


@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
def test_census_shows_every_variant_and_values_match_rows(which):
    net = _net_of(which)
    state = create_state(net, 7, dtype=F64)
    Z = torch.rand(3, *net.tensors[0], dtype=F64, generator=torch.Generator().manual_seed(7))
    eng = LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 28, max_chunk=2)
    g = torch.Generator().manual_seed(3)
    U = torch.randn(2, 3, eng.K, generator=g).cuda()
    w = (torch.rand(eng.D, generator=g) + 0.05).cuda()
    _wnorm_census(eng.lib)                                   # clear
    v = eng.vjp_wnorm(U, w, "l", 0.7)
    torch.cuda.synchronize()
    census = _wnorm_census(eng.lib)
    assert WNORM_NETS[which] <= set(census), f"net {which}: {sorted(WNORM_NETS[which] - set(census))} not launched ({census})"
    # one finish launch per tile / dense / reduce launch
    assert census["wnorm_finish"] == sum(c for r, c in census.items() if r != "wnorm_finish")
    assert not _wnorm_census(eng.lib)                        # reading clears
    ref = (eng.vjp_rows(U, "l", 0.7).double() ** 2) @ w.double()
    assert _err(v, ref) <= TOL


def test_all_six_tiles_are_covered_by_the_two_nets():
    lib = nv.load()
    n = lib.lip_debug_wnorm_route_count()
    names = (ctypes.c_char_p * n)()
    nv.check(lib.lip_debug_wnorm_routes(None, n, names), "lip_debug_wnorm_routes")
    assert {names[i].decode() for i in range(n)} == WNORM_NETS["a"] | WNORM_NETS["b"]


# the scratch never scales with D x pairs: at the CIFAR config (256 images, K = 10 probes) it is (pairs) x (18 output
# tiles of the largest op) floats against the 2.8e9 floats of the (P, n, D) rows block.  Measured ratio: 23 040 floats against 2 776 540 160: 8.3e-6
def test_scratch_is_a_sliver_of_the_rows_block_at_the_cifar_config():
    state = create_state(ResNet1M(10), 1231231234, dtype=torch.float32)
    X = torch.rand(256, 32, 32, 3, generator=torch.Generator().manual_seed(8)).cuda()
    eng = LinearizedNet(state, X, "classifier", workspace_bytes=8 << 30, max_chunk=10)
    assert eng.chunk == 10
    floats = ctypes.c_int64(0)
    nv.check(eng.lib.lip_vjp_wnorm_scratch(eng.h, eng.K, ctypes.byref(floats)), "lip_vjp_wnorm_scratch")
    rows = eng.K * eng.n * eng.D
    print(f"cifar config: scratch {floats.value} floats, rows block {rows} floats, ratio {floats.value / rows:.2e}")
    assert 0 < floats.value < rows / 1000
    assert floats.value % (eng.K * eng.n) == 0               # whole tiles of one pass's pairs
    v = eng.vjp_wnorm(_onehots(eng), None, "raw")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v).all()) and bool((v > 0).all())


# 6. the probit predictive against the mean softmax of 4000 draws of the same posterior on the XOR config.  Both sides
#    approximate the same integral (probit: the link; the draws: sampling noise ~ 0.5 / sqrt(4000) = 8e-3), so the gap
#    is bounded at 4 x the measured one.  Measured max |p_probit - p_mc| on MI355X: 9.04e-3 (bound 3.6e-2)
PROBIT_GAP = 9.04e-3


def test_probit_predictive_close_to_monte_carlo_and_evaluate_entry():
    net, Z, model_type = _cases()["xor_classifier"]
    state = create_state(net, 3, dtype=F64)
    alpha, N = 0.5, 100
    Xnew = _new_points(Z, 24, 23)
    mean, var = predict_lla_diag(state, Xnew, Z, model_type, alpha, full_set_size=N)
    probs = probit_predictive(mean, var)
    draws = predict_lla_diag_scalable(state, Xnew, Z, model_type, alpha, key=5, full_set_size=N, num_samples=4000)
    mc = torch.softmax(draws.double(), -1).mean(0)
    torch.cuda.synchronize()
    assert probs.shape == mc.shape
    assert torch.allclose(probs.sum(-1), torch.ones_like(probs[:, 0]), atol=1e-12)
    # the draws' variance is the closed-form variance (4000 draws: 4 standard errors)
    emp = draws.double().var(0)
    assert bool(((emp - var).abs() <= 4 * var * math.sqrt(2.0 / 4000)).all())
    gap = (probs - mc).abs().max().item()
    print(f"xor: max |p_probit - p_mc| = {gap:.2e}")
    assert gap <= 4 * PROBIT_GAP, f"{gap:.2e} > {4 * PROBIT_GAP:.2e}"

    y = torch.randint(0, 2, (24,), generator=torch.Generator().manual_seed(9))
    loader = [(Xnew[:16], y[:16]), (Xnew[16:], y[16:])]
    for posterior in ("diag", "inducing"):
        nll, acc, brier, ece_, p, labels = eval_dataset_probit(state, loader, Z, alpha, N, model_type, posterior=posterior)
        assert p.shape == (24, 2) and labels.shape == (24,)
        assert math.isfinite(nll) and nll > 0 and 0.0 <= acc <= 1.0 and 0.0 <= brier <= 2.0 and 0.0 <= ece_ <= 1.0
        if posterior == "diag":
            assert torch.allclose(p, probs, atol=1e-12)
            assert abs(acc - (probs.argmax(-1).cpu() == y).double().mean().item()) < 1e-12
