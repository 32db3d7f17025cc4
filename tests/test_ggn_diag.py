"""GPU checks of the exact GGN diagonal (``lip_vjp_sqsum``, ``compute_ggn_diag``) and the diagonal Laplace posterior.

References: the float64 oracle's dense GGN on nets small enough for a D x D matrix, and, at full size, the square
of the materialised factor rows (the per-example ``vjp_rows`` sweep) summed in float64.  The kernels are f32 MFMA
with f32 accumulation of non-negative squares, so the bound is elementwise |d - ref| <= 1e-5 * max(ref).
"""
import ctypes
import math

import pytest
import torch

from lip_amd import _native as nv
from lip_amd.engine import LinearizedNet
from lip_amd.ggn import clear_engine_cache, compute_ggn_diag, get_engine, materialize_factor
from lip_amd.lla import posterior_lla_diag, predict_lla_diag_scalable, predict_lla_scalable
from lip_amd.sample import sample_diag
from lip_amd.scalemodels import LargeClassifier, LeNet5, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from lip_amd.utils import flatten_nn_params
from oracle.ggn import compute_ggn_dense

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _cases():
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
        "lenet5": (LeNet5(10), torch.rand(7, 28, 28, 1, dtype=F64, generator=g), "classifier"),
    }


def _recal(state, M, N, model_type):
    r = N / M
    if model_type == "regressor":
        r *= math.exp(-float(state.params["logvar"]["logvar"]))
    return r


def _max_err(d, ref):
    """max |d - ref| / max ref (ref float64 on the host)"""
    return ((d.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _onehots(eng):
    return torch.eye(eng.K, device=eng.device)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# 1. against the float64 oracle's dense GGN.  Measured on MI355X (max|d - ref| / max ref): sine_regressor 4.1e-8,
#    xor_classifier 1.5e-7, mlp_ragged 1.3e-7, resnet_tiny 2.7e-7, resnet50_tiny 3.0e-7
@pytest.mark.parametrize("name", ["sine_regressor", "xor_classifier", "mlp_ragged", "resnet_tiny", "resnet50_tiny"])
def test_diag_matches_float64_oracle(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    N = 7 * Z.shape[0] + 5                                   # full_set_size != M
    G, _, _ = compute_ggn_dense(state, Z, model_type, full_set_size=N)
    ref = torch.diagonal(G).clone()
    d = compute_ggn_diag(state, Z, model_type, full_set_size=N)
    torch.cuda.synchronize()
    assert d.shape == ref.shape and d.dtype == torch.float32 and d.is_cuda
    err = _max_err(d, ref)
    print(f"{name}: D={ref.numel()} max|d - ref| / max ref = {err:.2e}")
    assert err <= 1e-5, f"{name}: {err:.2e}"


# 2. full size, against the squared factor rows (vjp_rows) summed in float64.  Measured: resnet1m_cifar 1.0e-7,
#    lenet5 2.5e-7, mlp_wide 2.8e-7
def _full_cases():
    g = torch.Generator().manual_seed(11)
    return {
        "resnet1m_cifar": (ResNet1M(10), torch.rand(50, 32, 32, 3, generator=g)),
        "lenet5": (LeNet5(10), torch.rand(20, 28, 28, 1, generator=g)),
        "mlp_wide": (_cases()["mlp_wide"][0], _cases()["mlp_wide"][1].float()),
    }


@pytest.mark.parametrize("name", ["resnet1m_cifar", "lenet5", "mlp_wide"])
def test_diag_matches_squared_factor_rows_full_size(name):
    net, Z = _full_cases()[name]
    state = create_state(net, 1231231234, dtype=torch.float32)
    Zd = Z.cuda()
    N = 10 * Z.shape[0]
    d = compute_ggn_diag(state, Zd, "classifier", full_set_size=N)
    eng = get_engine(state, Zd, "classifier")
    Wm = materialize_factor(eng)                             # (n K, D)
    ref = torch.zeros(eng.D, device="cuda", dtype=F64)
    for s in range(0, Wm.shape[0], 50):
        ref += (Wm[s:s + 50].double() ** 2).sum(0)
    del Wm
    ref *= _recal(state, Z.shape[0], N, "classifier")
    torch.cuda.synchronize()
    err = ((d.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"{name}: D={eng.D} max|d - ref| / max ref = {err:.2e}")
    assert err <= 1e-5, f"{name}: {err:.2e}"


# 3. probe chunking: K = 10 probes on a 3-probe workspace (passes of 3 + 3 + 3 + 1 -> balanced 3, 3, 3, 1)
@pytest.mark.parametrize("name", ["mlp_wide", "resnet_small"])
def test_probe_chunks_agree(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64)
    big = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30, max_chunk=16)
    small = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30, max_chunk=3)
    assert small.chunk == 3 and big.chunk >= big.K
    a = big.vjp_sqsum(_onehots(big), "l")
    b = small.vjp_sqsum(_onehots(small), "l")
    torch.cuda.synchronize()
    assert ((a - b).abs().max() / a.abs().max()).item() <= 1e-6


# 4. example chunks
def test_example_chunks_agree_and_halves_average():
    net, Z, model_type = _cases()["resnet_small"]
    state = create_state(net, 3, dtype=F64)
    M = Z.shape[0]
    N = 1000
    whole = compute_ggn_diag(state, Z, model_type, full_set_size=N)
    chunked = compute_ggn_diag(state, Z, model_type, full_set_size=N, example_chunk=M // 2)
    h0 = compute_ggn_diag(state, Z[:M // 2].clone(), model_type, full_set_size=N)
    h1 = compute_ggn_diag(state, Z[M // 2:].clone(), model_type, full_set_size=N)
    torch.cuda.synchronize()
    scale = whole.abs().max()
    assert ((chunked - whole).abs().max() / scale).item() <= 1e-6
    assert (((h0 + h1) / 2 - whole).abs().max() / scale).item() <= 1e-6


# 5. the raw head with arbitrary cotangents
@pytest.mark.parametrize("name", ["mlp_ragged", "resnet_tiny", "resnet50_tiny"])
def test_raw_head_equals_squared_rows(name):
    net, Z, model_type = _cases()[name]
    state = create_state(net, 3, dtype=F64)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    U = torch.randn(3, eng.n, eng.K, generator=torch.Generator().manual_seed(4)).cuda()
    d = eng.vjp_sqsum(U, "raw")
    ref = (eng.vjp_rows(U, "raw").double() ** 2).sum((0, 1))
    torch.cuda.synchronize()
    assert ((d.double() - ref).abs().max() / ref.abs().max()).item() <= 1e-5
    # ... and it ADDS into a given output
    y = d.clone()
    eng.vjp_sqsum(U, "raw", out=y)
    torch.cuda.synchronize()
    assert torch.allclose(y, 2 * d, rtol=1e-6, atol=0)


# 6. determinism and refusals
def test_bitwise_reproducible_and_refusals_leave_y_untouched():
    net, Z, model_type = _cases()["resnet_small"]
    state = create_state(net, 3, dtype=F64)
    eng = LinearizedNet(state, Z, model_type, workspace_bytes=1 << 30)
    E = _onehots(eng)
    a = eng.vjp_sqsum(E, "l")
    b = eng.vjp_sqsum(E, "l")
    torch.cuda.synchronize()
    assert torch.equal(a, b)

    lib = eng.lib
    P = eng.K
    floats = ctypes.c_int64(0)
    assert lib.lip_vjp_sqsum_scratch(eng.h, P, ctypes.byref(floats)) == 0
    assert floats.value > 0                                  # this binding's reductions split into groups
    scratch = torch.empty(floats.value, device="cuda")
    Y = torch.full((eng.D,), 3.0, device="cuda")
    st = nv.stream_ptr()
    rc = lib.lip_vjp_sqsum(eng.h, nv.ptr(E), nv.ptr(Y), P, nv.HEAD_GGN, 1.0, nv.ptr(scratch), floats.value, st)
    assert rc == 1 and b"bad argument" in lib.lip_last_error()
    rc = lib.lip_vjp_sqsum(eng.h, nv.ptr(E), nv.ptr(Y), P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value - 1, st)
    assert rc == 1 and b"scratch" in lib.lip_last_error()
    rc = lib.lip_vjp_sqsum(eng.h, nv.ptr(E), None, P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value, st)
    assert rc == 1
    torch.cuda.synchronize()
    assert torch.equal(Y, torch.full_like(Y, 3.0))
    # the exact size is enough
    Y.zero_()
    assert lib.lip_vjp_sqsum(eng.h, nv.ptr(E), nv.ptr(Y), P, nv.HEAD_L, 1.0, nv.ptr(scratch), floats.value, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(Y, a)


# 7. ResNet-50, K = 1000 (reduced resolution): probe chunking, 1x1 projection weight gradients, max-pool, dense head.
#    Measured: 5.7e-7 of max on the 4 096 coordinates
def test_resnet50_k1000_subset_against_rows():
    net = ResNet50(1000, input_shape=(64, 64, 3))
    state = create_state(net, 5, dtype=torch.float32)
    Z = torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(6)).cuda()
    d = compute_ggn_diag(state, Z, "classifier")
    eng = get_engine(state, Z, "classifier")
    assert bool(torch.isfinite(d).all()) and bool((d >= 0).all())
    idx = torch.randperm(eng.D, generator=torch.Generator().manual_seed(7))[:4096].cuda()
    ref = torch.zeros(4096, device="cuda", dtype=F64)
    for k0 in range(0, eng.K, 50):
        k1 = min(eng.K, k0 + 50)
        E = torch.zeros(k1 - k0, eng.n, eng.K, device="cuda")
        E[torch.arange(k1 - k0), :, torch.arange(k0, k1)] = 1.0
        rows = eng.vjp_rows(E, "l")
        ref += (rows[:, :, idx].double() ** 2).sum((0, 1))
        del rows
    torch.cuda.synchronize()
    err = ((d[idx].double() - ref).abs().max() / ref.abs().max()).item()
    print(f"resnet50 K=1000: D={eng.D} subset max|d - ref| / max ref = {err:.2e}")
    assert err <= 1e-5


# 8. the diagonal posterior
def test_diag_posterior_variance_samples_and_prediction():
    net, Z, model_type = _cases()["xor_classifier"]
    state = create_state(net, 3, dtype=F64)
    alpha, N = 0.5, 100
    d = compute_ggn_diag(state, Z, model_type, full_set_size=N)
    post = posterior_lla_diag(state, Z, model_type, alpha, full_set_size=N)
    flat, _ = flatten_nn_params(state.params)
    assert torch.allclose(post.mean().double().cpu(), flat, rtol=0, atol=1e-6)
    assert torch.allclose(post.variance(), 1.0 / (alpha + d), rtol=1e-6, atol=0)
    assert torch.allclose(post.stddev() ** 2, post.variance(), rtol=1e-5)

    S = 4096
    draws = sample_diag(state, Z, flat.numel(), alpha, 17, model_type, num_samples=S, full_set_size=N)
    assert draws.shape == (S, flat.numel())
    var = (1.0 / (alpha + d)).double()
    emp = draws.double().pow(2).mean(0)                      # zero-mean draws
    se = var * math.sqrt(2.0 / S)
    assert bool(((emp - var).abs() <= 4 * se).all()), ((emp - var).abs() / se).max().item()
    assert torch.equal(draws, sample_diag(state, Z, flat.numel(), alpha, 17, model_type, num_samples=S, full_set_size=N))

    Xnew = torch.randn(5, 2, dtype=F64, generator=torch.Generator().manual_seed(3))
    pd = predict_lla_diag_scalable(state, Xnew, Z, model_type, alpha, key=2, full_set_size=N, num_samples=2048)
    pf = predict_lla_scalable(state, Xnew, Z, model_type, alpha, key=2, full_set_size=N, num_samples=3)
    assert pd.shape[1:] == pf.shape[1:] and pd.shape[0] == 2048
    fmu = get_engine(state, Xnew, model_type, workspace_bytes=4 << 30).outputs()
    sd = pd.double().std(0)
    assert bool(((pd.double().mean(0) - fmu.double()).abs() <= 5 * sd / math.sqrt(2048) + 1e-6).all())
