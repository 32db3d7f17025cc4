"""CPU checks of the last-layer Laplace posterior: the flat layout of theta_L, the refusals, and the float64 helper
(``tests/last_layer_ref.py``) that the GPU tests use as their yardstick, against the oracle's dense GGN slice and
autograd Jacobians.  Everything here is float64 on the host: the bound 1e-10 * max|ref| leaves four decades over the
rounding of sums of at most n K (D + 1) terms through a solve of condition <= 1001 (alpha = 1e-3 lambda_max)."""
import pytest
import torch

import last_layer_ref as ref
from lip_amd.engine import compile_net
from lip_amd.last_layer import LAST_LAYER_MAX_DIM, last_layer_slice
from lip_amd.netspec import NetSpec
from lip_amd.scalemodels import LargeClassifier, LeNet5, ResNet1M, ResNet50
from lip_amd.toymodels import LinearRegressor1D, SimpleClassifier, SimpleRegressor, create_state
from oracle.ggn import compute_ggn_dense

F64 = torch.float64
TOL = 1e-10


def _layout_nets():
    return {
        "simple_regressor": SimpleRegressor(8, 4),
        "simple_classifier": SimpleClassifier(16, 2, 2),
        "large_classifier": LargeClassifier((6, 6, 1), [40, 24], 2, 5),
        "lenet5": LeNet5(),
        "resnet1m": ResNet1M(4, (8, 8, 3), (4, 8, 12), 2),
        "resnet50": ResNet50(6, (20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
    }


@pytest.mark.parametrize("name", list(_layout_nets()))
def test_layout_matches_param_layout(name):
    net = _layout_nets()[name]
    state = create_state(net, 3, dtype=F64)
    boff, bshape, koff, kshape = ref.layout_of_final_dense(state)
    off, F, K = last_layer_slice(state)
    assert (off, F, K) == (boff, kshape[0], kshape[1])
    assert bshape == (K,) and koff == boff + K
    assert compile_net(net, 2, state.params).last_layer() == (off, F, K)


def test_refuses_activated_last_unit():
    net = NetSpec((4,))
    h = net.dense(0, "Dense_0", 8, act="relu")
    net.dense(h, "Dense_1", 3, act="tanh")
    with pytest.raises(ValueError, match="plain final Dense"):
        last_layer_slice(create_state(net, 0, dtype=F64))


def test_refuses_meanpool_ending():
    net = NetSpec((4, 4, 2))
    c = net.conv(0, "Conv_0", 4, 3, use_bias=True)
    net.meanpool(c)
    with pytest.raises(ValueError, match="final Dense"):
        last_layer_slice(create_state(net, 0, dtype=F64))


def test_refuses_kernel_before_bias():
    with pytest.raises(ValueError, match="directly before"):            # flat order (W, b)
        last_layer_slice(create_state(LinearRegressor1D(), 0, dtype=F64))


def test_cap_names_the_kronecker_posterior():
    net = NetSpec((6,))
    h = net.dense(0, "Dense_0", 100, act="relu")
    net.dense(h, "Dense_1", 100)
    assert 101 * 100 > LAST_LAYER_MAX_DIM
    with pytest.raises(ValueError, match="Kronecker-factored"):
        last_layer_slice(create_state(net, 0, dtype=F64))


def _algebra_cases():
    g = torch.Generator().manual_seed(0)
    return {
        "sine_regressor": (SimpleRegressor(8, 4), torch.randn(16, 1, dtype=F64, generator=g), "regressor"),
        "xor_classifier": (SimpleClassifier(16, 2, 2), torch.randn(32, 2, dtype=F64, generator=g), "classifier"),
        "mlp_ragged": (LargeClassifier((6, 6, 1), [40, 24], 2, 5), torch.rand(9, 6, 6, 1, dtype=F64, generator=g),
                       "classifier"),
        "resnet_tiny": (ResNet1M(4, input_shape=(8, 8, 3), widths=(4, 8, 12), blocks_per_stage=2),
                        torch.rand(3, 8, 8, 3, dtype=F64, generator=g), "classifier"),
    }


@pytest.mark.parametrize("name", list(_algebra_cases()))
def test_host_algebra_matches_oracle_and_jacobians(name):
    net, Z, model_type = _algebra_cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    off, F, K = last_layer_slice(state)
    sl = slice(off, off + (F + 1) * K)
    G = ref.ggn_last_layer_ref(state, Z, model_type, full_set_size=40)
    G_or = compute_ggn_dense(state, Z, model_type, full_set_size=40)[0][sl, sl]
    assert (G - G_or).abs().max() <= TOL * G_or.abs().max()
    assert (G - G.T).abs().max() <= 1e-15 * G.abs().max()
    alpha = 1e-3 * float(torch.linalg.eigvalsh(G_or).max())
    S = ref.covariance_ref(G, alpha)
    g = torch.Generator().manual_seed(7)
    Xnew = (torch.randn if Z.dim() == 2 else torch.rand)((5,) + tuple(Z.shape[1:]), dtype=F64, generator=g)
    f, cov = ref.predict_ref(state, Xnew, S)
    f_ag, J = ref.jac64(state, Xnew, model_type)
    JL = J[:, :, sl]
    cov_ag = JL @ torch.linalg.inv(G_or + alpha * torch.eye(G.shape[0], dtype=F64)) @ JL.transpose(-1, -2)
    assert (f - f_ag).abs().max() <= TOL * f_ag.abs().max()
    assert (cov - cov_ag).abs().max() <= TOL * cov_ag.abs().max()


def test_evidence_formula_matches_its_restatement():
    """``train_alpha._lml_from_spectrum`` on the helper's spectrum against the helper's restatement of the value"""
    from lip_amd.train_alpha import _lml_from_spectrum
    net, Z, model_type = _algebra_cases()["xor_classifier"]
    state = create_state(net, 3, dtype=F64)
    lam = torch.linalg.eigvalsh(ref.ggn_last_layer_ref(state, Z, model_type)).clamp_min(0.0)
    alpha = 1e-3 * float(lam.max())
    got = _lml_from_spectrum(alpha, lam, 34, 2.5, 40 / 32)[0]
    want = ref.lml_ref(alpha, lam, 34, 2.5, 40 / 32)
    assert abs(got - want) <= 1e-12 * abs(want)
