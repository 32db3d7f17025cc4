"""CPU checks of the EKFAC second moments from backward sweeps: the refusals of the public surface, which come before
anything is bound, the definition the GPU tests rely on (``tests/ekfac_sweep_ref.py`` fed the exact-expectation cotangents
equals ``ekfac_ref.scales_ref``), and the key of the one-entry fit cache."""
import pytest
import torch

import ekfac_ref as er
import ekfac_sweep_ref as sr
import fisher_ref as fr
import kfac_ref as kf
from lip_amd import ekfac, fisher
from lip_amd.ggn import compute_ekfac_scales
from lip_amd.lla import posterior_lla_ekfac, predict_lla_ekfac
from lip_amd.train_alpha import log_marginal_likelihood_ekfac

F64 = torch.float64


def _bases(state):
    return [(torch.eye(Mt, dtype=F64), torch.eye(N, dtype=F64)) for _, _, Mt, N, _, _ in kf.blocks_of(state)]


@pytest.fixture
def no_binding(monkeypatch):
    """any attempt to bind an engine fails the test: the refusals below come first"""
    def refuse(*a, **kw):
        raise AssertionError("an engine was bound before the arguments were checked")
    monkeypatch.setattr(ekfac, "_engines", refuse)
    monkeypatch.setattr(ekfac._ggn, "get_engine", refuse)


def test_curvature_with_the_rows_route_is_refused(no_binding):
    state, Z, model_type = kf.make_case("xor_classifier")
    spec = fisher.MCFisher(2, 0)
    with pytest.raises(ValueError, match="sweep"):
        compute_ekfac_scales(state, Z, model_type, _bases(state), moments="rows", curvature=spec)
    with pytest.raises(ValueError, match="sweep"):
        compute_ekfac_scales(state, Z, model_type, _bases(state), curvature=spec)          # "rows" is the default
    with pytest.raises(ValueError, match="sweep"):
        ekfac.compute_ekfac_scales(state, Z, model_type, _bases(state), None, None, moments="rows", curvature=spec)
    for call in (lambda **kw: posterior_lla_ekfac(state, Z, model_type, 1.0, **kw),
                 lambda **kw: predict_lla_ekfac(state, Z[:2], Z, model_type, 1.0, cov="diag", **kw),
                 lambda **kw: log_marginal_likelihood_ekfac(1.0, Z, state, model_type, **kw)):
        with pytest.raises(ValueError, match="sweep"):
            call(moments="rows", curvature=spec)


def test_unknown_moments_is_refused(no_binding):
    state, Z, model_type = kf.make_case("xor_classifier")
    for bad in ("row", "SWEEP", "", 1):
        with pytest.raises(ValueError, match="moments"):
            compute_ekfac_scales(state, Z, model_type, _bases(state), moments=bad)
        with pytest.raises(ValueError, match="moments"):
            posterior_lla_ekfac(state, Z, model_type, 1.0, moments=bad)


def test_spec_validation_comes_before_any_binding(no_binding):
    state, Z, model_type = kf.make_case("xor_classifier")
    M, K = Z.shape[0], state.net.num_outputs
    for bad in (fisher.EmpiricalFisher(torch.zeros(M + 1, dtype=torch.int64)), fisher.EmpiricalFisher(torch.full((M,), K)),
                fisher.Cotangents(torch.zeros(2, M + 1, K)), "fisher"):
        with pytest.raises(ValueError):
            compute_ekfac_scales(state, Z, model_type, _bases(state), moments="sweep", curvature=bad)


@pytest.mark.parametrize("name", kf.NETS)
def test_exact_expectation_cotangents_give_the_exact_scales(name):
    """sum_k u_ki u_ki^T = H_i for u_ki = sqrt(p_ik) (e_k - p_i) (the identity probes for a Gaussian head), so the raw
    definition of the sweep tests is the definition of tests/test_ekfac.py"""
    state, Z, model_type = kf.make_case(name)
    f, J, H = er.jacobian(state, Z, model_type)
    n, K = f.shape
    if model_type == "regressor":
        U = torch.eye(K, dtype=F64)[:, None, :].expand(K, n, K)
    else:
        U = fr.exact_expectation_cotangents(torch.softmax(f, dim=-1))
    g = torch.Generator().manual_seed(3)
    bases = [(torch.randn(Mt, Mt, dtype=F64, generator=g), torch.randn(N, N, dtype=F64, generator=g))
             for _, _, Mt, N, _, _ in kf.blocks_of(state)]
    want = er.scales_ref(J, H, state, bases)
    got = sr.scales_from_cotangents_ref(J, U, 1.0, state, bases)
    half = sr.scales_from_cotangents_ref(J, U, 2.0, state, bases)
    worst = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(got, want))
    print(f"{name}: raw definition against scales_ref {worst:.2e}")
    assert worst <= 1e-11
    assert max(((2.0 * a - b).abs().max() / b.abs().max()).item() for a, b in zip(half, want)) <= 1e-11


def test_fit_cache_key_distinguishes_moments_and_seeds():
    state, Z, model_type = kf.make_case("xor_classifier")
    key = lambda moments, curvature: ekfac._fit_key(state, Z, model_type, 1.0, None, None, moments, curvature)     # noqa: E731
    keys = [key("rows", None), key("sweep", None), key("sweep", fisher.MCFisher(3, 1)), key("sweep", fisher.MCFisher(3, 2)),
            key("sweep", fisher.MCFisher(4, 1)), key("sweep", fisher.EmpiricalFisher(torch.zeros(Z.shape[0], dtype=torch.int64)))]
    assert len(set(keys)) == len(keys)
    for k in keys:
        hash(k)
    assert key("sweep", fisher.MCFisher(3, 1)) == keys[2] and key("sweep", "ggn") == keys[1]
    # a spec without a route is the sweep, no spec the rows
    assert ekfac._route(None, fisher.MCFisher(1)) == "sweep" and ekfac._route(None, None) == "rows"
    assert ekfac._route("sweep", None) == "sweep"
