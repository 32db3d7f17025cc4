"""CPU checks of the row-free Kronecker-factored predictive: the identity the GPU tests rely on
(``tests/kfac_predict_sweep_ref.py``, which never forms a Jacobian, equals ``kfac_ref.predict_dense`` on the autograd
Jacobian), and the ``route=`` keyword of the public surface, whose refusals come before anything is bound."""
import inspect

import pytest
import torch

import kfac_predict_sweep_ref as pr
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import ekfac, kfac
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.lla import predict_lla_ekfac, predict_lla_kfac

F64 = torch.float64
IDENTITY_NETS = ["sine_regressor", "xor_classifier", "mlp_ragged", "resnet_tiny", "stem_net"]
IDENTITY_TOL = 1e-12             # float64 products of at most a few thousand terms, regrouped


@pytest.mark.parametrize("name", IDENTITY_NETS)
def test_projected_products_give_the_dense_predictive(name):
    """sum_{j,m} R ((At V)^T (G Ub))^2 = J_l (V (x) Ub) diag(R) (V (x) Ub)^T J_l^T: the bias row, the frozen BN scale and
    every window geometry included (the nets cover Dense, SAME 3x3, stride 2, 1x1, the 7x7 stem)"""
    state, Z, model_type = kf.make_case(name)
    X = Z[:3]
    _, J = ref.jac64(state, X, model_type)
    g = torch.Generator().manual_seed(17)
    triples, cov_blocks = [], []
    for _, off, Mt, N, _, _ in kf.blocks_of(state):
        V = torch.randn(Mt, Mt, dtype=F64, generator=g) / Mt ** 0.5
        Ub = torch.randn(N, N, dtype=F64, generator=g) / N ** 0.5
        R = torch.rand(Mt, N, dtype=F64, generator=g) + 0.25
        triples.append((V, R, Ub))
        W = torch.kron(V, Ub)
        cov_blocks.append((off, (W * R.reshape(-1)[None, :]) @ W.T))
    rem = kf.remainder_of(state)
    rem_var = torch.rand(rem.numel(), dtype=F64, generator=g) + 0.25
    want = kf.predict_dense(J, cov_blocks, rem, rem_var)
    got = pr.predict_ref(state, X, triples, J, rem, rem_var)
    e = ((got - want).abs().max() / want.abs().max()).item()
    # the one-hot form of the helper is the diagonal, and raw probes are linear in the cotangents
    K = J.shape[1]
    var = sum(pr.block_terms(state, X, triples)).T + torch.diagonal(pr.remainder_covariance(J, rem, rem_var), dim1=1, dim2=2)
    e_diag = ((var - torch.diagonal(want, dim1=1, dim2=2)).abs().max() / want.abs().max()).item()
    U = torch.randn(2, 3, K, dtype=F64, generator=g)
    quad = sum(pr.block_terms(state, X, triples, U))
    blocks_only = kf.predict_dense(J, cov_blocks, rem, torch.zeros_like(rem_var))
    e_quad = ((quad - torch.einsum("pik,ikm,pim->pi", U, blocks_only, U)).abs().max() / want.abs().max()).item()
    print(f"{name}: helper against predict_dense {e:.2e}  diagonal {e_diag:.2e}  raw probes {e_quad:.2e}")
    assert max(e, e_diag, e_quad) <= IDENTITY_TOL


@pytest.fixture
def no_binding(monkeypatch):
    """any attempt to bind an engine, or to fit, fails the test: the refusals below come first"""
    def refuse(*a, **kw):
        raise AssertionError("an engine was bound before the arguments were checked")
    monkeypatch.setattr(kfac._ggn, "get_engine", refuse)
    monkeypatch.setattr(kfac, "_engines", refuse)
    monkeypatch.setattr(ekfac, "_engines", refuse)


def test_unknown_route_is_refused_before_any_binding(no_binding):
    state, Z, model_type = kf.make_case("xor_classifier")
    for bad in ("bogus", "row", "SWEEP", "", 1):
        with pytest.raises(ValueError, match="route"):
            kfac.predictive_from_fit(state, Z[:2], model_type, [], (torch.zeros(0), torch.zeros(0)), "diag", 2, route=bad)
        with pytest.raises(ValueError, match="route"):
            predict_lla_kfac(state, Z[:2], Z, model_type, 1.0, cov="diag", route=bad)
        with pytest.raises(ValueError, match="route"):
            predict_lla_ekfac(state, Z[:2], Z, model_type, 1.0, cov="diag", route=bad)


def test_route_is_keyword_only_and_defaults_to_the_rows_route():
    for fn in (predict_lla_kfac, predict_lla_ekfac, eval_dataset_probit):
        p = inspect.signature(fn).parameters["route"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert inspect.signature(kfac.predictive_from_fit).parameters["route"].default == "rows"
    assert kfac.checked_route(None) == "rows" and kfac.route_kwargs(None) == {} and kfac.route_kwargs("rows") == {}
    assert kfac.route_kwargs("sweep") == {"route": "sweep"}


def test_other_posteriors_refuse_a_route(no_binding):
    state, Z, model_type = kf.make_case("xor_classifier")
    y = torch.zeros(Z.shape[0], dtype=torch.int64)
    for posterior in ("diag", "inducing", "last_layer", "last_layer_kron", "lowrank", "subnetwork"):
        with pytest.raises(ValueError, match="route"):
            eval_dataset_probit(state, [(Z, y)], Z, 1.0, None, model_type, posterior=posterior, route="sweep")
    with pytest.raises(ValueError, match="route"):
        eval_dataset_probit(state, [(Z, y)], Z, 1.0, None, model_type, posterior="kfac", route="bogus")


def test_full_covariance_on_the_sweep_route_is_refused_beyond_32_outputs(no_binding):
    class Wide:
        num_outputs = 33

    class State:
        net = Wide()
        params = {}
    with pytest.raises(ValueError, match="33"):
        kfac.predictive_from_fit(State(), torch.zeros(2, 3), "classifier", [], (torch.zeros(0), torch.zeros(0)), "full", 2,
                                 route="sweep")
