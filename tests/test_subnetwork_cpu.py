"""CPU checks of subnetwork Laplace: index validation, the ``"layers"`` selection against ``param_layout`` by hand, the
tie rule of the variance ranking, and the host algebra (posterior from a given G, evidence from a spectrum) on CPU
tensors against dense float64 formulas.  Everything here is float64 on the host: the bound 1e-10 * max|ref| leaves
decades over the rounding of a solve of condition <= 1001."""
import pytest
import torch

import subnetwork_ref as ref
from lip_amd import _native as nv
from lip_amd import subnetwork as sn
from lip_amd.prior import GroupedPrior
from lip_amd.scalemodels import ResNet1M
from lip_amd.toymodels import SimpleClassifier, create_state
from lip_amd.utils import flatten_nn_params, param_layout

F64 = torch.float64
TOL = 1e-10


def _state():
    return create_state(SimpleClassifier(16, 2, 2), 3, dtype=F64)


def _dim(state):
    return flatten_nn_params(state.params)[0].numel()


def test_library_exports_the_four_symbols():
    lib = nv.load()
    for name in ("lip_sub_gram", "lip_sub_gram_scratch", "lip_sub_predict", "lip_sub_predict_scratch", "lip_sub_gather"):
        assert hasattr(lib, name) and name in nv.SIGNATURES


def test_explicit_indices_are_validated_and_sorted():
    state = _state()
    D = _dim(state)
    got = sn.subnetwork_indices(state, [5, 0, D - 1, 3])
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == [0, 3, 5, D - 1]
    assert sn.subnetwork_indices(state, torch.tensor([7, 2], dtype=torch.int32)).tolist() == [2, 7]
    with pytest.raises(ValueError, match="distinct"):
        sn.subnetwork_indices(state, [1, 2, 1])
    with pytest.raises(ValueError, match=r"lie in \[0"):
        sn.subnetwork_indices(state, [0, D])
    with pytest.raises(ValueError, match=r"lie in \[0"):
        sn.subnetwork_indices(state, [-1, 2])
    with pytest.raises(ValueError, match="empty"):
        sn.subnetwork_indices(state, [])
    with pytest.raises(ValueError, match="integers"):
        sn.subnetwork_indices(state, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="select must be"):
        sn.subnetwork_indices(state, "everything")


def test_more_than_the_cap_is_refused():
    state = _state()
    assert sn.SUBNETWORK_MAX_DIM == 8192
    with pytest.raises(ValueError, match="SUBNETWORK_MAX_DIM"):
        sn.subnetwork_indices(state, torch.arange(sn.SUBNETWORK_MAX_DIM + 1))
    with pytest.raises(ValueError, match="SUBNETWORK_MAX_DIM"):
        sn.subnetwork_indices(state, "largest_variance", sn.SUBNETWORK_MAX_DIM + 1, Z=torch.zeros(1, 2), model_type="classifier",
                              alpha=1.0)
    # a 'layers' selection over the cap: 101 * 100 parameters in the final Dense
    from lip_amd.netspec import NetSpec
    net = NetSpec((6,))
    net.dense(net.dense(0, "Dense_0", 100, act="relu"), "Dense_1", 100)
    big = create_state(net, 0, dtype=F64)
    with pytest.raises(ValueError, match="SUBNETWORK_MAX_DIM"):
        sn.subnetwork_indices(big, "layers", [("params", "Dense_1")])


def test_layers_selection_against_param_layout_by_hand():
    state = create_state(ResNet1M(4, (8, 8, 3), (4, 8, 12), 2), 3, dtype=F64)
    bn = ("params", "BasicBlock_2", "BatchNorm_0")
    conv = ("params", "BasicBlock_2", "Conv_2", "kernel")
    want = ref.layers_by_hand(state, {bn + ("bias",), bn + ("scale",), conv})
    assert want.numel() == 8 + 8 + 1 * 1 * 4 * 8
    for spec in ([bn, conv], ["params/BasicBlock_2/BatchNorm_0", "params/BasicBlock_2/Conv_2/kernel"],
                 lambda path: tuple(path[:3]) == bn or tuple(path) == conv):
        got = sn.subnetwork_indices(state, "layers", spec)
        assert got.dtype == torch.int64 and torch.equal(got, want)
    # a string prefix ends at a path component: BatchNorm_1 is no prefix match of BatchNorm_10 and the like
    lay = {"/".join(p): (o, s) for p, o, s in param_layout(state.params)}
    one = sn.subnetwork_indices(state, "layers", ["params/BasicBlock_2/BatchNorm_1/scale"])
    o, s = lay["params/BasicBlock_2/BatchNorm_1/scale"]
    assert one.tolist() == list(range(o, o + s[0]))
    with pytest.raises(ValueError, match="matches no parameter"):
        sn.subnetwork_indices(state, "layers", ["params/BasicBlock_2/BatchNorm"])
    with pytest.raises(ValueError, match="prefixes"):
        sn.subnetwork_indices(state, "layers")


def test_variance_ranking_breaks_ties_by_the_lower_index():
    diag = torch.tensor([3.0, 1.0, 1.0, 0.5, 1.0, 3.0, 0.5], dtype=F64)
    a = torch.full((7,), 0.25, dtype=F64)
    for size in range(1, 8):
        want, _ = ref.top_variances_ref(diag, a, size)
        assert torch.equal(sn.top_variances(diag, a, size), want), size
    assert sn.top_variances(diag, a, 3).tolist() == [1, 3, 6]         # 3 and 6 tie at the top; of 1, 2, 4 the lowest
    a2 = torch.tensor([0.25, 0.25, 0.25, 0.75, 0.25, 0.25, 0.25], dtype=F64)    # a vector prior moves 3 into the tie of 1, 2, 4
    assert sn.top_variances(diag, a2, 2).tolist() == [1, 6]


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
def test_posterior_from_a_given_g_matches_the_dense_formula(grouped):
    state = _state()
    flat, _ = flatten_nn_params(state.params)
    D = flat.numel()
    g = torch.Generator().manual_seed(0)
    idx = sn.check_indices(torch.randperm(D, generator=g)[:23], D)
    R = torch.randn(40, 23, dtype=F64, generator=g)
    G = R.T @ R
    alpha = 1e-3 * float(torch.linalg.eigvalsh(G).max())
    if grouped:
        prior = GroupedPrior(state.params, [alpha * (1 + i) for i in range(len({p[:-1] for p, _, _ in param_layout(state.params)}))],
                             "layer")
        a = prior.vector("cpu", F64)[idx]
        assert len(set(a.tolist())) > 1                                # the set straddles groups
    else:
        prior, a = alpha, torch.full((23,), alpha, dtype=F64)
    post = sn.posterior_from_ggn(G, prior, idx, flat)
    want = torch.linalg.inv(G + torch.diag(a))
    assert post.mean().dtype == F64 and torch.equal(post.mean(), flat[idx].double())
    assert (post.covariance() - want).abs().max() <= TOL * want.abs().max()
    assert (post.covariance() - ref.covariance_ref(G, a)).abs().max() <= TOL * want.abs().max()


def test_evidence_from_a_spectrum_matches_its_restatement():
    from lip_amd.train_alpha import _fit_from_spectrum, _lml_from_spectrum
    g = torch.Generator().manual_seed(1)
    R = torch.randn(30, 11, dtype=F64, generator=g)
    lam = torch.linalg.eigvalsh(R.T @ R).clamp_min(0.0)
    alpha = 1e-3 * float(lam.max())
    got = _lml_from_spectrum(alpha, lam, 11, 2.5, 40 / 30)[0]
    want = ref.lml_ref(alpha, lam, 11, 2.5, 40 / 30)
    assert abs(got - want) <= 1e-12 * abs(want)
    # the dense restatement: -1/2 alpha ||theta||^2 - 1/2 logdet(I + r G / alpha)
    dense = -0.5 * alpha * 2.5 - 0.5 * float(torch.logdet(torch.eye(11, dtype=F64) + (40 / 30) * (R.T @ R) / alpha))
    assert abs(got - dense) <= TOL * abs(dense)
    a_fit, hist = _fit_from_spectrum(lam, 11, 2.5, 40 / 30, alpha, 5e-2, 3)
    assert len(hist) == 3 and hist[0] == (pytest.approx(alpha, rel=1e-14), pytest.approx(want, rel=1e-12)) and a_fit > 0


def test_surface_is_re_exported():
    from lip_amd import ggn, lla, train_alpha
    assert lla.predict_lla_subnetwork is sn.predict_lla_subnetwork
    assert lla.posterior_lla_subnetwork is sn.posterior_lla_subnetwork
    assert lla.predict_lla_subnetwork_scalable is sn.predict_lla_subnetwork_scalable
    assert lla.SUBNETWORK_MAX_DIM == 8192 and lla.subnetwork_indices is sn.subnetwork_indices
    assert callable(ggn.compute_ggn_subnetwork) and callable(ggn.subnetwork_indices)
    assert callable(train_alpha.fit_alpha_subnetwork) and callable(train_alpha.log_marginal_likelihood_subnetwork)
