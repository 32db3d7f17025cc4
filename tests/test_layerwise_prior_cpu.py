"""CPU checks of the layer-wise prior: the group table of ``GroupedPrior`` and the float64 evidence algebra of
``train_alpha.lml_layerwise`` / ``fit_log_alphas`` against dense float64 expressions and the scalar code.  No engine,
no GPU: the Grams are those of random float64 factors."""
import math

import pytest
import torch

from lip_amd.prior import GroupedPrior
from lip_amd.scalemodels import LargeClassifier, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from lip_amd.train_alpha import Adam, _lml_from_spectrum, fit_log_alphas, lml_layerwise
from lip_amd.utils import flatten_nn_params, param_layout

F64 = torch.float64


def _nets():
    return {
        "sine_regressor": SimpleRegressor(8, 4),
        "xor_classifier": SimpleClassifier(16, 2, 2),
        "mlp_ragged": LargeClassifier((6, 6, 1), [40, 24], 2, 5),
        "resnet50_tiny": ResNet50(6, input_shape=(20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
        "resnet1m": ResNet1M(10),
    }


def _values(G, seed):
    """per-group precisions, log-uniform in [0.05, 20]"""
    u = torch.rand(G, dtype=F64, generator=torch.Generator().manual_seed(seed))
    return torch.exp(math.log(0.05) + u * (math.log(20.0) - math.log(0.05)))


def _states():
    return {k: create_state(net, 3, dtype=torch.float32) for k, net in _nets().items()}


STATES = _states()


@pytest.mark.parametrize("groups", ["tensor", "layer"])
@pytest.mark.parametrize("name", list(STATES))
def test_table_covers_the_flat_vector_exactly_once(name, groups):
    params = STATES[name].params
    flat, _ = flatten_nn_params(params)
    D = flat.numel()
    G0 = GroupedPrior(params, 1.0, groups).G
    prior = GroupedPrior(params, _values(G0, 1), groups)
    assert prior.D == D and prior.G == G0 == len(prior.names) == len(set(prior.names))
    hits = torch.zeros(D, dtype=torch.int64)
    for g in range(prior.G):
        for o, n in prior.segments(g):
            assert n > 0 and 0 <= o and o + n <= D
            hits[o:o + n] += 1
    assert bool((hits == 1).all())
    assert int(prior.sizes.sum()) == D
    assert [int(s) for s in prior.sizes] == [sum(n for _, n in prior.segments(g)) for g in range(prior.G)]
    if groups == "tensor":
        assert prior.G == len(param_layout(params))
    # the expanded vector agrees with the table, on both dtypes, and is cached
    a = prior.vector("cpu", F64)
    for g in range(prior.G):
        for o, n in prior.segments(g):
            assert bool((a[o:o + n] == prior.values[g]).all())
    assert prior.vector("cpu").dtype == torch.float32 and torch.equal(prior.vector("cpu"), a.float())
    assert prior.vector("cpu") is prior.vector("cpu")
    # group square norms against the flat vector
    ref = torch.stack([sum((flat[o:o + n].double() ** 2).sum() for o, n in prior.segments(g)) for g in range(prior.G)])
    assert torch.allclose(prior.group_sqnorms(flat), ref, rtol=1e-14, atol=0)
    assert abs(float(prior.group_sqnorms(flat).sum()) - float((flat.double() ** 2).sum())) <= 1e-12 * float((flat.double() ** 2).sum())


def test_one_element_groups_exist_on_the_regressor():
    prior = GroupedPrior(STATES["sine_regressor"].params, 1.0, "tensor")
    assert 1 in prior.sizes.tolist()


def test_layer_grouping_joins_a_kernel_and_its_bias():
    params = STATES["xor_classifier"].params
    prior = GroupedPrior(params, 1.0, "layer")
    layout = {path: (off, math.prod(shape)) for path, off, shape in param_layout(params)}
    for layer in ("Dense_0", "Dense_1", "Dense_2"):
        g = prior.names.index(f"params/{layer}")
        covered = set()
        for o, n in prior.segments(g):
            covered |= set(range(o, o + n))
        for leaf in ("kernel", "bias"):
            off, n = layout[("params", layer, leaf)]
            assert set(range(off, off + n)) <= covered
        assert len(covered) == sum(layout[("params", layer, leaf)][1] for leaf in ("kernel", "bias"))
    # a BN scale and its bias
    rp = GroupedPrior(STATES["resnet50_tiny"].params, 1.0, "layer")
    g = rp.names.index("params/BatchNorm_0")
    assert int(rp.sizes[g]) == 16 and rp.segments(g) == [(0, 16)]


def test_callable_and_explicit_groupings():
    params = STATES["mlp_ragged"].params
    prior = GroupedPrior(params, [2.0, 0.5], lambda path: path[-1] == "bias")
    assert prior.G == 2
    biases = prior.names.index("True")
    assert len(prior.segments(biases)) == 3                          # non-contiguous: one segment per layer
    assert prior.segments(biases) == [(0, 40), (1480, 24), (2464, 5)]
    assert int(prior.sizes[biases]) == 69
    a = prior.vector("cpu", F64)
    assert float(a[0]) == float(prior.values[biases]) and float(a[40]) == float(prior.values[1 - biases])
    explicit = GroupedPrior(params, [1.0, 2.0, 3.0], [0, 1, 0, 1, 2, 2])
    assert explicit.G == 3 and explicit.sizes.tolist() == [40 + 24, 1440 + 960, 125]
    same = explicit.with_values([3.0, 2.0, 1.0])
    assert same.table == explicit.table and same.values.tolist() == [3.0, 2.0, 1.0]
    assert same.key() != explicit.key() and explicit.key() == explicit.with_values([1.0, 2.0, 3.0]).key()


@pytest.mark.parametrize("bad", [[1.0, 0.0, 2.0], [1.0, -1.0, 2.0], [1.0, float("nan"), 2.0], [1.0, float("inf"), 2.0],
                                 [1.0, 2.0]])
def test_bad_values_are_refused(bad):
    with pytest.raises(ValueError):
        GroupedPrior(STATES["xor_classifier"].params, bad, "layer")


@pytest.mark.parametrize("table", [
    [("a", [(0, 4)]), ("b", [(5, 5)])],                              # gap
    [("a", [(0, 5)]), ("b", [(4, 6)])],                              # overlap
    [("a", [(0, 5)]), ("b", [(5, 4)])],                              # short
    [("a", [(0, 5)]), ("b", [(5, 6)])],                              # long
    [("a", [(0, 10)]), ("b", [])],                                   # empty group
    [("a", [(0, 10)]), ("b", [(3, 0)])],                             # empty segment
])
def test_bad_tables_are_refused(table):
    with pytest.raises(ValueError):
        GroupedPrior.from_table(table, [1.0, 2.0], 10)


def test_bad_groupings_are_refused():
    params = STATES["xor_classifier"].params
    with pytest.raises(ValueError):
        GroupedPrior(params, 1.0, "block")
    with pytest.raises(ValueError):
        GroupedPrior(params, 1.0, [0, 1, 2])                         # six leaves
    with pytest.raises(ValueError):
        GroupedPrior(params, 1.0, [0, 0, 2, 2, 3, 3])                # index 1 unused


# ---- the evidence algebra: d = 7, D = 23, G = 4 with a group of one parameter and a non-contiguous group
D_, d_ = 23, 7
TABLE = [("a", [(0, 9)]), ("one", [(9, 1)]), ("split", [(10, 4), (20, 3)]), ("b", [(14, 6)])]


def _factor():
    g = torch.Generator().manual_seed(5)
    Wm = torch.randn(d_, D_, dtype=F64, generator=g)
    theta = torch.randn(D_, dtype=F64, generator=g)
    return Wm, theta


def _grams(Wm, prior):
    out = []
    for g in range(prior.G):
        cols = torch.cat([Wm[:, o:o + n] for o, n in prior.segments(g)], 1)
        out.append(cols @ cols.T)
    return torch.stack(out)


def _dense_value(log_alphas, prior, Wm, theta, r):
    """-1/2 theta^T A theta - 1/2 (slogdet(A + r W W^T) - sum_g D_g log alpha_g), differentiable in log_alphas"""
    a = torch.zeros(D_, dtype=F64)
    for g in range(prior.G):
        for o, n in prior.segments(g):
            a = a + torch.nn.functional.pad(torch.ones(n, dtype=F64), (o, D_ - o - n)) * torch.exp(log_alphas[g])
    logdet = torch.linalg.slogdet(torch.diag(a) + r * Wm.T @ Wm)[1]
    return -0.5 * (a * theta ** 2).sum() - 0.5 * (logdet - (prior.sizes.double() * log_alphas).sum())


@pytest.mark.parametrize("r", [1.0, 37.5])
def test_lml_layerwise_matches_the_dense_determinant_and_autograd(r):
    Wm, theta = _factor()
    prior = GroupedPrior.from_table(TABLE, _values(4, 2), D_)
    grams, t2 = _grams(Wm, prior), prior.group_sqnorms(theta)
    la = torch.log(prior.values).clone().requires_grad_(True)
    ref = _dense_value(la, prior, Wm, theta, r)
    ref_grad, = torch.autograd.grad(ref, la)
    ref = ref.detach()
    v, g = lml_layerwise(la.detach(), grams, t2, r)
    assert isinstance(v, float) and g.shape == (4,) and g.dtype == F64
    assert abs(v - float(ref)) <= 1e-12 * abs(float(ref)), (v, float(ref))
    assert float((g - ref_grad).abs().max()) <= 1e-10 * max(1.0, float(ref_grad.abs().max())), (g, ref_grad)
    # a precision per group matters: the mean precision gives another value
    v_mean, _ = lml_layerwise(torch.log(prior.values.mean()).repeat(4), grams, t2, r)
    assert abs(v_mean - v) > 1e-3 * abs(v)


@pytest.mark.parametrize("alpha", [0.05, 1.0, 7.0])
def test_one_group_is_the_scalar_formula(alpha):
    Wm, theta = _factor()
    G = Wm @ Wm.T
    lam = torch.linalg.eigvalsh(G).clamp_min(0.0)
    theta2 = float((theta ** 2).sum())
    r = 12.5
    v0, g0 = _lml_from_spectrum(alpha, lam, D_, theta2, r)
    v, g = lml_layerwise([math.log(alpha)], G[None], torch.tensor([theta2], dtype=F64), r)
    assert abs(v - v0) <= 1e-12 * abs(v0)
    assert abs(float(g[0]) - g0) <= 1e-12 * max(1.0, abs(g0))


def test_one_group_walks_the_trajectory_of_fit_alpha():
    """the loop of ``fit_alpha`` on the spectrum (scalar ``Adam``) against ``fit_log_alphas`` with G = 1"""
    Wm, theta = _factor()
    G = Wm @ Wm.T
    lam = torch.linalg.eigvalsh(G).clamp_min(0.0)
    theta2 = float((theta ** 2).sum())
    r, lr, steps = 12.5, 5e-2, 120
    opt = Adam(lr)
    st, la, hist0 = opt.init(), math.log(1.0), []
    for _ in range(steps):
        v, g = _lml_from_spectrum(math.exp(la), lam, D_, theta2, r)
        hist0.append((math.exp(la), v))
        upd, st = opt.update(-g, st)
        la += upd
    la1, hist1 = fit_log_alphas(G[None], torch.tensor([theta2], dtype=F64), r, [0.0], lr, steps)
    assert len(hist1) == steps
    for (a0, v0), (a1, v1) in zip(hist0, hist1):
        assert abs(float(a1[0]) - a0) <= 1e-12 * a0 and abs(v1 - v0) <= 1e-12 * abs(v0)
    assert abs(float(la1[0]) - la) <= 1e-12 * max(1.0, abs(la))
    assert hist1[-1][1] > hist1[0][1]


def test_layerwise_fit_increases_the_evidence_beyond_the_shared_precision():
    Wm, theta = _factor()
    prior = GroupedPrior.from_table(TABLE, 1.0, D_)
    grams, t2 = _grams(Wm, prior), prior.group_sqnorms(theta)
    la, hist = fit_log_alphas(grams, t2, 12.5, torch.zeros(4, dtype=F64), 5e-2, 300)
    la1, hist1 = fit_log_alphas(grams.sum(0)[None], t2.sum()[None], 12.5, [0.0], 5e-2, 300)
    v = lml_layerwise(la, grams, t2, 12.5)[0]
    v1 = lml_layerwise(la1, grams.sum(0)[None], t2.sum()[None], 12.5)[0]
    assert v > hist[0][1] and v > v1
    assert hist[0][0].shape == (4,) and hist[0][0].dtype == F64
