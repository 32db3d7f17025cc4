"""CPU checks of the layer-wise evidence of the diagonal, KFAC and EKFAC posteriors (``evidence.py``): the host algebra
on CPU tensors, fed the float64 helpers' factors (``tests/kfac_ref.py``, ``tests/ekfac_ref.py``), against dense algebra;
the gradient against central differences; the reduction to the scalar evidence; the refusals, which return before
anything is bound; and the chunk table.

Everything is float64 on the host.  The "layer" prior of these tests has the group values alpha_for x (1, 2, 4, 8, 1, ..):
every value is at least alpha_for = 1e-3 max_l c_l lam_max(A_l) mu_max(S_l) and constant on a block, so the condition of
every block's dense precision is at most 1 + 1000 (asserted inside ``kf.covariance_blocks``, and here for the EKFAC
blocks), and a float64 ``eigvalsh`` of blocks of order ~1e3 at that condition supports rtol 1e-10 on the value.
"""
import functools
import math

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import evidence as ev
from lip_amd import kfac, train_alpha
from lip_amd.prior import GroupedPrior
from lip_amd.train_alpha import _fit_from_spectrum, _lml_from_spectrum
from lip_amd.utils import flatten_nn_params

F64 = torch.float64
N_FULL = kf.N_FULL
VALUE_RTOL = 1e-10


@functools.lru_cache(maxsize=None)
def _helper(name):
    """the float64 helper's curvature of a net, built once and never written to"""
    state, Z, model_type = kf.make_case(name)
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    flat = flatten_nn_params(state.params)[0].detach().double()
    _, J, H = er.jacobian(state, Z, model_type)
    bases = er.orthonormal_bases(state, As, Ss, model_type)
    return dict(state=state, Z=Z, model_type=model_type, As=As, Ss=Ss, M=M, alpha=alpha, flat=flat, D=flat.numel(),
                diag1=kf.ggn_diag_ref(state, Z, model_type, None), table=kfac.block_table(state), bases=bases,
                Lams0=er.scales_ref(J, H, state, bases), rescale=N_FULL / M,
                scale=math.exp(-float(state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0)


def _layer_prior(h, equal=False):
    G = GroupedPrior(h["state"].params, 1.0, "layer").G
    values = [h["alpha"] * (1.0 if equal else 2.0 ** (g % 4)) for g in range(G)]
    return GroupedPrior(h["state"].params, values, "layer")


def _plan(h, which, prior):
    if which == "diag":
        return ev.plan_from_diag(h["diag1"], prior, h["flat"])
    if which == "kfac":
        return ev.plan_from_kfac(h["table"], h["As"], h["Ss"], h["M"], h["model_type"] != "regressor", h["scale"], prior,
                                 h["flat"], h["diag1"])
    return ev.plan_from_ekfac(h["table"], h["Lams0"], h["scale"], prior, h["flat"], h["diag1"])


def _value(h, which, prior):
    return ev.lml_structured(torch.log(prior.values), _plan(h, which, prior), h["rescale"])[0]


def _prior_term(h, prior):
    return -0.5 * float((prior.vector("cpu", F64) * h["flat"] ** 2).sum())


def _remainder_logdet(h, a):
    rem = kf.remainder_of(h["state"])
    return float(torch.log1p(h["rescale"] * h["diag1"][rem] / a[rem]).sum())


@pytest.mark.parametrize("name", kf.NETS)
def test_layerwise_values_match_dense_algebra(name):
    h = _helper(name)
    state, model_type, M = h["state"], h["model_type"], h["M"]
    prior = _layer_prior(h)
    assert float(prior.values.min()) >= h["alpha"] and prior.G > 1
    a = prior.vector("cpu", F64)
    # KFAC: the helper's dense blocks c_l kron(A_l, S_l) + diag(a); it asserts the condition <= 1002 of every solve
    _, logdet = kf.covariance_blocks(state, h["As"], h["Ss"], M, model_type, a, N_FULL)
    want = _prior_term(h, prior) - 0.5 * (logdet + _remainder_logdet(h, a))
    got = _value(h, "kfac", prior)
    e_kfac = abs(got - want) / abs(want)
    # EKFAC: the helper's dense covariance (V (x) Ub) diag(1 / (recal Lam + 1)) (V (x) Ub)^T with V = U_A / sqrt(a_l),
    # Lam = Lam0 / a_l, the fit of a prior that is constant on the block
    recal = ref.recal(state, M, model_type, N_FULL)
    a_blocks = [float(a[b.off]) for b in h["table"]]
    bases = [(U / math.sqrt(al), Ub) for (U, Ub), al in zip(h["bases"], a_blocks)]
    Lams = [Lam / al for Lam, al in zip(h["Lams0"], a_blocks)]
    logdet = 0.0
    for (off, S), al in zip(er.covariance_blocks(state, bases, Lams, recal), a_blocks):
        lam = torch.linalg.eigvalsh(0.5 * (S + S.T))
        assert float(lam.max() / lam.min()) <= 1002.0 * (1 + 1e-12)
        logdet += float(-torch.log(lam).sum()) - S.shape[0] * math.log(al)
    want_e = _prior_term(h, prior) - 0.5 * (logdet + _remainder_logdet(h, a))
    got_e = _value(h, "ekfac", prior)
    e_ekfac = abs(got_e - want_e) / abs(want_e)
    # diagonal: the helper's exact GGN diagonal at N
    diag_n = kf.ggn_diag_ref(state, h["Z"], model_type, N_FULL)
    want_d = _prior_term(h, prior) - 0.5 * float(torch.log1p(diag_n / a).sum())
    got_d = _value(h, "diag", prior)
    e_diag = abs(got_d - want_d) / abs(want_d)
    print(f"{name}: G = {prior.G}  kfac {got:.12g} ({e_kfac:.2e})  ekfac {got_e:.12g} ({e_ekfac:.2e})  diag {got_d:.12g} ({e_diag:.2e})")
    assert max(e_kfac, e_ekfac, e_diag) <= VALUE_RTOL


@pytest.mark.parametrize("which", ["diag", "kfac", "ekfac"])
@pytest.mark.parametrize("name", kf.NETS)
def test_gradient_matches_central_differences(name, which):
    h = _helper(name)
    prior = _layer_prior(h)
    plan = _plan(h, which, prior)
    la = torch.log(prior.values)
    _, grad = ev.lml_structured(la, plan, h["rescale"])
    assert grad.shape == (prior.G,) and grad.dtype == F64
    step, worst = 1e-5, 0.0
    for g in range(prior.G):
        e = torch.zeros_like(la)
        e[g] = step
        fd = (ev.lml_structured(la + e, plan, h["rescale"])[0] - ev.lml_structured(la - e, plan, h["rescale"])[0]) / (2 * step)
        worst = max(worst, abs(fd - float(grad[g])) / abs(float(grad[g])))
    print(f"{name} {which}: worst relative difference to central differences {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("name", kf.NETS)
def test_equal_groups_reduce_to_the_scalar_evidence(name):
    h = _helper(name)
    prior = _layer_prior(h, equal=True)
    theta2 = float((h["flat"] ** 2).sum())
    specs = {"kfac": kf.spectrum_ref(h["state"], h["As"], h["Ss"], h["M"], h["model_type"], h["diag1"]),
             "ekfac": er.spectrum_ref(h["state"], h["Lams0"], h["model_type"], h["diag1"]),
             "diag": h["diag1"].clamp_min(0.0)}
    for which, spec in specs.items():
        assert spec.numel() == h["D"]
        want = _lml_from_spectrum(h["alpha"], spec, h["D"], theta2, h["rescale"])[0]
        got = _value(h, which, prior)
        assert int(_plan(h, which, prior).terms_per_group.sum()) == h["D"]
        print(f"{name} {which}: {got:.15g} against {want:.15g}")
        assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("which", ["diag", "kfac", "ekfac"])
def test_one_group_walks_the_scalar_fit(which):
    h = _helper("resnet_tiny")
    prior = GroupedPrior(h["state"].params, 3.0 * h["alpha"], lambda path: "all")
    assert prior.G == 1
    plan = _plan(h, which, prior)
    spec = {"kfac": kf.spectrum_ref(h["state"], h["As"], h["Ss"], h["M"], h["model_type"], h["diag1"]),
            "ekfac": er.spectrum_ref(h["state"], h["Lams0"], h["model_type"], h["diag1"]),
            "diag": h["diag1"].clamp_min(0.0)}[which]
    a_ref, hist_ref = _fit_from_spectrum(spec, h["D"], float((h["flat"] ** 2).sum()), h["rescale"], 3.0 * h["alpha"], 5e-2, 20)
    la, hist = ev.fit_log_alphas_structured(plan, h["rescale"], torch.log(prior.values), 5e-2, 20)
    assert len(hist) == len(hist_ref) == 20 and la.shape == (1,)
    for (a, v), (ar, vr) in zip(hist, hist_ref):
        assert a.shape == (1,) and a.dtype == F64 and not a.is_cuda and isinstance(v, float)
        assert abs(float(a) - ar) <= 1e-10 * ar and abs(v - vr) <= 1e-10 * abs(vr)
    assert abs(math.exp(float(la)) - a_ref) <= 1e-10 * a_ref
    assert a_ref != 3.0 * h["alpha"]                                     # the walk moved


def test_a_prior_that_cuts_a_block_is_refused_before_anything_is_bound():
    h = _helper("xor_classifier")                                         # Dense layers with a bias each
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    tensor = GroupedPrior(state.params, 1.0, "tensor")                    # equal values: the table decides, not the values
    first = h["table"][0]
    name = "/".join(map(str, first.unit.kernel[:-1]))
    for build in (lambda: _plan(h, "kfac", tensor), lambda: _plan(h, "ekfac", tensor),
                  lambda: ev.plan_kfac(state, Z, model_type, tensor), lambda: ev.plan_ekfac(state, Z, model_type, tensor),
                  lambda: train_alpha.log_marginal_likelihood_kfac_layerwise(tensor, Z, state, model_type),
                  lambda: train_alpha.log_marginal_likelihood_ekfac_layerwise(tensor, Z, state, model_type),
                  lambda: train_alpha.fit_alpha_kfac_layerwise(Z, state, model_type, groups="tensor", steps=2),
                  lambda: train_alpha.fit_alpha_ekfac_layerwise(Z, state, model_type, groups="tensor", steps=2)):
        with pytest.raises(ValueError, match=f"block of {name} at flat offset {first.off} lies in the prior groups") as err:
            build()                                                       # no GPU here: nothing was bound
        assert all(repr(n) in str(err.value) for n in tensor.names[:2])
    plan = _plan(h, "diag", tensor)                                       # any grouping suits the diagonal posterior
    assert plan.G == tensor.G and int(plan.terms_per_group.sum()) == h["D"]
    assert ev.block_groups(_layer_prior(h), h["table"], h["D"]) == list(range(len(h["table"])))
    # a net without biases: "tensor" groups are whole blocks
    r = _helper("resnet_tiny")
    t2 = GroupedPrior(r["state"].params, 1.0, "tensor")
    if all(not b.bias for b in r["table"]):
        assert len(ev.block_groups(t2, r["table"], r["D"])) == len(r["table"])
    # a prior of another net
    for which in ("diag", "kfac", "ekfac"):
        with pytest.raises(ValueError, match="the prior covers"):
            _plan(r, which, tensor)
    with pytest.raises(ValueError, match="the prior covers"):
        ev.plan_diag(r["state"], r["Z"], r["model_type"], tensor)
    with pytest.raises(ValueError, match="the prior covers"):
        ev.plan_kfac(r["state"], r["Z"], r["model_type"], tensor)


def test_chunk_table_covers_every_term_once():
    C = ev.CHUNK
    shapes = {C - 1: (217, 151), C: (256, 128), C + 1: (9, 3641)}         # rows x cols of the products
    assert all(r * c == n for n, (r, c) in shapes.items())
    segs, off = [], 0
    for n, (r, c) in shapes.items():
        segs.append(ev.Segment(ev.KRON, off, r, c, 1.0, 0))
        off += r + c
        segs.append(ev.Segment(ev.LIST, off, n, 1, 1.0, 1))
        off += n
    chunks = ev.chunk_table(segs)
    per_seg = [sum(1 for k, _ in chunks if k == i) for i in range(len(segs))]
    assert per_seg == [1, 1, 1, 1, 2, 2]
    for i, s in enumerate(segs):
        starts = [st for k, st in chunks if k == i]
        covered = torch.zeros(s.terms, dtype=torch.int64)
        for st in starts:
            covered[st:min(st + C, s.terms)] += 1
        assert bool((covered == 1).all())
    ptr, idx = ev.group_chunks(segs, chunks, 2)
    assert ptr == [0, 4, 8] and sorted(idx) == list(range(8))
    assert idx[:4] == sorted(idx[:4]) and all(segs[chunks[c][0]].group == 0 for c in idx[:4])     # chunk order inside a group
    plan = ev.EvidencePlan(torch.ones(off, dtype=F64), segs, torch.zeros(2), ["a", "b"])
    assert plan.chunks == chunks and plan.terms_per_group.tolist() == [3 * C, 3 * C]
    L, T = plan.terms(torch.zeros(2))
    assert torch.allclose(L, torch.full((2,), 3 * C * math.log(2.0), dtype=F64), rtol=1e-12)
    assert torch.allclose(T, torch.full((2,), 1.5 * C, dtype=F64), rtol=1e-12)
    for bad in ([(ev.KRON, 0, 0, 3, 1.0, 0)], [(ev.LIST, 0, 5, 1, 1.0, 2)], [(ev.LIST, off - 2, 3, 1, 1.0, 0)], [(7, 0, 1, 1, 1.0, 0)],
                [(ev.LIST, 0, 5, 1, float("nan"), 0)], []):
        with pytest.raises(ValueError):
            ev.EvidencePlan(torch.ones(off, dtype=F64), bad, torch.zeros(2), ["a", "b"])
