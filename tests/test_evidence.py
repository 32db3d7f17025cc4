"""GPU checks of the layer-wise evidence of the diagonal, KFAC and EKFAC posteriors: the kernel ``lip_evidence_terms``
through ``EvidencePlan.terms`` on synthetic pools against float64 torch on the CPU, its reproducibility, operands and
status codes, then the public functions of ``train_alpha.py`` on the nets of ``tests/kfac_ref.py`` against the float64
helpers' spectra, the fits, and a Fisher spec.

The kernel bound.  Every term is non-negative, so nothing cancels.  The kernel forms a term's argument as
(scale * (r / alpha_g)) * (max(lam_i, 0) * max(mu_j, 0)): four roundings (three for a list) after one exp; log1p and the
quotient x / (1 + x) are within a few ulp and have condition <= 1; the per-lane sums, the wave tree, the waves and the
chunk fold add n_g non-negative numbers in some order, which adds at most (n_g - 1) ulp.  The reference has the same
budget, so per group and per output |got - ref| <= (n_g + 16) 2^-52 ref.
"""
import ctypes
import functools
import math

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import evidence as ev
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.fisher import MCFisher
from lip_amd.ggn import clear_engine_cache
from lip_amd.lla import (posterior_lla_diag, posterior_lla_ekfac, posterior_lla_kfac, predict_lla_diag, predict_lla_ekfac,
                         predict_lla_kfac)
from lip_amd.prior import GroupedPrior
from lip_amd.train_alpha import (fit_alpha_diag, fit_alpha_diag_layerwise, fit_alpha_ekfac_layerwise, fit_alpha_kfac_layerwise,
                                 log_marginal_likelihood_diag, log_marginal_likelihood_ekfac,
                                 log_marginal_likelihood_ekfac_layerwise, log_marginal_likelihood_kfac,
                                 log_marginal_likelihood_kfac_layerwise)
from lip_amd.utils import flatten_nn_params

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
N_FULL = kf.N_FULL
C = ev.CHUNK


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
KRON_SHAPES = [(1, 1), (1, 10), (7, 3), (64, 64), (65, 1), (257, 33), (1153, 64),
               (217, 151), (256, 128), (9, 3641)]                    # the last three: CHUNK - 1, CHUNK, CHUNK + 1 terms
LIST_LENGTHS = [1, 63, 64, 65, 4099, C - 1, C, C + 1]
assert [r * c for r, c in KRON_SHAPES[-3:]] == [C - 1, C, C + 1]


def _values(n, g):
    """n values spread over 1e-12 .. 1e12 with exact zeros and small negatives (which count as 0)"""
    v = 10.0 ** (24.0 * torch.rand(n, dtype=F64, generator=g) - 12.0)
    u = torch.rand(n, generator=g)
    v[u < 0.05] = 0.0
    v[(u >= 0.05) & (u < 0.10)] = -1e-18
    return v


def _table(layout, seed):
    """(vals, segments, G) for a list of ("kron", (rows, cols), group) / ("list", n, group) entries"""
    g = torch.Generator().manual_seed(seed)
    parts, segs, off = [], [], 0
    for kind, shape, group in layout:
        scale = float(10.0 ** (4.0 * torch.rand((), dtype=F64, generator=g) - 2.0))
        if kind == "kron":
            r, c = shape
            segs.append(ev.Segment(ev.KRON, off, r, c, scale, group))
            n = r + c
        else:
            segs.append(ev.Segment(ev.LIST, off, shape, 1, scale, group))
            n = shape
        parts.append(_values(n, g))
        off += n
    return torch.cat(parts), segs, 1 + max(s.group for s in segs)


def _layouts():
    every = [("kron", s, 0) for s in KRON_SHAPES] + [("list", n, 0) for n in LIST_LENGTHS]
    own = [(k, s, i) for i, (k, s, _) in enumerate(every)]           # every shape alone in a group: a bound per shape
    one = every                                                      # G = 1
    five = [("kron", (257, 33), 0), ("list", 4099, 1), ("list", C + 1, 0), ("kron", (9, 3641), 2), ("kron", (7, 3), 0),
            ("list", 1, 3), ("list", 65, 4), ("kron", (64, 64), 1), ("list", 63, 0)]     # group 0: non-adjacent, both kinds;
    return {"own_groups": own, "one_group": one, "five_groups": five}                    # group 3: a single term


@functools.lru_cache(maxsize=None)
def _case(name):
    """the table of a layout, its plan on the CPU and on the device, and the log precisions in [-20, 20]"""
    vals, segs, G = _table(_layouts()[name], seed=len(name))
    if name == "five_groups":
        single = [s for s in segs if s.group == 3]
        assert len(single) == 1 and single[0].terms == 1
        vals[single[0].off] = 3.7e-3                                  # a single term that is not one of the planted zeros
    g = torch.Generator().manual_seed(7 + len(name))
    la = 40.0 * torch.rand(G, dtype=F64, generator=g) - 20.0
    la[0], la[-1] = -20.0, 20.0
    t2 = torch.rand(G, dtype=F64, generator=g)
    names = [f"g{i}" for i in range(G)]
    return dict(vals=vals, segs=segs, G=G, la=la, t2=t2, names=names, cpu=ev.EvidencePlan(vals, segs, t2, names),
                gpu=ev.EvidencePlan(vals.to(DEV), segs, t2, names))


@pytest.mark.parametrize("r", [1.0, 40.0 / 3.0], ids=["r1", "r40_3"])
@pytest.mark.parametrize("name", list(_layouts()))
def test_kernel_against_float64_torch_on_the_cpu(name, r):
    c = _case(name)
    Lr, Tr = c["cpu"].terms(c["la"], r)
    L, T = c["gpu"].terms(c["la"].to(DEV), r)
    assert L.is_cuda and L.dtype == T.dtype == F64 and L.shape == T.shape == (c["G"],)
    n = c["cpu"].terms_per_group.double()
    bound = (n + 16.0) * 2.0 ** -52
    eL = ((L.cpu() - Lr).abs() / (bound * Lr).clamp_min(1e-300)).max().item()
    eT = ((T.cpu() - Tr).abs() / (bound * Tr).clamp_min(1e-300)).max().item()
    print(f"{name} r={r:.3g}: G = {c['G']}, worst |got - ref| / bound  L {eL:.3f}  T {eT:.3f}")
    assert bool(torch.isfinite(L).all()) and bool(torch.isfinite(T).all()) and bool((Lr > 0).all())
    assert bool(((L.cpu() - Lr).abs() <= bound * Lr).all())
    assert bool(((T.cpu() - Tr).abs() <= bound * Tr).all())
    assert bool((T.cpu() <= n).all())                                 # every quotient is below 1


def test_results_are_bitwise_reproducible_and_operands_stay():
    c = _case("five_groups")
    plan, la = c["gpu"], c["la"].to(DEV)
    vals0, la0 = plan.vals.clone(), la.clone()
    L1, T1 = plan.terms(la, 40.0 / 3.0)
    L2, T2 = plan.terms(la, 40.0 / 3.0)
    again = ev.EvidencePlan(plan.vals.clone(), c["segs"], c["t2"], c["names"])          # a plan rebuilt from the same table
    L3, T3 = again.terms(la.clone(), 40.0 / 3.0)
    torch.cuda.synchronize()
    assert torch.equal(L1, L2) and torch.equal(T1, T2) and torch.equal(L1, L3) and torch.equal(T1, T3)
    assert torch.equal(plan.vals, vals0) and torch.equal(la, la0)
    v, g = ev.lml_structured(la, plan, 40.0 / 3.0)
    vr, gr = ev.lml_structured(c["la"], c["cpu"], 40.0 / 3.0)
    assert g.is_cuda and abs(v - vr) <= 1e-12 * abs(vr) and float((g.cpu() - gr).abs().max()) <= 1e-12 * float(gr.abs().max())


def test_bad_arguments_are_status_codes():
    c = _case("five_groups")
    plan, lib = c["gpu"], nv.load()
    d = plan._dev
    la = c["la"].to(DEV)
    out0 = torch.full((plan.G, 2), 3.0, device=DEV, dtype=F64)
    out = out0.clone()
    n_seg = len(plan.segments)

    def call(table=None, **kw):
        host = d["segs_host"] if table is None else table
        args = dict(vals=plan.vals.data_ptr(), n_vals=plan.vals.numel(), segs_host=ctypes.addressof(host), segs=d["segs"].data_ptr(),
                    n_seg=n_seg, chunks=d["chunks"].data_ptr(), n_chunks=len(plan.chunks), chunk_terms=plan.chunk,
                    ptr=d["ptr"].data_ptr(), idx=d["idx"].data_ptr(), la=la.data_ptr(), G=plan.G, r=1.0, out=out.data_ptr(),
                    scratch=d["scratch"].data_ptr(), scratch_doubles=d["scratch"].numel(), stream=nv.stream_ptr())
        args.update(kw)
        return lib.lip_evidence_terms(*args.values())

    def edited(k, **fields):
        host = (nv.EvSeg * n_seg).from_buffer_copy(d["segs_host"])
        for f, v in fields.items():
            setattr(host[k], f, v)
        return host

    for key in ("vals", "segs_host", "segs", "chunks", "ptr", "idx", "la", "out", "scratch"):
        assert call(**{key: None}) == 1, key
        assert b"lip_evidence_terms" in lib.lip_last_error()
    kron = next(k for k, s in enumerate(plan.segments) if s.kind == ev.KRON)
    lst = next(k for k, s in enumerate(plan.segments) if s.kind == ev.LIST)
    n_vals = plan.vals.numel()
    bad_tables = [edited(kron, group=plan.G), edited(lst, group=-1), edited(kron, rows=0), edited(kron, rows=-3),
                  edited(kron, cols=0), edited(lst, rows=0), edited(lst, cols=0), edited(kron, off=n_vals - 3),
                  edited(lst, off=n_vals - plan.segments[lst].rows + 1), edited(lst, off=-1), edited(lst, kind=2),
                  edited(lst, scale=float("nan"))]
    for i, host in enumerate(bad_tables):
        assert call(table=host) == 1, i
    for r in (float("inf"), float("-inf"), float("nan"), -1.0):
        assert call(r=r) == 1, r
    for kw in (dict(G=0), dict(n_seg=0), dict(n_vals=0), dict(n_chunks=len(plan.chunks) + 1), dict(chunk_terms=0),
               dict(scratch_doubles=2 * len(plan.chunks) - 1)):
        assert call(**kw) == 1, kw
    need = ctypes.c_int64(-7)
    assert lib.lip_evidence_terms_scratch(0, ctypes.byref(need)) == 1 and need.value == -7
    assert lib.lip_evidence_terms_scratch(5, None) == 1
    assert lib.lip_evidence_terms_scratch(5, ctypes.byref(need)) == 0 and need.value >= 10
    torch.cuda.synchronize()
    assert torch.equal(out, out0)                                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    L, T = plan.terms(la, 1.0)
    assert torch.equal(out[:, 0], L) and torch.equal(out[:, 1], T)
    with pytest.raises(ValueError, match="log precisions"):
        plan.terms(la[:-1])


# ------------------------------------------------------------------------------------------------ on the nets
@functools.lru_cache(maxsize=None)
def _helper(name):
    """the float64 helper's curvature of a net, built once and never written to"""
    state, Z, model_type = kf.make_case(name)
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    flat = flatten_nn_params(state.params)[0].detach().double()
    _, J, H = er.jacobian(state, Z, model_type)
    Lams0 = er.scales_ref(J, H, state, er.orthonormal_bases(state, As, Ss, model_type))
    diag1 = kf.ggn_diag_ref(state, Z, model_type, None)
    Xnew = kref.new_points(Z, 5, 7)
    f_new, J_new = ref.jac64(state, Xnew, model_type)
    return dict(state=state, Z=Z, model_type=model_type, M=M, alpha=alpha, flat=flat, D=flat.numel(), diag1=diag1,
                spec_kfac=kf.spectrum_ref(state, As, Ss, M, model_type, diag1),
                spec_ekfac=er.spectrum_ref(state, Lams0, model_type, diag1), Xnew=Xnew, J_new=J_new)


def _layer_prior(h, equal=False):
    G = GroupedPrior(h["state"].params, 1.0, "layer").G
    return GroupedPrior(h["state"].params, [h["alpha"] * (1.0 if equal else 2.0 ** (g % 4)) for g in range(G)], "layer")


def _spectrum_order(h, a):
    """the (D,) prior vector in the order of the helper's block spectra: block by block, then the remainder"""
    parts = [a[off:off + Mt * N] for _, off, Mt, N, _, _ in kf.blocks_of(h["state"])]
    return torch.cat(parts + [a[kf.remainder_of(h["state"])]])


def _want(h, prior, spec, a_spec):
    a = prior.vector("cpu", F64)
    return float(-0.5 * (a * h["flat"] ** 2).sum() - 0.5 * torch.log1p((N_FULL / h["M"]) * spec / a_spec).sum())


# measured on MI355X: |got - want| / |want| of the layer-wise evidence against the helper's spectra, diag / kfac / ekfac:
#   sine_regressor 2.33e-8 / 2.61e-8 / 9.36e-9    xor_classifier 6.75e-9 / 4.40e-9 / 1.39e-8
#   mlp_ragged     9.11e-9 / 2.91e-8 / 2.92e-8    resnet_tiny    2.50e-8 / 2.83e-8 / 3.05e-8
#   resnet50_tiny  1.65e-8 / 1.27e-8 / 8.67e-9    flat_head      2.85e-9 / 1.07e-8 / 1.19e-8
#   stem_net       1.96e-8 / 5.54e-9 / 9.42e-9
# (the float32 factors and diagonal of the fit against float64 ones; the kernel's own share is the 1e-16 of the test above)
DIAG_LML_TOL = 1.0e-7          # 4 x 2.50e-8
KFAC_LML_TOL = 1.2e-7          # 4 x 2.91e-8
EKFAC_LML_TOL = 1.3e-7         # 4 x 3.05e-8


@pytest.mark.parametrize("name", kf.NETS)
def test_layerwise_evidence_matches_the_float64_helper(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    prior = _layer_prior(h)
    a = prior.vector("cpu", F64)
    kw = dict(full_set_size=N_FULL)
    got = {"diag": log_marginal_likelihood_diag(prior, Z, state, model_type, **kw),
           "kfac": log_marginal_likelihood_kfac_layerwise(prior, Z, state, model_type, **kw),
           "ekfac": log_marginal_likelihood_ekfac_layerwise(prior, Z, state, model_type, **kw)}
    want = {"diag": _want(h, prior, h["diag1"].clamp_min(0.0), a),
            "kfac": _want(h, prior, h["spec_kfac"], _spectrum_order(h, a)),
            "ekfac": _want(h, prior, h["spec_ekfac"], _spectrum_order(h, a))}
    e = {k: abs(got[k] - want[k]) / abs(want[k]) for k in got}
    print(f"{name}: " + "  ".join(f"{k} got {got[k]:.12g} want {want[k]:.12g} rel {e[k]:.2e}" for k in got))
    assert e["diag"] <= DIAG_LML_TOL and e["kfac"] <= KFAC_LML_TOL and e["ekfac"] <= EKFAC_LML_TOL


@pytest.mark.parametrize("name", kf.NETS)
def test_equal_groups_give_the_scalar_evidence_of_the_same_binding(name):
    """the factors and their eigenvalues are the same numbers; only the order of the sums differs"""
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    prior = _layer_prior(h, equal=True)
    bound = (h["D"] + 16) * 2.0 ** -52
    pairs = {"kfac": (log_marginal_likelihood_kfac_layerwise(prior, Z, state, model_type, full_set_size=N_FULL),
                      log_marginal_likelihood_kfac(alpha, Z, state, model_type, full_set_size=N_FULL)),
             "ekfac": (log_marginal_likelihood_ekfac_layerwise(prior, Z, state, model_type, full_set_size=N_FULL),
                       log_marginal_likelihood_ekfac(alpha, Z, state, model_type, full_set_size=N_FULL)),
             "diag": (log_marginal_likelihood_diag(prior, Z, state, model_type, full_set_size=N_FULL),
                      log_marginal_likelihood_diag(alpha, Z, state, model_type, full_set_size=N_FULL))}
    for k, (got, want) in pairs.items():
        print(f"{name} {k}: layer-wise {got:.17g} scalar {want:.17g} rel {abs(got - want) / abs(want):.2e} bound {bound:.2e}")
    for k, (got, want) in pairs.items():
        assert abs(got - want) <= bound * abs(want), k


def _as_bk(x, B):
    return x.reshape(B, -1)


FITS = {"diag": (fit_alpha_diag_layerwise, posterior_lla_diag, lambda *a, **kw: predict_lla_diag(*a, cov="diag", **kw)),
        "kfac": (fit_alpha_kfac_layerwise, posterior_lla_kfac, lambda *a, **kw: predict_lla_kfac(*a, cov="diag", route="sweep", **kw)),
        "ekfac": (fit_alpha_ekfac_layerwise, posterior_lla_ekfac,
                  lambda *a, **kw: predict_lla_ekfac(*a, cov="diag", route="sweep", **kw))}


@pytest.mark.parametrize("which", list(FITS))
@pytest.mark.parametrize("name", kf.NETS)
def test_fitted_prior_goes_through_the_posterior_and_its_predictives(name, which):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    fit, posterior, predict = FITS[which]
    prior, hist = fit(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=20)
    assert isinstance(prior, GroupedPrior) and prior.D == h["D"] and len(hist) == 20
    assert all(a.shape == (prior.G,) and a.dtype == F64 and not a.is_cuda and isinstance(v, float) for a, v in hist)
    assert float((hist[0][0] - alpha).abs().max()) <= 1e-14 * alpha
    assert max(v for _, v in hist) >= hist[0][1]
    assert bool(torch.isfinite(prior.values).all()) and bool((prior.values > 0).all())
    post = posterior(state, Z, model_type, prior, full_set_size=N_FULL)
    assert bool(torch.isfinite(post.variance()).all())
    B = h["Xnew"].shape[0]
    mean, var = predict(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL)
    var = _as_bk(var, B).double().cpu()
    prior_var = torch.einsum("bkd,d,bkd->bk", h["J_new"], 1.0 / prior.vector("cpu", F64), h["J_new"])
    assert var.shape == prior_var.shape and bool(torch.isfinite(var).all()) and bool((var >= 0).all())
    worst = float((var / prior_var).max())
    print(f"{name} {which}: G = {prior.G}, evidence {hist[0][1]:.8g} -> {max(v for _, v in hist):.8g}, "
          f"largest predictive variance / prior variance {worst:.6f}")
    # the posterior precision is the prior's plus a positive semi-definite curvature; the float32 sums of the predictive
    # are within 1e-5 of their float64 value (tests/test_kfac_predict_sweep.py bounds them tighter)
    assert bool((var <= prior_var * (1.0 + 1e-5)).all())
    if model_type == "classifier":
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, h["J_new"].shape[1], (B,), generator=g)
        kw = {} if which == "diag" else {"route": "sweep"}
        nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(h["Xnew"][:3], y[:3]), (h["Xnew"][3:], y[3:])], Z, prior,
                                                                   N_FULL, model_type, posterior=which, **kw)
        assert probs.shape == (B, h["J_new"].shape[1]) and bool(torch.isfinite(probs).all())
        assert all(map(math.isfinite, (nll, acc, brier, ece_)))


def test_scalar_diag_fit_does_not_lose_evidence():
    h = _helper("resnet_tiny")
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    got = log_marginal_likelihood_diag(alpha, Z, state, model_type, full_set_size=N_FULL)
    a_fit, hist = fit_alpha_diag(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=20)
    assert len(hist) == 20 and abs(hist[0][1] - got) <= 1e-12 * abs(got) and a_fit > 0 and math.isfinite(a_fit)
    assert log_marginal_likelihood_diag(a_fit, Z, state, model_type, full_set_size=N_FULL) >= hist[0][1]


def test_mc_fisher_spec_builds_the_plans_reproducibly():
    h = _helper("xor_classifier")
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    prior = _layer_prior(h)
    for fn in (log_marginal_likelihood_diag, log_marginal_likelihood_kfac_layerwise, log_marginal_likelihood_ekfac_layerwise):
        v1 = fn(prior, Z, state, model_type, full_set_size=N_FULL, curvature=MCFisher(2, 11))
        clear_engine_cache()
        v2 = fn(prior, Z, state, model_type, full_set_size=N_FULL, curvature=MCFisher(2, 11))
        assert math.isfinite(v1) and v1 == v2, fn.__name__
        assert v1 != fn(prior, Z, state, model_type, full_set_size=N_FULL)
    plan = ev.plan_kfac(state, Z, model_type, prior, curvature=MCFisher(2, 11))
    assert plan.vals.is_cuda and plan.G == prior.G and int(plan.terms_per_group.sum()) == h["D"]
