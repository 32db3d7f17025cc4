"""GPU checks of the one-pass grid of prior precisions: the kernel ``lip_kfac_predict_grid`` on synthetic operands
through ctypes, then ``LinearizedNet.kfac_predict_grid``, the grid predictives of ``kfac.py`` / ``ekfac.py``,
``evaluate.eval_dataset_closed_form_grid`` and ``train_alpha.grid_search_alpha`` on the nets of tests/kfac_ref.py.

Kernel level: the reference is a float64 einsum of the up-cast float32 operands, and the bound is the float64 summation
bound of tests/test_kfac.py on the absolute-value twin of the reference, 4 (2 (Mt + N) + Mt N + 8) 2^-53; it holds for
any summation order, and the division and the add into ``out`` are two more roundings inside the + 8.

Engine level: the rows come from the float32 passes, so no bound is derivable; every bound there is 4 x the worst error
measured on MI355X against the float64 helpers, with the measured figure next to it.
"""
import ctypes
import functools
import math

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
from lip_amd import _native as nv
from lip_amd import ekfac, evaluate, kfac
from lip_amd.engine import LinearizedNet
from lip_amd.evaluate import eval_dataset_closed_form, eval_dataset_closed_form_grid
from lip_amd.ggn import clear_engine_cache, get_engine
from lip_amd.lla import predict_lla_ekfac, predict_lla_ekfac_grid, predict_lla_kfac, predict_lla_kfac_grid
from lip_amd.prior import GroupedPrior
from lip_amd.train_alpha import grid_search_alpha
from test_ekfac import _helper

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -53
DEV = "cuda"
N_FULL = kf.N_FULL
SCALES = (1.0, 3.5, 12.0)


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
GRID_BLOCKS = [(1, 1), (9, 3), (37, 5), (33, 33), (145, 16), (3, 130)]      # (3, 130): past the four-column-tile block edge


def _grid_scratch(B, Kc, Mt, N, G):
    d = ctypes.c_int64(0)
    nv.check(nv.load().lip_kfac_predict_grid_scratch(B, Kc, Mt, N, G, ctypes.byref(d)), "lip_kfac_predict_grid_scratch")
    tiles = ((Mt + 31) // 32) * ((N + 31) // 32)
    assert d.value == G * Mt * N + B * Kc * (Mt * N + tiles * G)                # the header's formula
    return d.value


def _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales, out=None, scratch_doubles=None):
    G = len(scales)
    doubles = _grid_scratch(B, Kc, Mt, N, G) if scratch_doubles is None else scratch_doubles
    scratch = torch.empty(doubles, device=DEV, dtype=F64)
    out = torch.zeros(G, B, Kc, device=DEV, dtype=F64) if out is None else out
    sc = (ctypes.c_double * G)(*scales)
    nv.check(nv.load().lip_kfac_predict_grid(Jr.data_ptr(), ldj, B, Kc, off, Mt, N, V.data_ptr(), Ub.data_ptr(), Ev.data_ptr(),
                                             sc, G, out.data_ptr(), scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_kfac_predict_grid")
    torch.cuda.synchronize()
    return out


def _run_predict_diag(Jr, ldj, B, Kc, off, Mt, N, V, Ub, R):
    scratch = torch.empty(2 * B * Kc * Mt * N, device=DEV, dtype=F64)
    out = torch.zeros(B, Kc, device=DEV, dtype=F64)
    nv.check(nv.load().lip_kfac_predict(Jr.data_ptr(), ldj, B, Kc, off, Mt, N, V.data_ptr(), Ub.data_ptr(), R.data_ptr(),
                                        out.data_ptr(), 1, scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
             "lip_kfac_predict")
    torch.cuda.synchronize()
    return out


def _log_scales(G):
    return [0.03] if G == 1 else [0.03 * (40.0 / 0.03) ** (g / (G - 1)) for g in range(G)]


@pytest.mark.parametrize("G", [1, 3, 32])
@pytest.mark.parametrize("Mt,N", GRID_BLOCKS)
def test_grid_against_float64_einsum(Mt, N, G):
    g = torch.Generator().manual_seed(Mt * 1000 + N * 10 + G)
    off = 5
    ldj = off + Mt * N + 3
    V = torch.randn(Mt, Mt, generator=g, dtype=F64).to(DEV)
    Ub = torch.randn(N, N, generator=g, dtype=F64).to(DEV)
    Ev = 5.0 * torch.rand(Mt, N, generator=g, dtype=F64)
    Ev[0] = 0.0                                                                  # exact zeros, as the centred head has
    Ev = Ev.to(DEV)
    scales = _log_scales(G)
    Wt = 1.0 / (Ev[None] + torch.tensor(scales, dtype=F64, device=DEV)[:, None, None])      # (G, Mt, N)
    c = 4 * (2 * (Mt + N) + Mt * N + 8) * U
    for B, Kc in [(1, 1), (5, 3)]:
        Jr = torch.randn(Kc * B, ldj, generator=g, dtype=F32).to(DEV)
        J = Jr[:, off:off + Mt * N].double().reshape(Kc, B, Mt, N)
        T = V.T @ J @ Ub
        want = torch.einsum("gjl,kbjl->gbk", Wt, T * T)
        Ta = V.abs().T @ J.abs() @ Ub.abs()
        twin = torch.einsum("gjl,kbjl->gbk", Wt, Ta * Ta)
        base = _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales)
        out0 = torch.randn(G, B, Kc, generator=g, dtype=F64).to(DEV)
        added = _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales, out=out0.clone())
        err = (base - want).abs()
        err_added = (added - (out0 + want)).abs()
        ratio = max((err / (c * twin)).max().item(), (err_added / (c * (twin + out0.abs()))).max().item())
        assert bool((err <= c * twin).all()) and bool((err_added <= c * (twin + out0.abs())).all())
        assert torch.equal(added, out0 + base)                                  # out is added into, by one rounded add
        assert torch.equal(base, _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales))   # bitwise reproducible
        if B > 1:                                                               # a scratch for two points: three chunks
            small = _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales, scratch_doubles=_grid_scratch(2, Kc, Mt, N, G))
            assert torch.equal(small, base)
        if G >= 3:                                                              # a slice sees its own scale alone
            three = _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales[:3])
            one = _run_grid(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Ev, scales[1:2])
            assert torch.equal(three[1], one[0]) and torch.equal(three, base[:3])
        worst = 0.0
        for gi in sorted({0, G // 2, G - 1}):                                   # lip_kfac_predict(diag) at R = 1 / (Ev + s_g)
            dg = _run_predict_diag(Jr, ldj, B, Kc, off, Mt, N, V, Ub, Wt[gi].contiguous())
            d = (base[gi] - dg).abs() / (2 * c * twin[gi])
            worst = max(worst, d.max().item())
        print(f"grid Mt={Mt} N={N} G={G} B={B} Kc={Kc}: max err / bound {ratio:.3f}  against lip_kfac_predict / (2 bound) "
              f"{worst:.3f}")
        assert worst <= 1.0


def test_grid_status_codes_leave_the_output_untouched():
    lib = nv.load()
    B, Kc, off, Mt, N, G = 2, 3, 4, 9, 3, 3
    ldj = off + Mt * N
    Jr = torch.randn(Kc * B, ldj, dtype=F32).to(DEV)
    V, Ub = (torch.randn(s, dtype=F64).to(DEV) for s in ((Mt, Mt), (N, N)))
    Ev = torch.rand(Mt, N, dtype=F64).to(DEV)
    out0 = torch.full((G, B, Kc), 3.0, device=DEV, dtype=F64)
    out = out0.clone()
    scratch = torch.empty(_grid_scratch(B, Kc, Mt, N, G), device=DEV, dtype=F64)
    sc = (ctypes.c_double * 33)(*([1.0, 2.0, 3.0] + [1.0] * 30))
    good = [Jr.data_ptr(), ldj, B, Kc, off, Mt, N, V.data_ptr(), Ub.data_ptr(), Ev.data_ptr(), sc, G, out.data_ptr(),
            scratch.data_ptr(), scratch.numel(), nv.stream_ptr()]
    one_point = G * Mt * N + Kc * (Mt * N + G)                                   # one tile
    for i, v in [(0, 0), (7, 0), (8, 0), (9, 0), (10, None), (12, 0), (13, 0),                # null pointers
                 (2, 0), (3, 0), (5, 0), (6, 0), (2, -1),                                      # non-positive extents
                 (11, 0), (11, 33), (11, -1),                                                  # G outside [1, LIP_GRID_MAX]
                 (1, ldj - 1), (4, -1), (14, one_point - 1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_predict_grid(*args) == 1, (i, v)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for at in range(G):
            vals = [1.0, 2.0, 3.0]
            vals[at] = bad
            args = list(good)
            args[10] = (ctypes.c_double * G)(*vals)
            assert lib.lip_kfac_predict_grid(*args) == 1 and b"scale" in lib.lip_last_error(), (bad, at)
    # Mt N >= 2^31 is refused before any launch (nothing of that size exists)
    big = list(good)
    big[5], big[6], big[1] = 1 << 16, 1 << 15, 1 << 40
    assert lib.lip_kfac_predict_grid(*big) == 1
    d = ctypes.c_int64(-7)
    for bad in [(0, Kc, Mt, N, G), (B, Kc, Mt, N, 0), (B, Kc, Mt, N, 33), (B, Kc, 1 << 16, 1 << 15, G)]:
        assert lib.lip_kfac_predict_grid_scratch(*bad, ctypes.byref(d)) == 1 and d.value == -7
    assert lib.lip_kfac_predict_grid_scratch(B, Kc, Mt, N, G, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(out, out0)
    args = list(good)
    args[14] = one_point                                                        # the one-point minimum itself is taken
    assert lib.lip_kfac_predict_grid(*args) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out, out0)


# ------------------------------------------------------------------------------------------------ engine level
def _prior(h, grouped):
    return kf.split_prior(h["state"], h["alpha"]) if grouped else h["alpha"]


def _rem_var(h, a, s):
    return 1.0 / (s * a[h["rem"]] + h["diag"][h["rem"]])


@functools.lru_cache(maxsize=None)
def _kfac_reference(name, grouped):
    """(G, 5, K) float64 CPU: the dense helper's marginal variances of the new points at every s a; built once per net
    and prior and never written to"""
    h = _helper(name)
    a = kf.prior_vector(h["state"], h["alpha"], grouped)
    out = []
    for s in SCALES:
        cov_blocks, _ = kf.covariance_blocks(h["state"], h["As"], h["Ss"], h["M"], h["model_type"], s * a, N_FULL)
        out.append(torch.diagonal(kf.predict_dense(h["J_new"], cov_blocks, h["rem"], _rem_var(h, a, s)), dim1=1, dim2=2))
    return torch.stack(out)


def _ekfac_reference(h, grouped, bases):
    """the EKFAC helper of tests/test_ekfac.py's comparison at every s a: the product's basis at s a is (V / sqrt(s), Ub),
    the helper forms the second moments of its own float64 rows in that basis and the dense covariance"""
    a = kf.prior_vector(h["state"], h["alpha"], grouped)
    out = []
    for s in SCALES:
        scaled = [(V / math.sqrt(s), Ub) for V, Ub in bases]
        cov_blocks = er.covariance_blocks(h["state"], scaled, er.scales_ref(h["J"], h["H"], h["state"], scaled), h["recal"])
        out.append(torch.diagonal(kf.predict_dense(h["J_new"], cov_blocks, h["rem"], _rem_var(h, a, s)), dim1=1, dim2=2))
    return torch.stack(out)


def _rel(got, want):
    want = want.to(got.device)
    return ((got.double() - want).abs().max() / want.abs().max()).item()


# measured on MI355X, worst over the three scales of max|got - ref| / max|ref| of the grid variances against the float64
# helper, KFAC / EKFAC, scalar prior (two-group prior):
#   sine_regressor 3.66e-7 / 3.04e-7 (3.67e-7 / 3.07e-7)   xor_classifier 6.27e-8 / 6.58e-8 (7.45e-8 / 6.66e-8)
#   mlp_ragged     1.24e-7 / 1.15e-7 (1.34e-7 / 1.19e-7)   resnet_tiny    6.71e-8 / 6.09e-8 (6.69e-8 / 6.28e-8)
#   resnet50_tiny  2.01e-7 / 1.81e-7 (2.17e-7 / 1.92e-7)   flat_head      7.92e-8 / 7.16e-8 (6.17e-8 / 5.56e-8)
#   stem_net       3.54e-8 / 3.68e-8 (3.58e-8 / 3.74e-8)
# At s = 1 these are the figures of tests/test_kfac.py and tests/test_ekfac.py for the diag predictive (the same rows and
# float64 products); none exceeds their PREDICT_TOL.
GRID_TOL = 1.5e-6              # 4 x 3.67e-7
MEAN_TOL = 1.3e-6              # tests/test_kfac.py: 4 x 3.20e-7, the same float32 forward pass


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kf.NETS)
def test_grid_predictives_match_the_float64_helpers(name, grouped):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    prior = _prior(h, grouped)
    K = h["f_new"].shape[1]
    shape = (len(SCALES), 5) if model_type == "regressor" else (len(SCALES), 5, K)
    mean, var = predict_lla_kfac_grid(state, h["Xnew"], Z, model_type, prior, SCALES, full_set_size=N_FULL, batch=3)
    assert var.shape == shape and mean.shape == shape[1:] and var.dtype == mean.dtype == F64 and var.is_cuda
    assert float(var.min()) >= 0.0 and bool((var[0] >= var[1]).all()) and bool((var[1] >= var[2]).all())
    e_kfac = [_rel(var[g].reshape(5, K), w) for g, w in enumerate(_kfac_reference(name, grouped))]
    e_mean = _rel(mean.reshape(5, K), h["f_new"])
    mean_e, var_e = predict_lla_ekfac_grid(state, h["Xnew"], Z, model_type, prior, SCALES, full_set_size=N_FULL, batch=3)
    assert var_e.shape == shape and mean_e.shape == shape[1:] and float(var_e.min()) >= 0.0
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, prior, N_FULL, None)
    want_e = _ekfac_reference(h, grouped, [(V.cpu(), Ub.cpu()) for V, _, Ub in fits])
    e_ekfac = [_rel(var_e[g].reshape(5, K), w) for g, w in enumerate(want_e)]
    print(f"{name} {'grouped' if grouped else 'scalar'}: grid against the helper  KFAC {max(e_kfac):.2e}  EKFAC {max(e_ekfac):.2e}  "
          f"mean {e_mean:.2e}  per scale {['%.2e' % e for e in e_kfac + e_ekfac]}")
    assert max(e_kfac) <= GRID_TOL and max(e_ekfac) <= GRID_TOL and e_mean <= MEAN_TOL


# measured on MI355X, worst scale, KFAC / EKFAC: resnet_tiny 1.83e-7 / 1.89e-7, xor_classifier 9.66e-8 / 5.36e-8
SWEEP_ROWS_TOL = 7.6e-7        # tests/test_kfac_predict_sweep.py's DIAG_ROWS_TOL: the sweep's diag form against the rows route


@pytest.mark.parametrize("name", ["resnet_tiny", "xor_classifier"])
def test_sweep_route_matches_the_rows_route(name, monkeypatch):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    calls = []
    inner = kfac.compute_kfac_factors
    monkeypatch.setattr(kfac, "compute_kfac_factors", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    worst = []
    for predict in (predict_lla_kfac_grid, predict_lla_ekfac_grid):
        _, rows = predict(state, h["Xnew"][:3], Z, model_type, h["alpha"], SCALES, full_set_size=N_FULL)
        _, sweep = predict(state, h["Xnew"][:3], Z, model_type, h["alpha"], SCALES, full_set_size=N_FULL, route="sweep")
        assert sweep.shape == rows.shape and sweep.dtype == F64
        worst.append(max(((sweep[g] - rows[g]).abs().max() / rows[g].abs().max()).item() for g in range(len(SCALES))))
    print(f"{name}: sweep route against the rows route  KFAC {worst[0]:.2e}  EKFAC {worst[1]:.2e}")
    assert len(calls) == 2                                                      # one fit per posterior, no refit per scale
    assert max(worst) <= SWEEP_ROWS_TOL


# measured on MI355X, worst over the three scales of max|grid slice - fresh fit| / max|fresh fit|, scalar prior (two-group
# prior), KFAC / EKFAC:
#   xor_classifier 1.07e-15 / 9.48e-16 (1.18e-15 / 1.05e-15)   resnet_tiny 8.29e-9 / 1.24e-8 (1.06e-8 / 4.31e-9)
# (a second run repeated xor_classifier's figures and gave resnet_tiny 6.29e-9 / 8.78e-9 (5.86e-9 / 1.16e-8))
# Far below the float32 floor of the rows: on the dense net the two fits read bitwise the same factors and only the
# float64 algebra differs; on resnet_tiny the fresh fit's factors come from a backward sweep of their own, whose BN
# reductions may go through float atomics (the note in tests/test_kfac.py), so they differ in the last float32 bits.
# The validation NLLs of the search against a loop over its ten values (xor_classifier): 0 (KFAC), 1.59e-16 (EKFAC).
SLICE_TOL = 5.0e-8             # 4 x 1.24e-8


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", ["xor_classifier", "resnet_tiny"])
def test_grid_slice_is_the_predictive_of_a_fresh_fit_at_the_scaled_prior(name, grouped):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    prior = _prior(h, grouped)
    _, var = predict_lla_kfac_grid(state, h["Xnew"], Z, model_type, prior, SCALES, full_set_size=N_FULL)
    _, var_e = predict_lla_ekfac_grid(state, h["Xnew"], Z, model_type, prior, SCALES, full_set_size=N_FULL)
    errs = []
    for g, s in enumerate(SCALES):
        clear_engine_cache()
        _, fresh = predict_lla_kfac(state, h["Xnew"], Z, model_type, evaluate.scaled_prior(prior, s), full_set_size=N_FULL,
                                    cov="diag")
        _, fresh_e = predict_lla_ekfac(state, h["Xnew"], Z, model_type, evaluate.scaled_prior(prior, s), full_set_size=N_FULL,
                                       cov="diag")
        errs += [_rel(var[g], fresh), _rel(var_e[g], fresh_e)]
    print(f"{name} {'grouped' if grouped else 'scalar'}: grid slice against a fresh fit  KFAC {max(errs[0::2]):.2e}  "
          f"EKFAC {max(errs[1::2]):.2e}")
    assert max(errs) <= SLICE_TOL


def test_engine_method_checks_its_operands_and_groups_the_scales():
    h = _helper("xor_classifier")
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    fit = kfac._cached_fit(state, Z, model_type, h["alpha"], N_FULL, None)
    assert isinstance(fit, kfac.Fit) and len(fit) == 5                           # the private tuple keeps its shape
    (_, fits, rem_idx, _, a_rem), Evs, h_rem = fit, fit.Evs, fit.h_rem
    bases = [(f[0], f[2]) for f in fits]
    rem = (rem_idx, a_rem, h_rem)
    eng = get_engine(state, h["Xnew"], model_type)
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_predict_grid(bases[:1], Evs, rem, [1.0])
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_predict_grid(bases, Evs[:1], rem, [1.0])
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_predict_grid([(bases[0][0].float(), bases[0][1])] + bases[1:], Evs, rem, [1.0])
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_predict_grid(bases, [Evs[0].T] + Evs[1:], rem, [1.0])
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_predict_grid(bases, [Evs[0].cpu()] + Evs[1:], rem, [1.0])
    for bad in ([], [0.0], [1.0, float("nan")]):
        with pytest.raises(ValueError, match="finite positive"):
            eng.kfac_predict_grid(bases, Evs, rem, bad)
    with pytest.raises(ValueError, match="class_chunk must be positive"):
        eng.kfac_predict_grid(bases, Evs, rem, [1.0], class_chunk=0)
    # one set of rows for every call below: more than 32 scales go through the kernel in groups of 32, and the class
    # blocks and a capped scratch change nothing, bitwise
    K = eng.K
    rows = eng._one_hot_rows(0, K, "raw").clone()
    eng._one_hot_rows = lambda k0, k1, mode: rows[k0:k1].contiguous()
    s35 = [0.05 * 1.25 ** g for g in range(35)]
    whole = eng.kfac_predict_grid(bases, Evs, rem, s35)
    assert whole.shape == (35, 5, K)
    for g in (0, 31, 32, 34):
        assert torch.equal(whole[g], eng.kfac_predict_grid(bases, Evs, rem, s35[g:g + 1])[0])
    assert torch.equal(whole, eng.kfac_predict_grid(bases, Evs, rem, s35, class_chunk=1))
    eng._scratches.pop("lip_kfac_predict_grid", None)
    eng.KFAC_SCRATCH_BYTES = 8                                                  # the one-point minimum per block
    assert torch.equal(whole, eng.kfac_predict_grid(bases, Evs, rem, s35))
    # slice g is kfac_predict (diag) on the rescaled triples, to the float64 algebra
    del eng.KFAC_SCRATCH_BYTES
    triples, rem_var = kfac.rescale_fit(fits, Evs, rem, s35[7])
    assert _rel(whole[7], eng.kfac_predict(triples, (rem_idx, rem_var), diag=True)) <= 1e-12
    del eng._one_hot_rows


# ------------------------------------------------------------------------------------------------ the surface
def _validation(state_dim, classes, seed=2):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(12, state_dim, dtype=F64, generator=g)
    y = torch.randint(0, classes, (12,), generator=g)
    return [(X[i:i + 4], y[i:i + 4]) for i in range(0, 12, 4)]


@pytest.mark.parametrize("posterior", ["kfac", "ekfac"])
def test_grid_search_selects_the_value_a_loop_over_the_grid_selects(posterior, monkeypatch):
    h = _helper("xor_classifier")
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    val = _validation(2, 2)
    fits, sweeps = [], []
    inner = kfac.compute_kfac_factors
    monkeypatch.setattr(kfac, "compute_kfac_factors", lambda *a, **kw: (fits.append(1), inner(*a, **kw))[1])
    rows = LinearizedNet._one_hot_rows
    monkeypatch.setattr(LinearizedNet, "_one_hot_rows", lambda self, k0, k1, mode: (sweeps.append(mode), rows(self, k0, k1, mode))[1])
    alpha, history = grid_search_alpha(state, Z, val, N_FULL, model_type, posterior=posterior, verbose=False,
                                       return_history=True)
    assert len(fits) == 1 and len(history) == 10 and isinstance(alpha, float)
    class_blocks = len(get_engine(state, val[0][0], model_type)._class_blocks(None))
    # two passes over three batches, one sweep of 'raw' rows per class block each; the EKFAC fit reads factor rows ('l')
    assert sweeps.count("raw") == 2 * 3 * class_blocks
    if posterior == "kfac":
        assert len(sweeps) == 2 * 3 * class_blocks
    monkeypatch.undo()
    loop = [eval_dataset_closed_form(state, val, Z, a, N_FULL, model_type, posterior=posterior, link="probit")[0]
            for a, _ in history]
    worst = max(abs(v - w) / abs(w) for (_, v), w in zip(history, loop))
    print(f"{posterior}: NLL of the search against a loop over its ten values {worst:.2e}")
    assert worst <= SLICE_TOL
    assert alpha == history[loop.index(min(loop))][0]
    # the four metrics of one grid call, link by link, against the same loop
    for link in ("probit", "bridge", "mc"):
        got = eval_dataset_closed_form_grid(state, val, Z, 1.0, [history[3][0], history[8][0]], N_FULL, model_type, posterior,
                                            link, num_samples=64, seed=3)
        for (a, _), m in zip((history[3], history[8]), got):
            want = eval_dataset_closed_form(state, val, Z, a, N_FULL, model_type, posterior=posterior, link=link,
                                            num_samples=64, seed=3)[:4]
            assert len(m) == 4 and all(abs(x - y) <= 1e-5 * max(1.0, abs(y)) for x, y in zip(m, want)), (link, m, want)


def test_grid_search_scales_a_grouped_prior_and_loops_the_other_posteriors():
    h = _helper("xor_classifier")
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    val = _validation(2, 2)
    base = kf.split_prior(state, h["alpha"])
    out, history = grid_search_alpha(state, Z, val, N_FULL, model_type, log10_min=-1, log10_max=1, n_coarse=3, refine=False,
                                     verbose=False, posterior="kfac", alpha_base=base, return_history=True)
    assert isinstance(out, GroupedPrior) and out.table == base.table and len(history) == 3
    ratio = out.values / base.values
    assert any(bool(((ratio - s).abs() <= 1e-12 * s).all()) for s in (0.1, 1.0, 10.0))
    want = eval_dataset_closed_form(state, val, Z, out, N_FULL, model_type, posterior="kfac")[0]
    best = min(v for _, v in history)
    assert abs(best - want) <= SLICE_TOL * abs(want)
    # a posterior without a grid predictive is evaluated value by value
    diag = eval_dataset_closed_form_grid(state, val, Z, h["alpha"], [1.0, 4.0], N_FULL, model_type, posterior="diag")
    for s, m in zip((1.0, 4.0), diag):
        assert m == eval_dataset_closed_form(state, val, Z, s * h["alpha"], N_FULL, model_type, posterior="diag")[:4]


def test_regressor_grid_gives_the_gaussian_nll_of_the_helper_variances():
    """NLL = mean 1/2 [log(2 pi v) + (y - m)^2 / v], v = f_var + exp(logvar).  A variance error dv moves a point's term by
    at most 1/2 (1 / v + r^2 / v^2) |dv| to first order, and |dv| <= GRID_TOL max|var_ref| by the engine test: that, with
    the largest factor over the points, is the bound (the means are the product's own on both sides)."""
    h = _helper("sine_regressor")
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    g = torch.Generator().manual_seed(4)
    y = h["f_new"].reshape(-1) + 0.3 * torch.randn(5, generator=g, dtype=F64)
    X = h["Xnew"]
    loader = [(X[:3], y[:3]), (X[3:], y[3:])]
    noise = math.exp(float(state.params["logvar"]["logvar"]))
    mean, _ = predict_lla_kfac_grid(state, X, Z, model_type, h["alpha"], SCALES, full_set_size=N_FULL)
    mean = mean.cpu()
    for posterior, want_var in (("kfac", _kfac_reference("sine_regressor", False)),):
        got = eval_dataset_closed_form_grid(state, loader, Z, h["alpha"], SCALES, N_FULL, model_type, posterior=posterior)
        assert len(got) == len(SCALES)
        for (nll, *rest), var in zip(got, want_var):
            v = var.reshape(-1) + noise
            r2 = (y - mean) ** 2
            want = float((0.5 * (torch.log(2.0 * math.pi * v) + r2 / v)).mean())
            bound = GRID_TOL * float(var.abs().max()) * float((0.5 * (1.0 / v + r2 / v ** 2)).max())
            print(f"{posterior}: Gaussian NLL {nll:.12g} against {want:.12g}, |diff| / bound {abs(nll - want) / bound:.3f}")
            assert abs(nll - want) <= bound and all(x != x for x in rest) and len(rest) == 3
