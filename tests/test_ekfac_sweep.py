"""GPU checks of the EKFAC second moments from backward sweeps: the projection kernels ``lip_kfac_project_patches`` and
``lip_rows_project`` on synthetic operands through ctypes, then the ``EIGEN`` sweep (``lip_vjp_eigen``,
``LinearizedNet.kfac_eigen_sqsums_sweep``) and the public surface (``moments="sweep"``, ``curvature=``) on the nets of
tests/kfac_ref.py, and ResNet-50 with K = 1000.

Kernel level: the reference is the float64 product of the up-cast float32 operands (``tests/ekfac_sweep_ref.py``) and
the bound is derived: one float32 rounding of the result plus the float64 summation bound on the absolute-value twin with
the factor 4 of tests/test_kfac.py, |err| <= 2^-24 |want| + 4 (L + 8) 2^-53 (|a| |V|), L the inner length.

Engine level: the operands come from the float32 passes, so no bound is derivable; every bound there is 4 x the worst
error measured on MI355X against the float64 helper, as max|err| / max|ref| over the blocks of a net, with the measured
figures next to it (the convention of tests/test_ekfac.py).  No measured figure exceeds 1e-5 of the maximum, the bound
tests/test_ggn_diag.py holds the square-sum sweep to.  The helper always works in the product's own basis.
"""
import ctypes
import math

import pytest
import torch

import ekfac_ref as er
import ekfac_sweep_ref as sr
import fisher_ref as fr
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import ekfac, krylov
from lip_amd.engine import LinearizedNet
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.fisher import Cotangents, EmpiricalFisher, MCFisher
from lip_amd.ggn import clear_engine_cache, compute_ekfac_scales, compute_ggn_diag, get_engine
from lip_amd.lla import posterior_lla_ekfac, predict_lla_ekfac
from lip_amd.scalemodels import ResNet50
from lip_amd.toymodels import create_state
from lip_amd.train_alpha import fit_alpha_ekfac, log_marginal_likelihood_ekfac
from lip_amd.utils import flatten_nn_params
from test_ekfac import CONV_NETS, _cpu, _helper, _orthonormal, _rel

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U53, U24 = 2.0 ** -53, 2.0 ** -24
DEV = "cuda"
N_FULL = kf.N_FULL
PAD = 64                                   # canary floats either side of an output
CANARY = -12345.5


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


def _guarded(count):
    """(buffer, view): ``count`` output floats with PAD canaries either side; the view is 16-byte aligned"""
    buf = torch.full((count + 2 * PAD,), CANARY, device=DEV, dtype=F32)
    return buf, buf[PAD:PAD + count]


def _canaries_intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ kernel level
# (IH, IW, C, KH, KW, stride, pad_h, pad_w, bias) and the output map (OH, OW): a Dense, a SAME 3x3, stride 2 with unequal
# low-side padding whose last windows hang over the high side, a flat head with one output position, Mt = 70 (tile
# edges: three row tiles of 32 with a ragged last, one ragged column block), a 7x7 stride-2 stem
PATCH_CASES = [((1, 1, 5, 1, 1, 1, 0, 0, 1), (1, 1)), ((5, 4, 3, 3, 3, 1, 1, 1, 0), (5, 4)), ((7, 5, 2, 3, 3, 2, 1, 0, 1), (4, 3)),
               ((3, 2, 4, 3, 2, 1, 0, 0, 1), (1, 1)), ((2, 3, 70, 1, 1, 1, 0, 0, 0), (2, 3)), ((9, 9, 3, 7, 7, 2, 3, 3, 0), (5, 5))]


def _patch_args(X, n, case, out_hw, V, AV):
    IH, IW, C, KH, KW, stride, pad_h, pad_w, bias = case
    return [X.data_ptr(), n, IH, IW, C, KH, KW, stride, pad_h, pad_w, out_hw[0], out_hw[1], bias, V.data_ptr(), AV.data_ptr(),
            nv.stream_ptr()]


@pytest.mark.parametrize("case,out_hw", PATCH_CASES)
def test_patch_projection_against_float64_product(case, out_hw):
    lib = nv.load()
    IH, IW, C, KH, KW, stride, pad_h, pad_w, bias = case
    OH, OW = out_hw
    Mt = KH * KW * C + bias
    g = torch.Generator().manual_seed(sum(case) * 7 + Mt)
    V = torch.randn(Mt, Mt, generator=g, dtype=F64).to(DEV)
    for n in (1, 3):
        X = torch.randn(n, IH, IW, C, generator=g, dtype=F32).to(DEV)
        want, twin = sr.project_patches_ref(X, case[:8] + (OH, OW, bias), V)
        bound = U24 * want.abs() + 4 * (Mt + 8) * U53 * twin
        buf, AV = _guarded(n * OH * OW * Mt)
        assert lib.lip_kfac_project_patches(*_patch_args(X, n, case, out_hw, V, AV)) == 0
        torch.cuda.synchronize()
        got = AV.reshape(n * OH * OW, Mt).double().cpu()
        err = (got - want).abs()
        print(f"patches {case} n={n}: max err / bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()) and _canaries_intact(buf)
        buf2, AV2 = _guarded(n * OH * OW * Mt)
        assert lib.lip_kfac_project_patches(*_patch_args(X, n, case, out_hw, V, AV2)) == 0
        torch.cuda.synchronize()
        assert torch.equal(AV, AV2)                                                          # bitwise reproducible


@pytest.mark.parametrize("N", [1, 3, 33, 130])
def test_row_projection_against_float64_product(N):
    lib = nv.load()
    g = torch.Generator().manual_seed(N)
    Ub = torch.randn(N, N, generator=g, dtype=F64).to(DEV)
    P = 2
    for R in (1, 3, 50, 257):
        # packed probes (one launch), then a row stride and a per-probe stride larger than the row block (one per probe)
        for ldg, extra in ((N, 0), (N + 2, 7)):
            pstride = R * ldg + extra
            G = torch.randn(P * pstride, generator=g, dtype=F32).to(DEV)
            rows = torch.stack([G[p * pstride:p * pstride + R * ldg].reshape(R, ldg)[:, :N] for p in range(P)]).reshape(P * R, N)
            want, twin = sr.rows_project_ref(rows, Ub)
            bound = U24 * want.abs() + 4 * (N + 8) * U53 * twin
            buf, GU = _guarded(P * R * N)
            args = [G.data_ptr(), ldg, pstride, P, R, N, Ub.data_ptr(), GU.data_ptr(), nv.stream_ptr()]
            assert lib.lip_rows_project(*args) == 0
            torch.cuda.synchronize()
            err = (GU.reshape(P * R, N).double().cpu() - want).abs()
            print(f"rows N={N} R={R} ldg={ldg} pstride={pstride}: max err / bound {(err / bound).max().item():.3f}")
            assert bool((err <= bound).all()) and _canaries_intact(buf)
            buf2, GU2 = _guarded(P * R * N)
            args[7] = GU2.data_ptr()
            assert lib.lip_rows_project(*args) == 0
            torch.cuda.synchronize()
            assert torch.equal(GU, GU2)                                                      # bitwise reproducible


def test_projection_status_codes_leave_the_output_untouched():
    lib = nv.load()
    case, out_hw, n = (5, 4, 3, 3, 3, 1, 1, 1, 0), (5, 4), 2
    Mt = 27
    X = torch.randn(n, 5, 4, 3, dtype=F32).to(DEV)
    V = torch.randn(Mt, Mt, dtype=F64).to(DEV)
    buf, AV = _guarded(n * 20 * Mt)
    good = _patch_args(X, n, case, out_hw, V, AV)
    # null pointers; non-positive extents; a negative padding; an output map whose last window starts past the input
    for i, v in [(0, 0), (13, 0), (14, 0), (1, 0), (1, -1), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, -1), (9, -1),
                 (10, 0), (11, 0), (10, 7), (11, 6)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_project_patches(*args) == 1, (i, v)
    big = list(good)                                                     # 2^31 or more elements: refused before any launch
    big[1] = 1 << 27
    assert lib.lip_kfac_project_patches(*big) == 1
    big = list(good)
    big[4], big[5], big[6] = 1 << 12, 1 << 3, 1 << 3                     # Mt Mt >= 2^31
    assert lib.lip_kfac_project_patches(*big) == 1
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    assert lib.lip_kfac_project_patches(*good) == 0
    torch.cuda.synchronize()
    assert not bool((AV == CANARY).any()) and _canaries_intact(buf)

    P, R, N = 2, 5, 3
    G = torch.randn(P * R * N, dtype=F32).to(DEV)
    Ub = torch.randn(N, N, dtype=F64).to(DEV)
    buf, GU = _guarded(P * R * N)
    good = [G.data_ptr(), N, R * N, P, R, N, Ub.data_ptr(), GU.data_ptr(), nv.stream_ptr()]
    # null pointers; non-positive extents; a row stride below N; a per-probe stride below the row block
    for i, v in [(0, 0), (6, 0), (7, 0), (3, 0), (3, -1), (4, 0), (5, 0), (5, -2), (1, N - 1), (2, R * N - 1), (2, 0)]:
        args = list(good)
        args[i] = v
        assert lib.lip_rows_project(*args) == 1, (i, v)
    big = list(good)
    big[3], big[4], big[2] = 1 << 15, 1 << 15, 1 << 40                   # P R N >= 2^31
    assert lib.lip_rows_project(*big) == 1
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    assert lib.lip_rows_project(*good) == 0
    torch.cuda.synchronize()
    assert not bool((GU == CANARY).any()) and _canaries_intact(buf)


# ------------------------------------------------------------------------------------------------ engine level
def _worst(got, want):
    return max(_rel(a, b) for a, b in zip(got, want))


# measured on MI355X, worst over the blocks of a net of max|Lam_l - ref| / max|ref|: the sweep against the float64
# helper in the fitted basis / in the orthonormal basis / against the rows route (fitted basis):
#   sine_regressor 2.60e-7 / 3.95e-7 / 1.24e-7   xor_classifier 1.30e-7 / 8.45e-8 / 1.23e-7
#   mlp_ragged     5.78e-8 / 8.31e-8 / 6.01e-8   resnet_tiny    4.80e-7 / 3.78e-7 / 1.05e-7
#   resnet50_tiny  2.57e-7 / 4.25e-7 / 1.91e-7   flat_head      1.14e-7 / 1.37e-7 / 1.19e-7
#   stem_net       1.69e-7 / 1.88e-7 / 1.53e-7
SWEEP_TOL = 2.0e-6             # 4 x 4.80e-7
ROWS_TOL = 7.7e-7              # 4 x 1.91e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_sweep_scales_match_the_float64_helper_and_the_rows_route(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, h["alpha"], N_FULL, None)
    fitted = [(V, Ub) for V, _, Ub in fits]
    blocks, ortho = _orthonormal(h)
    worst = []
    for bases in (fitted, ortho):
        Lams = compute_ekfac_scales(state, Z, model_type, bases, moments="sweep")
        want = er.scales_ref(h["J"], h["H"], state, _cpu(bases))
        assert len(Lams) == len(blocks) == len(want)
        for b, Lam in zip(blocks, Lams):
            assert Lam.dtype == F64 and Lam.is_cuda and Lam.shape == (b.Mt, b.N) and float(Lam.min()) >= 0.0
        worst.append(_worst(Lams, want))
    Lams = compute_ekfac_scales(state, Z, model_type, fitted, moments="sweep")
    rows = compute_ekfac_scales(state, Z, model_type, fitted, moments="rows")
    e_rows = _worst(Lams, rows)
    print(f"{name}: sweep scales fitted basis {worst[0]:.2e}  orthonormal basis {worst[1]:.2e}  against the rows route {e_rows:.2e}")
    assert max(worst) <= SWEEP_TOL and e_rows <= ROWS_TOL
    again = compute_ekfac_scales(state, Z, model_type, fitted, moments="sweep")
    assert all(torch.equal(a, b) for a, b in zip(again, Lams))                               # bitwise reproducible


# measured on MI355X: identity bases against compute_ggn_diag over every block's slice, max|.| / max|diag slice|, worst
# block; and the orthonormal basis' per-block sum against the sum of that slice [either side against the helper's
# ggn_diag_ref]:
#   sine_regressor 7.14e-8 [4.19e-7], 1.03e-7 [3.50e-7]   xor_classifier 2.78e-7 [1.22e-7], 9.83e-8 [5.89e-8]
#   mlp_ragged     1.53e-7 [1.53e-7], 4.65e-8 [5.46e-8]   resnet_tiny    2.36e-7 [3.59e-7], 1.20e-7 [1.44e-7]
#   resnet50_tiny  2.86e-7 [4.16e-7], 2.06e-7 [3.41e-7]   flat_head      2.20e-7 [1.13e-7], 2.90e-8 [5.64e-8]
#   stem_net       9.45e-8 [3.25e-7], 4.91e-8 [1.19e-7]
IDENTITY_TOL = 1.7e-6          # 4 x 4.19e-7
TRACE_TOL = 1.4e-6             # 4 x 3.50e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_identity_bases_give_the_diagonal_and_orthonormal_bases_its_trace(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    blocks, ortho = _orthonormal(h)
    eye = [(torch.eye(b.Mt, device=DEV, dtype=F64), torch.eye(b.N, device=DEV, dtype=F64)) for b in blocks]
    diag = compute_ggn_diag(state, Z, model_type).double()
    scale = ref.recal(state, h["M"], model_type, None)
    Li = compute_ekfac_scales(state, Z, model_type, eye, moments="sweep")
    e_id = max(_rel(scale * Lam.reshape(-1), diag[b.off:b.off + b.Mt * b.N].cpu()) for b, Lam in zip(blocks, Li))
    e_ref = max(_rel(scale * Lam.reshape(-1), h["diag1"][b.off:b.off + b.Mt * b.N]) for b, Lam in zip(blocks, Li))
    Lo = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep")
    worst, worst_ref = 0.0, 0.0
    for b, Lam in zip(blocks, Lo):
        sl = slice(b.off, b.off + b.Mt * b.N)
        got, other, want = scale * float(Lam.sum()), float(diag[sl].sum()), float(h["diag1"][sl].sum())
        worst = max(worst, abs(got - other) / want)
        worst_ref = max(worst_ref, abs(got - want) / want, abs(other - want) / want)
    print(f"{name}: identity basis against compute_ggn_diag {e_id:.2e} [against the helper {e_ref:.2e}]  "
          f"trace against compute_ggn_diag {worst:.2e} [against the helper {worst_ref:.2e}]")
    assert e_id <= IDENTITY_TOL and e_ref <= IDENTITY_TOL and worst <= TRACE_TOL and worst_ref <= TRACE_TOL


def _reference_cotangents(h, eng, kind):
    """(spec, U (P, M, K) float64 CPU, divisor): the cotangents a spec sweeps, restated (the replay of the head sampler
    on the device's float32 probabilities; the device's own normal block for a Gaussian head)"""
    state, model_type = h["state"], h["model_type"]
    M, K = eng.n, eng.K
    g = torch.Generator().manual_seed(12)
    if kind == "mc":
        S, seed = 3, 5
        if model_type == "regressor":
            U = krylov.fill_normal(S, M * K, seed, DEV).reshape(S, M, K)
        else:
            U = torch.as_tensor(fr.replay(eng.probs().cpu().numpy(), S, seed, 0)[0])
        return MCFisher(S, seed), U.double().cpu(), float(S)
    if model_type == "regressor":
        y = torch.randn(M, K, dtype=F64, generator=g)
        logvar = float(state.params["logvar"]["logvar"])
        U = ((y.to(DEV).float() - eng.outputs()) * math.exp(-0.5 * logvar))[None]
    else:
        y = torch.randint(0, K, (M,), generator=g)
        U = (torch.nn.functional.one_hot(y, K).float().to(DEV) - eng.probs())[None]
    return EmpiricalFisher(y), U.double().cpu(), 1.0


# measured on MI355X, worst block of a net, max|Lam_l - ref| / max|ref|: exact-expectation cotangents through the raw
# sweep against the exact ('l') sweep / MCFisher(3, 5) / EmpiricalFisher against scales_from_cotangents_ref:
#   sine_regressor 0 (the same probes) / 3.49e-7 / 2.11e-7   xor_classifier 9.50e-8 / 1.63e-7 / 1.43e-7
#   mlp_ragged     6.57e-8 / 4.06e-8 / 7.51e-8               resnet_tiny    2.19e-7 / 3.81e-7 / 6.43e-7
#   resnet50_tiny  1.80e-7 / 2.20e-7 / 2.52e-7               flat_head      1.02e-7 / 2.08e-7 / 8.85e-8
#   stem_net       5.83e-8 / 1.70e-7 / 2.02e-7
EXPECTATION_TOL = 8.8e-7       # 4 x 2.19e-7
SPEC_TOL = 2.6e-6              # 4 x 6.43e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_curvature_specs_through_the_sweep(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    _, ortho = _orthonormal(h)
    eng = get_engine(state, Z, model_type)
    exact = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep")
    if model_type == "regressor":
        Ue = torch.eye(eng.K, dtype=F64)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()
    else:
        Ue = fr.exact_expectation_cotangents(eng.probs().double().cpu())
    via = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=Cotangents(Ue, 1))
    e_exp = _worst(via, exact)
    half = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=Cotangents(Ue, 2.0))
    assert _worst([2.0 * L for L in half], exact) <= EXPECTATION_TOL
    errs = {}
    for kind in ("mc", "ef"):
        spec, U, divisor = _reference_cotangents(h, eng, kind)
        got = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=spec)
        want = sr.scales_from_cotangents_ref(h["J"], U, divisor, state, _cpu(ortho))
        assert all(float(L.min()) >= 0.0 for L in got)
        errs[kind] = _worst(got, want)
        if kind == "mc":
            same = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=MCFisher(3, 5))
            other = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=MCFisher(3, 6))
            assert all(torch.equal(a, b) for a, b in zip(same, got))                         # the same seed: bitwise
            assert any(not torch.equal(a, b) for a, b in zip(other, got))                    # another seed: another estimate
    print(f"{name}: exact-expectation cotangents against the exact sweep {e_exp:.2e}  MC {errs['mc']:.2e}  "
          f"empirical Fisher {errs['ef']:.2e}")
    assert e_exp <= EXPECTATION_TOL and max(errs.values()) <= SPEC_TOL


# The float32 partial sums of a pass are grouped differently when the examples or the classes are chunked, so this is the
# float32 order of the square-sum sweep, not the 1e-12 of the rows route.  Measured on MI355X, worst block, example
# chunks / class chunks: sine_regressor 1.05e-7 / 0, xor_classifier 9.66e-8 / 9.31e-8, mlp_ragged 6.16e-8 / 9.44e-8,
# resnet_tiny 1.21e-7 / 9.89e-8, resnet50_tiny 1.35e-7 / 1.35e-7, flat_head 1.53e-7 / 1.15e-7, stem_net 1.01e-7 / 8.97e-8
# ... and MCFisher(3, 5) in example chunks / with its three probes swept as 2 + 1: sine_regressor 3.65e-8 / 1.28e-7,
# xor_classifier 1.20e-7 / 1.20e-7, mlp_ragged 8.88e-8 / 1.27e-7, resnet_tiny 8.35e-8 / 6.99e-8, resnet50_tiny 1.22e-7 /
# 7.10e-8, flat_head 1.32e-7 / 1.10e-7, stem_net 4.56e-8 / 3.34e-8
SPLIT_TOL = 6.2e-7             # 4 x 1.53e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_example_and_class_chunks_agree_with_the_unsplit_sweep(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    M, K = h["M"], h["f_new"].shape[1]
    _, ortho = _orthonormal(h)
    Lams = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep")
    Le = compute_ekfac_scales(state, Z, model_type, ortho, example_chunk=max(1, M // 2), moments="sweep")
    Lc = compute_ekfac_scales(state, Z, model_type, ortho, class_chunk=max(1, K // 2), moments="sweep")
    e_e, e_c = _worst(Le, Lams), _worst(Lc, Lams)
    # a spec in example chunks sweeps the cotangents of the same global examples, and its probes in chunks of two
    spec = MCFisher(3, 5)
    Ls = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep", curvature=spec)
    Lse = compute_ekfac_scales(state, Z, model_type, ortho, example_chunk=max(1, M // 2), moments="sweep", curvature=spec)
    Lsc = compute_ekfac_scales(state, Z, model_type, ortho, class_chunk=2, moments="sweep", curvature=spec)
    e_se, e_sc = _worst(Lse, Ls), _worst(Lsc, Ls)
    print(f"{name}: chunked sweep against unsplit  examples {e_e:.2e}  classes {e_c:.2e}  "
          f"MCFisher(3) examples {e_se:.2e}  probes 2 + 1 {e_sc:.2e}")
    assert max(e_e, e_c, e_se, e_sc) <= SPLIT_TOL


# measured on MI355X with moments="sweep", max|. - ref| / max|ref| of the posterior variance / predictive covariance
# (diag form) / mean, scalar prior (two-group prior), and |got - want| / |want| of the evidence:
#   sine_regressor 1.26e-7 / 3.20e-7 (3.20e-7) / 3.20e-7 (1.26e-7 / 3.23e-7 (3.23e-7) / 3.20e-7), 3.28e-8
#   xor_classifier 2.42e-8 / 6.34e-8 (6.34e-8) / 1.01e-7 (2.42e-8 / 6.30e-8 (6.30e-8) / 1.01e-7), 1.22e-8
#   mlp_ragged     2.38e-8 / 1.14e-7 (1.14e-7) / 2.18e-7 (1.83e-8 / 1.16e-7 (1.16e-7) / 2.18e-7), 3.18e-8
#   resnet_tiny    1.54e-7 / 4.19e-8 (4.19e-8) / 1.14e-7 (1.54e-7 / 4.00e-8 (3.96e-8) / 1.14e-7), 2.78e-8
#   resnet50_tiny  2.80e-7 / 1.25e-7 (1.24e-7) / 2.47e-7 (2.80e-7 / 1.41e-7 (1.40e-7) / 2.47e-7), 2.80e-8
#   flat_head      3.38e-8 / 8.96e-8 (7.28e-8) / 1.72e-7 (3.88e-8 / 6.60e-8 (5.72e-8) / 1.72e-7), 5.40e-9
#   stem_net       7.31e-8 / 3.69e-8 (3.69e-8) / 2.06e-7 (7.31e-8 / 3.74e-8 (3.74e-8) / 2.06e-7), 1.51e-8
VARIANCE_TOL = 1.2e-6          # 4 x 2.80e-7
PREDICT_TOL = 1.3e-6           # 4 x 3.23e-7
MEAN_TOL = 1.3e-6              # 4 x 3.20e-7
LML_TOL = 1.4e-7               # 4 x 3.28e-8


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kf.NETS)
def test_posterior_and_predictive_from_the_sweep(name, grouped):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    post = posterior_lla_ekfac(state, Z, model_type, prior, full_set_size=N_FULL, moments="sweep")
    theta = flatten_nn_params(state.params)[0]
    assert post.mean().dtype == F64 and torch.equal(post.mean().cpu(), theta.double())
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, prior, N_FULL, None, "sweep")
    bases = _cpu([(V, Ub) for V, _, Ub in fits])
    cov_blocks = er.covariance_blocks(state, bases, er.scales_ref(h["J"], h["H"], state, bases), h["recal"])
    rem = h["rem"]
    rem_var = 1.0 / (a[rem] + h["diag"][rem])
    e_var = _rel(post.variance(), kf.variance_ref(state, cov_blocks, rem, rem_var))
    K = h["f_new"].shape[1]
    cov_ref = kf.predict_dense(h["J_new"], cov_blocks, rem, rem_var)
    full = predict_lla_ekfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="full", batch=3, moments="sweep")
    mean, var = predict_lla_ekfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="diag", batch=3,
                                  moments="sweep")
    cov = torch.diagonal(full.covariance())[:, None, None] if model_type == "regressor" else full.covariance()
    var_ref = torch.diagonal(cov_ref, dim1=1, dim2=2).to(DEV)
    e_diag = ((var.reshape(5, K) - var_ref).abs().max() / cov_ref.abs().max()).item()
    e_cov = _rel(cov, cov_ref)
    e_mean = _rel(mean.reshape(5, K), h["f_new"])
    print(f"{name} {'grouped' if grouped else 'scalar'} (sweep): variance {e_var:.2e} predictive {e_cov:.2e} "
          f"(diag form {e_diag:.2e}) mean {e_mean:.2e}")
    assert e_var <= VARIANCE_TOL and e_cov <= PREDICT_TOL and e_diag <= PREDICT_TOL and e_mean <= MEAN_TOL


@pytest.mark.parametrize("name", kf.NETS)
def test_evidence_from_the_sweep(name, monkeypatch):
    h = _helper(name)
    state, Z, model_type, alpha, M = h["state"], h["Z"], h["model_type"], h["alpha"], h["M"]
    seen = []
    inner = ekfac.compute_ekfac_scales
    monkeypatch.setattr(ekfac, "compute_ekfac_scales",
                        lambda s, z, m, bases, **kw: (seen.append((bases, kw)), inner(s, z, m, bases, **kw))[1])
    got = log_marginal_likelihood_ekfac(alpha, Z, state, model_type, full_set_size=N_FULL, moments="sweep")
    assert len(seen) == 1 and seen[0][1].get("moments") == "sweep"
    spec = er.spectrum_ref(state, er.scales_ref(h["J"], h["H"], state, _cpu(seen[0][0])), model_type, h["diag1"])
    theta = flatten_nn_params(state.params)[0].double()
    want = ref.lml_ref(alpha, spec, theta.numel(), float((theta ** 2).sum()), N_FULL / M)
    e = abs(got - want) / abs(want)
    print(f"{name}: evidence (sweep) got {got:.12g} want {want:.12g} rel {e:.2e}")
    assert e <= LML_TOL
    a_fit, hist = fit_alpha_ekfac(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=20, moments="sweep")
    assert len(hist) == 20 and abs(hist[0][0] - alpha) <= 1e-14 * alpha and abs(hist[0][1] - got) <= 1e-9 * abs(got)
    assert a_fit > 0 and a_fit == a_fit and a_fit != float("inf")
    assert log_marginal_likelihood_ekfac(a_fit, Z, state, model_type, full_set_size=N_FULL, moments="sweep") >= hist[0][1]


@pytest.mark.parametrize("name", CONV_NETS)
def test_corrected_block_from_the_sweep_is_never_further_than_kfac(name):
    """the inequality of tests/test_ekfac.py with the sweep's scales: ||G_l - Q diag(recal Lam0) Q^T||_F <=
    ||G_l - c_l A_l (x) S_l||_F (1 + 1e-10) for every block, strictly by more than 1e-6 relative on a block with T_l > 1"""
    h = _helper(name)
    state, Z, model_type, M = h["state"], h["Z"], h["model_type"], h["M"]
    blocks, ortho = _orthonormal(h)
    Lams = compute_ekfac_scales(state, Z, model_type, ortho, moments="sweep")
    recal = ref.recal(state, M, model_type, None)
    strict, covered = [], []
    for b, (u, off, Mt, N, T, _), (Ut, Ub), Lam, A, S in zip(blocks, kf.blocks_of(state), _cpu(ortho), Lams, h["As"], h["Ss"]):
        assert Mt * N <= er.DENSE_CAP
        G = recal * er.exact_block(h["J"], h["H"], off, Mt, N)
        e_ek = er.frobenius_error(G, torch.kron(Ut, Ub), recal * Lam.cpu().reshape(-1))
        e_kf = float(torch.linalg.norm(G - recal / (M * T) * torch.kron(A, kf.head_factor(state, u, S, model_type))))
        nG = float(torch.linalg.norm(G))
        print(f"{name} block at {off} ({Mt}, {N}) T={T}: EKFAC (sweep) {e_ek / nG:.3e}  KFAC {e_kf / nG:.3e}  of ||G||_F")
        covered.append(T)
        assert e_ek <= e_kf * (1 + 1e-10)
        if T > 1 and e_ek < e_kf * (1 - 1e-6):
            strict.append(off)
    assert any(T > 1 for T in covered) and strict


def test_eval_dataset_probit_takes_a_curvature_spec_and_fits_once(monkeypatch):
    h = _helper("xor_classifier")
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    calls = []
    inner = ekfac.compute_ekfac_scales
    monkeypatch.setattr(ekfac, "compute_ekfac_scales", lambda *a, **kw: (calls.append(kw), inner(*a, **kw))[1])
    nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N_FULL,
                                                               model_type, posterior="ekfac", curvature=MCFisher(2, 0))
    assert len(calls) == 1 and calls[0].get("moments") == "sweep"                            # one fit for both batches
    assert probs.shape == (16, 2) and labels.shape == (16,)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), (nll, acc, brier, ece_)))
    assert bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1).abs() < 1e-9).all())
    with pytest.raises(ValueError):
        eval_dataset_probit(state, [(X, y)], Z, alpha, N_FULL, model_type, posterior="last_layer", curvature=MCFisher(2, 0))


def test_engine_method_checks_its_operands():
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    blocks = eng.kfac_blocks()
    bases = [(torch.eye(b.Mt, device=DEV, dtype=F64), torch.eye(b.N, device=DEV, dtype=F64)) for b in blocks]
    Lams = [torch.zeros(b.Mt, b.N, device=DEV, dtype=F64) for b in blocks]
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_eigen_sqsums_sweep(bases[:1], Lams)
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_eigen_sqsums_sweep(bases, Lams[:1])
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_eigen_sqsums_sweep([(bases[0][0].float(), bases[0][1]), bases[1]], Lams)
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_eigen_sqsums_sweep(bases, [Lams[0].T, Lams[1]])
    with pytest.raises(ValueError, match="class_chunk must be positive"):
        eng.kfac_eigen_sqsums_sweep(bases, Lams, class_chunk=0)
    assert all(float(Lam.abs().sum()) == 0.0 for Lam in Lams)
    # the call adds: a second pass doubles the first, bitwise (the same float64 sums added to themselves)
    eng.kfac_eigen_sqsums_sweep(bases, Lams)
    once = [Lam.clone() for Lam in Lams]
    eng.kfac_eigen_sqsums_sweep(bases, Lams)
    assert all(torch.equal(Lam, 2.0 * o) for Lam, o in zip(Lams, once))


def test_sweep_refusals_leave_the_sums_untouched():
    """``lip_vjp_eigen`` checks every op before its first launch: every refused call returns 1 and writes no Lam"""
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    lib, C = eng.lib, ctypes
    blocks = eng.kfac_blocks()
    cap = len(blocks)
    koff, ooff, Ns = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
    count, total = C.c_int32(0), C.c_int64(0)
    assert lib.lip_vjp_kron_layout(eng.h, cap, koff, ooff, Ns, C.byref(count), C.byref(total)) == 0 and count.value == cap
    order = {int(koff[i]): i for i in range(cap)}
    Vs = [torch.eye(b.Mt, device=DEV, dtype=F64) for b in blocks]
    Us = [torch.eye(b.N, device=DEV, dtype=F64) for b in blocks]
    Lams = [torch.full((b.Mt, b.N), 3.0, device=DEV, dtype=F64) for b in blocks]

    def arrays():
        Vp, Up, Lp, Mts = (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_int32 * cap)()
        for b, V, Ub, Lam in zip(blocks, Vs, Us, Lams):
            k = order[b.kernel_off]
            Vp[k], Up[k], Lp[k], Mts[k] = V.data_ptr(), Ub.data_ptr(), Lam.data_ptr(), b.Mt
        return Vp, Up, Lp, Mts

    K = eng.K
    E = torch.eye(K, device=DEV, dtype=F32)[:, None, :].expand(K, eng.n, K).contiguous()
    floats = C.c_int64(0)
    assert lib.lip_vjp_eigen_scratch(eng.h, K, C.byref(floats)) == 0 and floats.value > 0
    assert lib.lip_vjp_eigen_scratch(eng.h, 0, C.byref(floats)) == 1 and lib.lip_vjp_eigen_scratch(eng.h, K, None) == 1
    scratch = torch.empty(floats.value + 4, device=DEV, dtype=F32)
    Vp, Up, Lp, Mts = arrays()
    good = [eng.h, E.data_ptr(), Vp, Up, Lp, Mts, cap, K, nv.HEAD_L, 1.0, scratch.data_ptr(), floats.value, nv.stream_ptr()]
    # null arguments; a block count that is not the tape's; no probes; a head mode of the forward sweeps; a scratch that
    # is missing, one float short, or not 16-byte aligned
    for i, v in [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, cap - 1), (6, cap + 1), (6, 0), (7, 0),
                 (8, nv.HEAD_LT), (10, None), (11, floats.value - 1), (11, 0), (10, scratch.data_ptr() + 4)]:
        args = list(good)
        args[i] = v
        assert lib.lip_vjp_eigen(*args) == 1, (i, v)
    for which in range(4):                          # a null block operand; a row count that is not the op's KH KW C (+ 1)
        bad = list(arrays())
        if which < 3:
            bad[which][cap - 1] = None
        else:
            bad[3][0] += 2
        args = list(good)
        args[2:6] = bad
        assert lib.lip_vjp_eigen(*args) == 1, which
    torch.cuda.synchronize()
    assert all(bool((Lam == 3.0).all()) for Lam in Lams)
    assert lib.lip_vjp_eigen(*good) == 0
    torch.cuda.synchronize()
    assert all(bool((Lam >= 3.0).all()) and bool((Lam > 3.0).any()) for Lam in Lams)


# ------------------------------------------------------------------------------------------------ K = 1000
def _householder(m, g):
    """I - 2 v v^T / v^T v: dense, orthonormal, no eigensolver"""
    v = torch.randn(m, generator=g, dtype=F64).to(DEV)
    return (torch.eye(m, device=DEV, dtype=F64) - (2.0 / float(v @ v)) * torch.outer(v, v)).contiguous()


# measured on MI355X (ResNet-50, K = 1000, 64 x 64, two images, two probes): worst block of
# |Lam_l.sum() - sum of compute_ggn_diag(curvature=spec) over the slice| / that sum, and the final Dense block against its
# closed form, max|.| / max|ref|: 2.70e-8 over the 54 blocks, and 1.10e-6 (the features behind the final Dense come from
# fifty float32 layers)
R50_TRACE_TOL = 1.1e-7         # 4 x 2.70e-8
R50_DENSE_TOL = 4.4e-6         # 4 x 1.10e-6


def test_resnet50_k1000_sweep_under_a_cotangent_spec(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a D-wide row block was asked for")
    monkeypatch.setattr(LinearizedNet, "vjp_rows", refuse)
    net = ResNet50(1000, input_shape=(64, 64, 3))
    state = create_state(net, 5, dtype=F64)
    Z = torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(6), dtype=F64)
    P, divisor = 2, 2.0
    g = torch.Generator().manual_seed(8)
    U = torch.randn(P, 2, 1000, generator=g, dtype=F64)
    spec = Cotangents(U, divisor)
    blocks = get_engine(state, Z, "classifier").kfac_blocks()
    bases = [(_householder(b.Mt, g), _householder(b.N, g)) for b in blocks]
    Lams = compute_ekfac_scales(state, Z, "classifier", bases, moments="sweep", curvature=spec)
    diag = compute_ggn_diag(state, Z, "classifier", curvature=spec).double()
    worst = 0.0
    for b, Lam in zip(blocks, Lams):
        assert Lam.shape == (b.Mt, b.N) and float(Lam.min()) >= 0.0 and bool(torch.isfinite(Lam).all())
        want = float(diag[b.off:b.off + b.Mt * b.N].sum())
        worst = max(worst, abs(float(Lam.sum()) - want) / want)
    f, phit, _ = ref.features64(state, Z)
    V, Ub = _cpu(bases)[-1]
    closed = torch.einsum("ij,pil->jl", (phit @ V) ** 2, (U @ Ub) ** 2) / divisor
    e_dense = _rel(Lams[-1], closed)
    print(f"resnet50 K=1000 sweep P={P}: {len(blocks)} blocks, trace against compute_ggn_diag {worst:.2e}  "
          f"final Dense against the closed form {e_dense:.2e}")
    assert blocks[-1].final and worst <= R50_TRACE_TOL and e_dense <= R50_DENSE_TOL
