"""GPU checks of the Monte-Carlo and empirical Fisher fits: the head sampler ``lip_head_sample`` against its integer
replay (``tests/fisher_ref.py``, bitwise), then the curvature specs of ``lip_amd.fisher`` through ``compute_ggn_diag``,
``compute_kfac_factors`` and the posterior surface, on the nets of tests/test_ggn_diag.py and tests/kfac_ref.py.

Bounds.  The sampler is defined in integers: labels and cotangents are compared bitwise.  The diagonal goes through the
``lip_vjp_sqsum`` kernels whatever the cotangents are, so it keeps the bound tests/test_ggn_diag.py sets for them,
|d - ref| <= 1e-5 max(ref); chunked against unchunked keeps that file's 1e-6 max.  The Kronecker output factors keep
``FACTOR_S_TOL = 1.1e-6`` (tests/test_kfac.py:207) and the posterior variance ``VARIANCE_TOL = 1.2e-6``
(tests/test_kfac.py:262), both max|. - ref| / max|ref|.

Measured on MI355X: exact-expectation probes against the exact diagonal mlp_ragged 3.7e-8, resnet_tiny 1.6e-7,
sine_regressor 0; MC diagonal (S = 3) xor_classifier 1.2e-7, mlp_ragged 1.1e-7, resnet_tiny 1.6e-7, sine_regressor
8.7e-8; example chunks 9.9e-8; empirical Fisher 4.9e-8 / 5.8e-8 / 5.7e-8; MC output factors (S = 4) resnet_tiny 3.0e-7,
mlp_ragged 4.9e-8; KFAC variance from exact-expectation cotangents 6.9e-8 / 1.4e-8; ResNet-50, K = 1000, S = 4: 1.6e-7.
"""
import functools
import math

import numpy as np
import pytest
import torch

import fisher_ref as fr
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import kfac, krylov
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.fisher import Cotangents, EmpiricalFisher, MCFisher, sample_head_cotangents
from lip_amd.ggn import clear_engine_cache, compute_ggn_diag, compute_kfac_factors, get_engine
from lip_amd.lla import posterior_lla_diag, posterior_lla_kfac, predict_lla_diag
from lip_amd.scalemodels import ResNet50
from lip_amd.toymodels import create_state
from test_ggn_diag import _cases as diag_cases

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
DIAG_TOL = 1e-5                # tests/test_ggn_diag.py: |d - ref| <= 1e-5 max(ref)
CHUNK_TOL = 1e-6               # tests/test_ggn_diag.py::test_example_chunks_agree_and_halves_average
FACTOR_S_TOL = 1.1e-6          # tests/test_kfac.py:207
VARIANCE_TOL = 1.2e-6          # tests/test_kfac.py:262
LIP_ERR_ARG = 1
FILL = 12345.0                 # canary value of the words a call must not write
SEEDS = (0, 1234, 2 ** 63 + 11)
OFFSETS = (0, 5, 2 ** 31 + 3)


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ the sampler
def _rows(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(8.0 * torch.randn(n, K, generator=g), dim=-1).float().contiguous()


def _special_rows(K, seed):
    """(5, K): exact zeros at the front, exact zeros at the tail, one-hot, a row whose float32 sum is not 1, a plain row"""
    p = _rows(5, K, seed)
    z = max(1, K // 4)
    p[0, :z] = 0.0
    p[0] /= p[0].sum()
    p[1, K - z:] = 0.0
    p[1] /= p[1].sum()
    p[2] = 0.0
    p[2, K // 2] = 1.0
    for s in range(seed + 1, seed + 200):                          # softmax rows rarely sum to 1 exactly in float32
        cand = _rows(1, K, s)[0]
        if float(cand.sum(dtype=torch.float32)) != 1.0:
            p[3] = cand
            break
    assert bool((p[0, :z] == 0).all()) and bool((p[1, K - z:] == 0).all()) and float(p[2].max()) == 1.0
    assert float(p[3].sum(dtype=torch.float32)) != 1.0
    assert abs(float(p[3].sum(dtype=torch.float32)) - 1.0) <= 4 * 2.0 ** -24 * math.ceil(math.log2(K) + 1)
    return p.contiguous()


def _sample(lib, p_dev, S, seed, off, with_labels=True, misalign=0):
    """one call on canary-filled buffers -> (U (S, n, K) numpy, labels (S, n) numpy or None); asserts the status and that
    the words before and after U and after the labels are untouched"""
    n, K = p_dev.shape
    tot, guard = S * n * K, 64
    start = 4 + misalign                                           # floats: U starts `misalign` floats past a 16-byte boundary
    buf = torch.full((start + tot + guard,), FILL, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    U = buf[start:start + tot]
    assert (U.data_ptr() % 16 == 0) == (misalign % 4 == 0)
    lab = torch.full((S * n + guard,), -77, device=DEV, dtype=torch.int32) if with_labels else None
    rc = lib.lip_head_sample(nv.ptr(p_dev), n, K, S, seed, off, U.data_ptr(), nv.ptr(lab), nv.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.lip_last_error()
    host = buf.cpu()
    assert bool((host[:start] == FILL).all()) and bool((host[start + tot:] == FILL).all()), "a word outside U was written"
    labels = None
    if with_labels:
        lh = lab.cpu()
        assert bool((lh[S * n:] == -77).all()), "a word after the labels was written"
        labels = lh[:S * n].reshape(S, n).numpy()
    return host[start:start + tot].reshape(S, n, K).numpy(), labels


def _assert_equals_replay(lib, p, S, seed, off, **kw):
    U, labels = _sample(lib, p.to(DEV), S, seed, off, **kw)
    U_ref, lab_ref = fr.replay(p.numpy(), S, seed, off)
    if labels is not None:
        assert np.array_equal(labels, lab_ref), f"labels differ at {np.argwhere(labels != lab_ref)[:4].tolist()}"
    assert np.array_equal(U.view(np.int32), U_ref.view(np.int32)), "U is not bitwise float32(onehot) - p"


SHAPES = [(1, 1, 1), (3, 2, 5), (2, 63, 65), (2, 64, 3), (3, 65, 4), (2, 257, 2), (1, 1000, 70), (2, 8192, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"n{n}-K{K}-S{S}" for n, K, S in SHAPES])
def test_sampler_equals_replay(shape):
    n, K, S = shape
    lib = nv.load()
    p = _rows(n, K, 100 + K)
    for seed in SEEDS:
        for off in OFFSETS:
            _assert_equals_replay(lib, p, S, seed, off)
    _assert_equals_replay(lib, p, S, 1234, 5, with_labels=False)       # labels = NULL is accepted


@pytest.mark.parametrize("K", [5, 64, 257, 1000])
def test_sampler_equals_replay_on_special_rows(K):
    """rows with exact zeros at the front / at the tail, a one-hot row, a row whose float32 sum differs from 1"""
    lib = nv.load()
    p = _special_rows(K, 7 * K)
    for seed, off in zip(SEEDS, OFFSETS):
        _assert_equals_replay(lib, p, 300, seed, off)                  # 300 draws: more than one round of a block
    _, labels = _sample(lib, p.to(DEV), 300, 3, 0)
    z = max(1, K // 4)
    assert labels[:, 0].min() >= z and labels[:, 1].max() < K - z and bool((labels[:, 2] == K // 2).all())


@pytest.mark.parametrize("n,K,S,misalign", [(2, 64, 3, 1), (3, 65, 4, 0), (3, 65, 4, 3), (2, 1000, 5, 1), (2, 6, 70, 2)],
                         ids=["K64-off1", "K65-aligned", "K65-off3", "K1000-off1", "K6-off2"])
def test_sampler_dword_path_and_canaries(n, K, S, misalign):
    """a U one float past a 16-byte boundary and a K that is no multiple of 4 take the dword stores; the words around U
    stay as they were (checked by ``_sample``)"""
    _assert_equals_replay(nv.load(), _rows(n, K, 9), S, 1234, 5, misalign=misalign)


def test_sampler_dead_rows_get_label_minus_one():
    lib = nv.load()
    p = _rows(3, 6, 1)
    p[0] = 0.0
    p[1, 2] = float("nan")
    p[1, 4] = float("inf")
    U, labels = _sample(lib, p.to(DEV), 9, 4, 0)
    U_ref, lab_ref = fr.replay(p.numpy(), 9, 4, 0)
    assert bool((labels[:, :2] == -1).all()) and bool((labels[:, 2] >= 0).all()) and np.array_equal(labels, lab_ref)
    assert np.array_equal(U.view(np.int32)[:, 0], U_ref.view(np.int32)[:, 0])
    assert np.array_equal(np.isnan(U), np.isnan(U_ref)) and np.array_equal(U[~np.isnan(U)], U_ref[~np.isnan(U_ref)])


def test_sampler_chunk_invariance():
    lib = nv.load()
    p = _rows(7, 65, 21)
    whole, lab = _sample(lib, p.to(DEV), 5, 77, 11)
    for a, b in ((0, 3), (2, 5), (6, 7)):
        part, lab_p = _sample(lib, p[a:b].contiguous().to(DEV), 5, 77, 11 + a)
        assert np.array_equal(part.view(np.int32), whole[:, a:b].view(np.int32)) and np.array_equal(lab_p, lab[:, a:b])
    U, labels = sample_head_cotangents(p.to(DEV), 5, 77, example_offset=11, return_labels=True)
    assert U.shape == (5, 7, 65) and labels.dtype == torch.int32
    assert np.array_equal(U.cpu().numpy().view(np.int32), whole.view(np.int32)) and np.array_equal(labels.cpu().numpy(), lab)
    assert torch.equal(sample_head_cotangents(p.to(DEV), 5, 77, 11), U)


def test_sampler_refusals_write_nothing():
    lib = nv.load()
    p = _rows(2, 8, 3).to(DEV)
    big = torch.zeros(8193, device=DEV)
    U = torch.full((4 * 2 * 8,), FILL, device=DEV)
    lab = torch.full((4 * 2,), -77, device=DEV, dtype=torch.int32)
    st = nv.stream_ptr()
    calls = [(nv.ptr(big), 1, 8193, 1, 0, 0, nv.ptr(U), None),                  # K = 8193
             (nv.ptr(p), 2, 8, 0, 0, 0, nv.ptr(U), nv.ptr(lab)),                # S = 0
             (nv.ptr(p), 0, 8, 4, 0, 0, nv.ptr(U), nv.ptr(lab)),                # n = 0
             (nv.ptr(p), 2, 0, 4, 0, 0, nv.ptr(U), nv.ptr(lab)),                # K = 0
             (None, 2, 8, 4, 0, 0, nv.ptr(U), nv.ptr(lab)),                     # probs = NULL
             (nv.ptr(p), 2, 8, 4, 0, 0, None, nv.ptr(lab)),                     # U = NULL
             (nv.ptr(p), 2, 8, 4, 0, -1, nv.ptr(U), nv.ptr(lab)),               # example_offset = -1
             (nv.ptr(p), 2, 8, 4, 0, 2 ** 32 - 1, nv.ptr(U), nv.ptr(lab))]      # example_offset + n > 2^32
    for args in calls:
        assert lib.lip_head_sample(*args, st) == LIP_ERR_ARG, args
        assert b"lip_head_sample" in lib.lip_last_error()
    torch.cuda.synchronize()
    assert bool((U == FILL).all()) and bool((lab == -77).all())
    assert lib.lip_head_sample(nv.ptr(p), 2, 8, 4, 0, 2 ** 32 - 2, nv.ptr(U), nv.ptr(lab), st) == 0    # the last legal offset
    torch.cuda.synchronize()
    assert bool((U != FILL).all())


# ------------------------------------------------------------------------------------------------ the diagonal
@functools.lru_cache(maxsize=None)
def _diag_case(name):
    """the net of tests/test_ggn_diag.py with its float64 outputs, probabilities and Jacobian, built once, never written"""
    net, Z, model_type = diag_cases()[name]
    state = create_state(net, 3, dtype=F64, logvar=-0.3)
    f, J = ref.jac64(state, Z, model_type)
    return dict(state=state, Z=Z, model_type=model_type, f=f, J=J, p=torch.softmax(f, dim=-1), N=7 * Z.shape[0] + 5)


def _max_err(d, r):
    return ((d.double().cpu() - r.cpu()).abs().max() / r.abs().max()).item()


@pytest.mark.parametrize("name", ["mlp_ragged", "resnet_tiny", "sine_regressor"])
def test_exact_expectation_probes_reproduce_the_exact_diagonal(name):
    """U[k, i] = sqrt(p_ik) (e_k - p_i) (identity probes for the regressor) sum to the head Hessian: the raw route with
    every normalisation, no randomness"""
    c = _diag_case(name)
    state, Z, model_type, N = c["state"], c["Z"], c["model_type"], c["N"]
    exact = compute_ggn_diag(state, Z, model_type, full_set_size=N)
    eng = get_engine(state, Z, model_type)
    if model_type == "regressor":
        U = torch.eye(eng.K, dtype=F64)[:, None, :].expand(eng.K, eng.n, eng.K).contiguous()
    else:
        U = fr.exact_expectation_cotangents(eng.probs().double().cpu())
    d = compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=Cotangents(U, 1))
    torch.cuda.synchronize()
    err = _max_err(d, exact.double())
    print(f"{name}: exact-expectation probes against the exact diagonal: {err:.2e}")
    assert d.dtype == torch.float32 and d.is_cuda and err <= DIAG_TOL
    half = compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=Cotangents(U, 2.0))
    assert _max_err(2.0 * half, exact.double()) <= DIAG_TOL


def _mc_reference_cotangents(c, eng, S, seed):
    """(S, M, K) float64 cotangents of MCFisher(S, seed): the replayed labels of the device's float32 probabilities with
    the float64 probabilities of the reference forward (classifier), the device's own normal block (regressor)"""
    M, K = c["f"].shape
    if c["model_type"] == "regressor":
        return krylov.fill_normal(S, M * K, seed, DEV).reshape(S, M, K).double().cpu()
    labels = torch.as_tensor(fr.replay_labels(eng.probs().cpu().numpy(), S, seed, 0)).long()
    return torch.nn.functional.one_hot(labels, K).double() - c["p"][None]


@pytest.mark.parametrize("name", ["xor_classifier", "mlp_ragged", "resnet_tiny", "sine_regressor"])
def test_mc_diagonal_matches_the_float64_reference(name):
    c = _diag_case(name)
    state, Z, model_type, N = c["state"], c["Z"], c["model_type"], c["N"]
    S, seed = 3, 5
    d = compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=MCFisher(S, seed))
    U = _mc_reference_cotangents(c, get_engine(state, Z, model_type), S, seed)
    want = fr.diag_ref(state, Z, model_type, U, S, N, J=c["J"])
    torch.cuda.synchronize()
    err = _max_err(d, want)
    print(f"{name}: MC diagonal S={S} against float64: D={want.numel()} max|d - ref| / max ref = {err:.2e}")
    assert bool(torch.isfinite(d).all()) and bool((d >= 0).all()) and err <= DIAG_TOL


@pytest.mark.parametrize("chunk", [3, 4])
def test_mc_diagonal_example_chunks_agree(chunk):
    """chunks of 3 + 3 and of 4 + 2 examples draw what the single binding draws (``example_offset`` = the chunk's start)"""
    net, Z, model_type = diag_cases()["resnet_small"]
    state = create_state(net, 3, dtype=F64)
    spec = MCFisher(3, 9)
    whole = compute_ggn_diag(state, Z, model_type, full_set_size=1000, curvature=spec)
    chunked = compute_ggn_diag(state, Z, model_type, full_set_size=1000, example_chunk=chunk, curvature=spec)
    other = compute_ggn_diag(state, Z, model_type, full_set_size=1000, curvature=MCFisher(3, 10))
    torch.cuda.synchronize()
    scale = whole.abs().max()
    err = ((chunked - whole).abs().max() / scale).item()
    print(f"resnet_small: MC diagonal in example chunks of {chunk} against one binding: {err:.2e}")
    assert err <= CHUNK_TOL
    assert ((other - whole).abs().max() / scale).item() > 1e-3            # another seed is another estimate


@pytest.mark.parametrize("name", ["xor_classifier", "mlp_ragged", "sine_regressor"])
def test_empirical_fisher_diagonal(name):
    c = _diag_case(name)
    state, Z, model_type, N = c["state"], c["Z"], c["model_type"], c["N"]
    M, K = c["f"].shape
    g = torch.Generator().manual_seed(12)
    logvar = float(state.params["logvar"]["logvar"]) if model_type == "regressor" else 0.0
    if model_type == "regressor":
        y = torch.randn(M, K, dtype=F64, generator=g)
        U = ((y - c["f"]) * math.exp(-0.5 * logvar))[None]
    else:
        y = torch.randint(0, K, (M,), generator=g)
        U = (torch.nn.functional.one_hot(y, K).double() - c["p"])[None]
    d = compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=EmpiricalFisher(y))
    want = fr.diag_ref(state, Z, model_type, U, 1, N, J=c["J"])
    err = _max_err(d, want)
    print(f"{name}: empirical Fisher diagonal against float64: {err:.2e}")
    assert err <= DIAG_TOL
    # ... and it is the raw square-sum sweep called by hand
    eng = get_engine(state, Z, model_type)
    if model_type == "regressor":
        Uh = ((y.to(DEV).float() - eng.outputs()) * math.exp(-0.5 * logvar))[None]
    else:
        Uh = (torch.nn.functional.one_hot(y, K).float().to(DEV) - eng.probs())[None]
    hand = eng.vjp_sqsum(Uh.contiguous(), "raw") * ref.recal(state, M, model_type, N)
    torch.cuda.synchronize()
    assert ((hand - d).abs().max() / d.abs().max()).item() <= CHUNK_TOL
    chunked = compute_ggn_diag(state, Z, model_type, full_set_size=N, example_chunk=max(1, M // 2 - 1),
                               curvature=EmpiricalFisher(y))
    assert ((chunked - d).abs().max() / d.abs().max()).item() <= CHUNK_TOL


# ------------------------------------------------------------------------------------------------ KFAC
@functools.lru_cache(maxsize=None)
def _kfac_case(name):
    state, Z, model_type = kf.make_case(name)
    f, ats, Gs = kf.patches_and_cotangents(state, Z)
    As, Ss, M = kf.factors_from(f, ats, Gs, model_type)
    return dict(state=state, Z=Z, model_type=model_type, f=f, Gs=Gs, p=torch.softmax(f, dim=-1), M=M,
                alpha=kf.alpha_for(state, As, Ss, M, model_type, kf.N_FULL))


def _rel(v, r):
    r = r.to(v.device)
    return ((v.double() - r).abs().max() / r.abs().max()).item()


@pytest.mark.parametrize("name", ["resnet_tiny", "mlp_ragged"])        # conv blocks with BN; an MLP
def test_kfac_output_factors_of_mc_fisher(name):
    c = _kfac_case(name)
    state, Z, model_type = c["state"], c["Z"], c["model_type"]
    S, seed = 4, 3
    blocks, As, Ss, M = compute_kfac_factors(state, Z, model_type, curvature=MCFisher(S, seed))
    _, As0, _, _ = compute_kfac_factors(state, Z, model_type)
    assert all(torch.equal(A, A0) for A, A0 in zip(As, As0))           # the input factors do not see the spec
    eng = get_engine(state, Z, model_type)
    labels = torch.as_tensor(fr.replay_labels(eng.probs().cpu().numpy(), S, seed, 0)).long()
    U = torch.nn.functional.one_hot(labels, eng.K).double() - c["p"][None]
    want = fr.kfac_output_factors_ref(state, Z, U, S, Gs=c["Gs"])
    e_s = max(_rel(Sl, Sr) for Sl, Sr in zip(Ss, want))
    print(f"{name}: MC output factors S={S} against float64, worst block: {e_s:.2e}")
    assert M == c["M"] and len(Ss) == len(want) and all(torch.equal(Sl, Sl.T) for Sl in Ss)
    assert e_s <= FACTOR_S_TOL
    _, Ae, Se, _ = compute_kfac_factors(state, Z, model_type, example_chunk=max(1, M // 2), curvature=MCFisher(S, seed))
    assert max(_rel(a, b) for a, b in zip(Se, Ss)) <= 1e-12            # SPLIT_TOL of tests/test_kfac.py: float64 regrouping
    _, _, Sc, _ = kfac.compute_kfac_factors(state, Z, model_type, class_chunk=3, curvature=MCFisher(S, seed))
    assert max(_rel(a, b) for a, b in zip(Sc, Ss)) <= 1e-12            # the four probes swept as 3 + 1


@pytest.mark.parametrize("name", ["resnet_tiny", "mlp_ragged"])
def test_kfac_posterior_of_exact_expectation_cotangents(name):
    c = _kfac_case(name)
    state, Z, model_type, alpha = c["state"], c["Z"], c["model_type"], c["alpha"]
    exact = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=kf.N_FULL).variance()
    eng = get_engine(state, Z, model_type)
    U = fr.exact_expectation_cotangents(eng.probs().double().cpu())
    got = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=kf.N_FULL, curvature=Cotangents(U, 1)).variance()
    err = _rel(got, exact)
    print(f"{name}: KFAC variance from exact-expectation cotangents against the exact fit: {err:.2e}")
    assert err <= VARIANCE_TOL


# ------------------------------------------------------------------------------------------------ K = 1000
def test_resnet50_k1000_mc_diagonal_against_rows():
    """four probes where tests/test_ggn_diag.py::test_resnet50_k1000_subset_against_rows needs 1000"""
    net = ResNet50(1000, input_shape=(64, 64, 3))
    state = create_state(net, 5, dtype=torch.float32)
    Z = torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(6)).cuda()
    S = 4
    d = compute_ggn_diag(state, Z, "classifier", curvature=MCFisher(S, 1))
    eng = get_engine(state, Z, "classifier")
    assert bool(torch.isfinite(d).all()) and bool((d >= 0).all())
    U, labels = sample_head_cotangents(eng.probs(), S, 1, return_labels=True)
    assert np.array_equal(labels.cpu().numpy(), fr.replay_labels(eng.probs().cpu().numpy(), S, 1, 0))
    idx = torch.randperm(eng.D, generator=torch.Generator().manual_seed(7))[:4096].cuda()
    rows = eng.vjp_rows(U, "raw")
    want = (rows[:, :, idx].double() ** 2).sum((0, 1)) / S
    del rows
    torch.cuda.synchronize()
    err = ((d[idx].double() - want).abs().max() / want.abs().max()).item()
    print(f"resnet50 K=1000 MC S={S}: D={eng.D} subset max|d - ref| / max ref = {err:.2e}")
    assert err <= DIAG_TOL


# ------------------------------------------------------------------------------------------------ the posterior surface
def _finite(*vals):
    return all(v == v and abs(v) != float("inf") for v in vals)


def test_posterior_surface_and_fit_cache(monkeypatch):
    c = _kfac_case("xor_classifier")
    state, Z, model_type, alpha, N = c["state"], c["Z"], c["model_type"], c["alpha"], kf.N_FULL
    spec = MCFisher(3, 2)
    d_mc = compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=spec)
    post = posterior_lla_diag(state, Z, model_type, alpha, full_set_size=N, curvature=spec)
    assert torch.allclose(post.variance(), 1.0 / (alpha + d_mc), rtol=1e-6, atol=0)
    assert torch.equal(d_mc, compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=MCFisher(3, 2)))
    assert not torch.equal(d_mc, compute_ggn_diag(state, Z, model_type, full_set_size=N, curvature=MCFisher(3, 4)))

    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    mean, var = predict_lla_diag(state, X, Z, model_type, alpha, full_set_size=N, curvature=spec)
    assert mean.shape == var.shape == (16, 2) and bool(torch.isfinite(var).all()) and bool((var >= 0).all())
    for posterior in ("diag", "kfac"):
        nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N,
                                                                   model_type, posterior=posterior, curvature=spec)
        assert _finite(nll, acc, brier, ece_) and probs.shape == (16, 2) and bool(torch.isfinite(probs).all())
    with pytest.raises(ValueError):
        eval_dataset_probit(state, [(X, y)], Z, alpha, N, model_type, posterior="last_layer", curvature=spec)
    with pytest.raises(ValueError):
        compute_ggn_diag(state, Z, model_type, curvature=EmpiricalFisher(y))          # 16 labels for 32 examples

    # the one-entry fit cache: the same seed is a hit (bitwise the same posterior), another seed is another fit
    clear_engine_cache()
    fits = []
    inner = kfac._fit
    monkeypatch.setattr(kfac, "_fit", lambda *a, **kw: (fits.append(1), inner(*a, **kw))[1])
    v1 = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N, curvature=MCFisher(3, 2)).variance()
    v2 = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N, curvature=MCFisher(3, 2)).variance()
    assert len(fits) == 1 and torch.equal(v1, v2)
    v3 = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N, curvature=MCFisher(3, 4)).variance()
    assert len(fits) == 2 and not torch.equal(v1, v3)
    v0 = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N).variance()
    assert len(fits) == 3 and not torch.equal(v0, v1)
    clear_engine_cache()
    v1b = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N, curvature=MCFisher(3, 2)).variance()
    assert len(fits) == 4 and torch.equal(v1, v1b)                      # a fresh binding draws the same labels


def test_curvature_none_is_the_exact_route_bitwise():
    c = _kfac_case("xor_classifier")
    state, Z, model_type, alpha, N = c["state"], c["Z"], c["model_type"], c["alpha"], kf.N_FULL
    for kw in ({"curvature": None}, {"curvature": "ggn"}):
        assert torch.equal(compute_ggn_diag(state, Z, model_type, full_set_size=N, **kw),
                           compute_ggn_diag(state, Z, model_type, full_set_size=N))
        _, As, Ss, _ = compute_kfac_factors(state, Z, model_type, **kw)
        _, As0, Ss0, _ = compute_kfac_factors(state, Z, model_type)
        assert all(torch.equal(a, b) for a, b in zip(As + Ss, As0 + Ss0))
        clear_engine_cache()
        v = posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N, **kw).variance()
        clear_engine_cache()
        assert torch.equal(v, posterior_lla_kfac(state, Z, model_type, alpha, full_set_size=N).variance())
        assert torch.equal(posterior_lla_diag(state, Z, model_type, alpha, full_set_size=N, **kw).variance(),
                           posterior_lla_diag(state, Z, model_type, alpha, full_set_size=N).variance())
