"""GPU checks of the Monte-Carlo softmax link: ``lip_link_mc`` and ``lip_link_chol`` against their float64 replay
(tests/link_ref.py), then ``link_predictive``, ``eval_dataset_closed_form`` and ``auroc_ood_closed_form`` on the small
nets of tests/kfac_ref.py.

Bounds.  The kernel draws, scales and exponentiates in float32; the replay does the same draws in float64.  A
probability moves by at most delta / 2 when the logits move by at most delta, and per case

    delta = max_k [ sum_j |L_kj| e_eps + 2^-23 (|m_k| + 5.89 sum_j |L_kj|) (K_row + 2) ],

e_eps = K_FILL_NORMAL 2^-24 5.89 the project's measured Box-Muller bound (tests/test_krylov_ops.py:30) at the largest
radius sqrt(50 ln 2) = 5.89, K_row the non-zeros of the row of L (the variance form: L = diag(sd), K_row = 1); the
float32 softmax adds 2^-22:  max |probs - replay| <= delta / 2 + 2^-22,  and ``mean_entropy`` gets the same bound times
1 + max_k |log p_k| over the replay's per-draw probabilities above 2^-24.  ``lip_link_chol``: max |L - ref| <= 2^-23
max |ref| (one rounding to float32 plus a margin of one ulp); zero columns and flags match exactly.  Everything else is
bitwise.

Measured on MI355X (``-s`` prints every case): worst ratio to the derived bound over all shapes, seeds and offsets 0.007
for the probabilities (variances, K = 9; |probs - replay| at most 1.0e-7 anywhere) and 0.002 for the entropy (variances,
K = 8192; at most 4.7e-7): the bound is dominated by its Box-Muller term, a worst case at the largest radius.
``lip_link_chol``: at most 0.47 of 2^-23 max |ref| (K = 2).  Surface: xor_classifier diagonal 3.1e-8 against 2.2e-5,
resnet_tiny full KFAC covariance 4.8e-8 against 1.4e-4.  (Figures printed with the lane -> wave switch at K = 32, before
the K = 48 | 49 shapes were added; with the switch at 48 every shape passes, figures not re-printed.)
"""
import functools
import math

import numpy as np
import pytest
import torch

import kfac_ref as kf
import link_ref as lr
from lip_amd import _native as nv
from lip_amd.distributions import MultivariateNormalFullCovariance
from lip_amd.evaluate import (auroc_ood_closed_form, eval_dataset_closed_form, eval_dataset_probit, ood_scores, roc_auc)
from lip_amd.ggn import clear_engine_cache
from lip_amd.link import cholesky_semidefinite, link_predictive
from lip_amd.lla import predict_lla_diag, predict_lla_kfac
from test_krylov_ops import K_FILL_NORMAL

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
LIP_ERR_ARG = 1
FILL = 12345.0                 # canary value of the words a call must not write
GUARD = 16
RAD_MAX = 5.89                 # sqrt(50 ln 2): the largest Box-Muller radius, u1 = 2^-25
E_EPS = K_FILL_NORMAL * 2.0 ** -24 * RAD_MAX
RUNS = ((0, 0), (2 ** 63 + 11, 2 ** 31 + 3))       # (seed, example_offset)
N_FULL = kf.N_FULL


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ inputs and calls
def _psd(rng, K, kind):
    if kind == "zero":
        return np.zeros((K, K))
    if kind == "rank1":
        v = rng.uniform(-1.5, 1.5, K)
        return np.outer(v, v)
    A = rng.standard_normal((K, 2 * K)) * (1.2 / math.sqrt(2 * K))     # row norms about 1.2: logit spreads like sd in [0, 2]
    return A @ A.T


@functools.lru_cache(maxsize=None)
def _inputs(n, K, factor):
    """(mean (n, K) float64, var (n, K) float64 or None, L (n, K, K) float32 or None): means uniform in [-8, 8]; standard
    deviations in [0, 2] with exact zeros; factors of random PSD matrices, the second one rank 1, the third all zero"""
    rng = np.random.default_rng(1000 * K + n + (7 if factor else 0))
    mean = rng.uniform(-8.0, 8.0, (n, K))
    if not factor:
        sd = rng.uniform(0.0, 2.0, (n, K))
        sd[rng.uniform(size=(n, K)) < 0.2] = 0.0
        sd[0, 0] = 0.0
        return mean, sd * sd, None
    kinds = ["full", "rank1", "zero"]
    L = np.stack([lr.cholesky_semidefinite(_psd(rng, K, kinds[i % 3]))[0] for i in range(n)]).astype(np.float32)
    return mean, None, L


def _dev(x, dtype):
    return None if x is None else torch.as_tensor(x, dtype=dtype).contiguous().to(DEV)


def _guarded(count, dtype, fill):
    buf = torch.full((GUARD + count + GUARD,), fill, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + count]


def _assert_guards(buf, count, fill, what):
    host = buf.cpu()
    assert bool((host[:GUARD] == fill).all()) and bool((host[GUARD + count:] == fill).all()), f"a word outside {what} was written"


def _mc(mean, var, L, S, seed, off, entropy=True):
    """one call on canary-guarded buffers -> (probs (n, K), mean_entropy (n,) or None, flags (n,)) numpy"""
    lib = nv.load()
    n, K = mean.shape
    m, v, Lf = _dev(mean, F64), _dev(var, F64), _dev(L, torch.float32)
    pb, probs = _guarded(n * K, F64, FILL)
    eb, ent = _guarded(n, F64, FILL)
    fb, flags = _guarded(n, torch.int32, -77)
    rc = lib.lip_link_mc(nv.ptr(m), nv.ptr(v), nv.ptr(Lf), n, K, S, seed, off, probs.data_ptr(),
                         ent.data_ptr() if entropy else None, flags.data_ptr(), nv.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.lip_last_error()
    _assert_guards(pb, n * K, FILL, "probs")
    _assert_guards(fb, n, -77, "flags")
    if entropy:
        _assert_guards(eb, n, FILL, "mean_entropy")
    else:
        assert bool((eb == FILL).all()), "a null mean_entropy was written"
    return probs.cpu().numpy().reshape(n, K), ent.cpu().numpy() if entropy else None, flags.cpu().numpy()


def _bounds(mean, var, L, p_draws):
    """(bound on |probs - replay|, bound on |mean_entropy - replay|), derived from the inputs (module docstring)"""
    if L is None:
        sumabs = np.sqrt(var)
        k_row = np.ones_like(sumabs)
    else:
        low = np.tril(L.astype(np.float64))
        sumabs, k_row = np.abs(low).sum(-1), np.maximum((low != 0).sum(-1), 1)
    delta = (sumabs * E_EPS + 2.0 ** -23 * (np.abs(mean) + RAD_MAX * sumabs) * (k_row + 2)).max()
    tol = delta / 2 + 2.0 ** -22
    big = p_draws[p_draws > 2.0 ** -24]
    return tol, tol * (1.0 + np.abs(np.log(big)).max())


def _check_shape(n, K, S, factor):
    mean, var, L = _inputs(n, K, factor)
    worst_p = worst_h = 0.0
    for seed, off in RUNS:
        probs, ent, flags = _mc(mean, var, L, S, seed, off)
        p_ref, h_ref, p_draws = lr.replay(mean, var=var, L=L, S=S, seed=seed, example_offset=off, return_draws=True)
        tol_p, tol_h = _bounds(mean, var, L, p_draws)
        assert not flags.any() and np.isfinite(probs).all() and np.isfinite(ent).all()
        e_p, e_h = np.abs(probs - p_ref).max(), np.abs(ent - h_ref).max()
        worst_p, worst_h = max(worst_p, e_p / tol_p), max(worst_h, e_h / tol_h)
        print(f"STAT link_mc {'factor' if factor else 'diag'} n{n} K{K} S{S} seed {seed} off {off}: probs {e_p:.3g} / {tol_p:.3g} = "
              f"{e_p / tol_p:.3f}, entropy {e_h:.3g} / {tol_h:.3g} = {e_h / tol_h:.3f}")
        assert e_p <= tol_p, f"probs: {e_p:.4g} above the derived bound {tol_p:.4g}"
        assert e_h <= tol_h, f"mean_entropy: {e_h:.4g} above the derived bound {tol_h:.4g}"
        assert np.abs(probs.sum(-1) - 1.0).max() <= 2.0 ** -20
        again = _mc(mean, var, L, S, seed, off)                            # two runs are identical
        assert np.array_equal(again[0].view(np.int64), probs.view(np.int64)) and np.array_equal(again[1].view(np.int64), ent.view(np.int64))
        without = _mc(mean, var, L, S, seed, off, entropy=False)           # mean_entropy = NULL is accepted
        assert without[1] is None and np.array_equal(without[0].view(np.int64), probs.view(np.int64))
        if n > 1:                                                          # rows [1, n) at example_offset + 1
            part = _mc(mean[1:], None if var is None else var[1:], None if L is None else L[1:], S, seed, off + 1)
            assert np.array_equal(part[0].view(np.int64), probs[1:].view(np.int64))
            assert np.array_equal(part[1].view(np.int64), ent[1:].view(np.int64))
    return worst_p, worst_h


# the issue's shapes, then the K just below and just above every switch of the launcher: lane-per-draw register tiles
# 4 | 8 | 16 | 32 | 33, lane -> wave per draw at 48 | 49 (16-lane groups), 64 | 65 (32-lane), 128 | 129 (64-lane), quads per lane
# 256 | 257, 512 | 513, 1024 | 1025, wave -> block per draw 2048 | 2049, 4096 | 4097; S beyond one round of each geometry
DIAG_SHAPES = [(1, 1, 1), (3, 2, 5), (2, 10, 64), (2, 10, 65), (2, 63, 7), (2, 257, 6), (1, 1000, 70), (2, 8192, 3),
               (2, 4, 5), (2, 5, 5), (2, 8, 5), (2, 9, 5), (2, 16, 5), (2, 17, 5), (2, 32, 70), (2, 33, 70), (2, 48, 70), (2, 49, 70), (2, 64, 9),
               (2, 65, 9), (2, 128, 5), (2, 129, 5), (2, 256, 5), (2, 512, 3), (2, 513, 3), (1, 1024, 3), (1, 1025, 3),
               (1, 2048, 3), (1, 2049, 3), (1, 4096, 2), (1, 4097, 2), (1, 10, 300)]
FACTOR_SHAPES = [(3, 2, 5), (2, 10, 65), (2, 31, 9), (1, 64, 130),
                 (2, 4, 5), (2, 5, 5), (2, 8, 5), (2, 9, 5), (2, 16, 5), (2, 17, 5), (2, 32, 5), (2, 33, 5), (1, 3, 300)]


@pytest.mark.parametrize("shape", DIAG_SHAPES, ids=[f"n{n}-K{K}-S{S}" for n, K, S in DIAG_SHAPES])
def test_mc_diag_equals_replay(shape):
    _check_shape(*shape, factor=False)


@pytest.mark.parametrize("shape", FACTOR_SHAPES, ids=[f"n{n}-K{K}-S{S}" for n, K, S in FACTOR_SHAPES])
def test_mc_factor_equals_replay(shape):
    _check_shape(*shape, factor=True)


@pytest.mark.parametrize("K,factor", [(10, False), (100, False), (3000, False), (10, True)])
def test_no_spread_gives_softmax_of_the_mean_whatever_S(K, factor):
    mean = _inputs(2, K, False)[0]
    var = None if factor else np.zeros((2, K))
    L = np.zeros((2, K, K), dtype=np.float32) if factor else None
    one = _mc(mean, var, L, 1, 5, 3)
    seven = _mc(mean, var, L, 7, 5, 3)
    assert np.array_equal(one[0].view(np.int64), seven[0].view(np.int64)) and np.array_equal(one[1].view(np.int64), seven[1].view(np.int64))
    want = lr.softmax(mean.astype(np.float32).astype(np.float64))
    assert np.abs(one[0] - want).max() <= 2.0 ** -22
    assert np.abs(one[1] - lr.entropy(want)).max() <= 2.0 ** -22 * (1.0 + math.log(2.0 ** 24))


DEAD = ["nan_mean", "inf_var", "negative_var", "nan_factor"]


@pytest.mark.parametrize("what", DEAD)
def test_dead_row_is_flagged_and_leaves_its_neighbours_alone(what):
    factor = what == "nan_factor"
    mean, var, L = (np.array(x, copy=True) if x is not None else None for x in _inputs(3, 10, factor))
    if what == "nan_mean":
        mean[1, 4] = float("nan")
    elif what == "inf_var":
        var[1, 9] = float("inf")
    elif what == "negative_var":
        var[1, 0] = -1e-3
    else:
        L[1, 7, 2] = float("nan")
    probs, ent, flags = _mc(mean, var, L, 9, 4, 6)
    assert flags.tolist() == [0, 1, 0]
    assert np.isnan(probs[1]).all() and np.isnan(ent[1]) and np.isfinite(probs[[0, 2]]).all() and np.isfinite(ent[[0, 2]]).all()
    for r in (0, 2):                                                       # the call without the dead row
        alone = _mc(mean[r:r + 1], None if var is None else var[r:r + 1], None if L is None else L[r:r + 1], 9, 4, 6 + r)
        assert np.array_equal(alone[0].view(np.int64), probs[r:r + 1].view(np.int64)) and alone[1][0] == ent[r]
    if factor:                                                             # the strict upper triangle is not read
        L2 = np.array(_inputs(3, 10, True)[2], copy=True)
        L2[1, 2, 7] = float("nan")
        assert _mc(mean, None, L2, 9, 4, 6)[2].tolist() == [0, 0, 0]


def test_mc_refusals_write_nothing():
    lib = nv.load()
    n, K, S = 2, 8, 4
    m = torch.zeros(n * 8193, device=DEV, dtype=F64)
    v = torch.ones(n * 8193, device=DEV, dtype=F64)
    L = torch.zeros(n * 65 * 65, device=DEV, dtype=torch.float32)
    probs = torch.full((n * 8193,), FILL, device=DEV, dtype=F64)
    ent = torch.full((n,), FILL, device=DEV, dtype=F64)
    flags = torch.full((n,), -77, device=DEV, dtype=torch.int32)
    M, V, Lp, P, E, Fl = (nv.ptr(x) for x in (m, v, L, probs, ent, flags))
    calls = [(None, V, None, n, K, S, 0, 0, P, E, Fl),                      # mean = NULL
             (M, V, None, n, K, S, 0, 0, None, E, Fl),                      # probs = NULL
             (M, V, None, n, K, S, 0, 0, P, E, None),                       # flags = NULL
             (M, V, Lp, n, K, S, 0, 0, P, E, Fl),                           # both var and L
             (M, None, None, n, K, S, 0, 0, P, E, Fl),                      # neither
             (M, V, None, 0, K, S, 0, 0, P, E, Fl),                         # n = 0
             (M, V, None, n, K, 0, 0, 0, P, E, Fl),                         # S = 0
             (M, V, None, n, 0, S, 0, 0, P, E, Fl),                         # K = 0
             (M, V, None, n, 8193, S, 0, 0, P, E, Fl),                      # K over the cap of the variance form
             (M, None, Lp, n, 65, S, 0, 0, P, E, Fl),                       # K over the cap of the factor form
             (M, V, None, n, K, 2 ** 31, 0, 0, P, E, Fl),                   # S = 2^31
             (M, V, None, n, K, S, 0, -1, P, E, Fl),                        # example_offset = -1
             (M, V, None, n, K, S, 0, 2 ** 32 - 1, P, E, Fl)]               # example_offset + n > 2^32
    st = nv.stream_ptr()
    for args in calls:
        assert lib.lip_link_mc(*args, st) == LIP_ERR_ARG, args
        assert b"lip_link_mc" in lib.lip_last_error()
    torch.cuda.synchronize()
    assert bool((probs == FILL).all()) and bool((ent == FILL).all()) and bool((flags == -77).all())
    assert lib.lip_link_mc(M, V, None, n, K, S, 0, 2 ** 32 - 2, P, E, Fl, st) == 0      # the last legal offset
    torch.cuda.synchronize()
    assert bool((probs[:n * K] != FILL).all()) and bool((probs[n * K:] == FILL).all()) and bool((flags == 0).all())


# ------------------------------------------------------------------------------------------------ the factor
def _chol(C):
    """lip_link_chol on canary-guarded buffers -> (L (n, K, K) float32 numpy, flags (n,))"""
    lib = nv.load()
    n, K = C.shape[0], C.shape[-1]
    c = _dev(C, F64)
    lb, L = _guarded(n * K * K, torch.float32, FILL)
    fb, flags = _guarded(n, torch.int32, -77)
    rc = lib.lip_link_chol(nv.ptr(c), n, K, L.data_ptr(), flags.data_ptr(), nv.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.lip_last_error()
    _assert_guards(lb, n * K * K, FILL, "L")
    _assert_guards(fb, n, -77, "flags")
    return L.cpu().numpy().reshape(n, K, K), flags.cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 5, 31, 64])
def test_chol_equals_the_column_rule(K):
    rng = np.random.default_rng(K)
    low_rank = rng.standard_normal((K, max(1, K // 3)))
    mats = [_psd(rng, K, "full"), _psd(rng, K, "rank1"), low_rank @ low_rank.T, _psd(rng, K, "zero"),
            1e6 * _psd(rng, K, "full"), 1e-6 * _psd(rng, K, "full")]
    neg = _psd(rng, K, "full")
    neg[K // 2, K // 2] = -1.0
    nan_low = _psd(rng, K, "full")
    nan_low[K - 1, 0] = float("nan")
    mats += [neg, nan_low]
    if K > 1:
        nan_up = _psd(rng, K, "full")
        nan_up[0, K - 1] = float("inf")                                    # the strict upper triangle is not read
        mats.append(nan_up)
    C = np.stack(mats)
    L, flags = _chol(C)
    worst = 0.0
    for i in range(C.shape[0]):
        ref, dead = lr.cholesky_semidefinite(C[i])
        assert flags[i] == dead, f"matrix {i}: flag {flags[i]}, the rule says {dead}"
        assert not np.triu(L[i], 1).any()
        assert np.array_equal((L[i] == 0).all(0), (ref == 0).all(0)), f"matrix {i}: the zero columns differ"
        scale = np.abs(ref).max()
        if scale > 0:
            worst = max(worst, np.abs(L[i] - ref).max() / (2.0 ** -23 * scale))
        assert np.abs(L[i] - ref).max() <= 2.0 ** -23 * scale, f"matrix {i}"
    assert flags.tolist()[6:8] == [1, 1] and not L[6:8].any()
    print(f"STAT link_chol K{K}: worst |L - ref| / (2^-23 max|ref|) {worst:.3f}")
    again, _ = _chol(C)
    assert np.array_equal(again.view(np.int32), L.view(np.int32))


def test_chol_refusals_write_nothing():
    lib = nv.load()
    c = torch.ones(2 * 65 * 65, device=DEV, dtype=F64)
    L = torch.full((2 * 65 * 65,), FILL, device=DEV, dtype=torch.float32)
    flags = torch.full((2,), -77, device=DEV, dtype=torch.int32)
    C, Lp, Fl = nv.ptr(c), nv.ptr(L), nv.ptr(flags)
    for args in [(None, 2, 4, Lp, Fl), (C, 2, 4, None, Fl), (C, 2, 4, Lp, None), (C, 0, 4, Lp, Fl), (C, 2, 0, Lp, Fl),
                 (C, 2, 65, Lp, Fl)]:
        assert lib.lip_link_chol(*args, nv.stream_ptr()) == LIP_ERR_ARG, args
        assert b"lip_link_chol" in lib.lip_last_error()
    torch.cuda.synchronize()
    assert bool((L == FILL).all()) and bool((flags == -77).all())


# ------------------------------------------------------------------------------------------------ the surface
@functools.lru_cache(maxsize=None)
def _case(name):
    """(state, Z, model_type, Xnew (11 points), labels, alpha) of a net of tests/kfac_ref.py, built once, never written"""
    state, Z, model_type = kf.make_case(name)
    g = torch.Generator().manual_seed(5)
    X = torch.randn((11,) + tuple(Z.shape[1:]), dtype=F64, generator=g)
    y = torch.randint(0, int(state.net.num_outputs), (11,), generator=g)
    return state, Z, model_type, X, y, 0.7


def _assert_close_to_replay(probs, unc, mean, var, L, S, seed, off):
    mean, var, L = (None if x is None else x.cpu().numpy() for x in (mean, var, L))
    p_ref, h_ref, p_draws = lr.replay(mean, var=var, L=L, S=S, seed=seed, example_offset=off, return_draws=True)
    tol_p, tol_h = _bounds(mean, var, L, p_draws)
    e_p, e_h = np.abs(probs.cpu().numpy() - p_ref).max(), np.abs(unc["aleatoric"].cpu().numpy() - h_ref).max()
    print(f"STAT link surface: probs {e_p:.3g} / {tol_p:.3g}, entropy {e_h:.3g} / {tol_h:.3g}")
    assert e_p <= tol_p and e_h <= tol_h
    total = -torch.xlogy(probs, probs).sum(-1)
    assert torch.equal(unc["total"], total) and torch.equal(unc["epistemic"], total - unc["aleatoric"])
    assert float(unc["epistemic"].min()) >= -(tol_h + 2.0 ** -40)          # Jensen, up to the float32 entropies of the draws


def test_link_predictive_mc_on_the_diagonal_predictive():
    state, Z, model_type, X, _, alpha = _case("xor_classifier")
    mean, var = predict_lla_diag(state, X, Z, model_type, alpha, full_set_size=N_FULL)
    probs, unc = link_predictive(mean, var, link="mc", num_samples=64, seed=3, example_offset=5, return_uncertainty=True)
    assert probs.dtype == F64 and probs.shape == (11, 2) and probs.is_cuda
    _assert_close_to_replay(probs, unc, mean, var, None, 64, 3, 5)
    assert torch.equal(link_predictive(mean, var, link="mc", num_samples=64, seed=3, example_offset=5), probs)
    bad = mean.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="row 4"):
        link_predictive(bad, var, link="mc", num_samples=8)


def test_link_predictive_mc_on_a_full_kfac_covariance():
    state, Z, model_type, X, _, alpha = _case("resnet_tiny")
    dist = predict_lla_kfac(state, X, Z, model_type, alpha, full_set_size=N_FULL, cov="full")
    assert isinstance(dist, MultivariateNormalFullCovariance) and dist.covariance().shape == (11, 4, 4)
    L = cholesky_semidefinite(dist.covariance())
    C = dist.covariance().cpu().numpy()
    for i in range(11):
        ref, dead = lr.cholesky_semidefinite(C[i])
        assert not dead and np.abs(L[i].cpu().numpy() - ref).max() <= 2.0 ** -23 * np.abs(ref).max()
    probs, unc = link_predictive(dist, link="mc", num_samples=70, seed=11, return_uncertainty=True)
    _assert_close_to_replay(probs, unc, dist.mean().reshape(11, 4), None, L, 70, 11, 0)
    off = link_predictive(dist.mean(), dist.variance(), link="mc", num_samples=70, seed=11)
    assert not torch.equal(off, probs)                                     # the off-diagonal covariances are used


@pytest.mark.parametrize("posterior", ["diag", "kfac"])
def test_closed_form_probit_equals_eval_dataset_probit(posterior):
    state, Z, model_type, X, y, alpha = _case("xor_classifier")
    loader = [(X[:4], y[:4]), (X[4:], y[4:])]
    want = eval_dataset_probit(state, loader, Z, alpha, N_FULL, model_type, posterior=posterior)
    got = eval_dataset_closed_form(state, loader, Z, alpha, N_FULL, model_type, posterior=posterior, link="probit")
    assert got[:4] == want[:4] and torch.equal(got[4], want[4]) and torch.equal(got[5], want[5])


def test_closed_form_mc_does_not_depend_on_the_batch_size():
    state, Z, model_type, X, y, alpha = _case("xor_classifier")
    outs = []
    for bs in (4, 7):
        loader = [(X[s:s + bs], y[s:s + bs]) for s in range(0, 11, bs)]
        outs.append(eval_dataset_closed_form(state, loader, Z, alpha, N_FULL, model_type, posterior="diag", link="mc",
                                             num_samples=50, seed=2))
    assert outs[0][4].shape == (11, 2) and torch.equal(outs[0][4], outs[1][4]) and outs[0][:4] == outs[1][:4]
    other = eval_dataset_closed_form(state, [(X, y)], Z, alpha, N_FULL, model_type, posterior="diag", link="mc",
                                     num_samples=50, seed=3)
    assert not torch.equal(other[4], outs[0][4])                           # the seed matters
    for link in ("bridge", "bridge_norm"):
        p = eval_dataset_closed_form(state, [(X, y)], Z, alpha, N_FULL, model_type, posterior="diag", link=link)[4]
        assert p.shape == (11, 2) and bool(((p.sum(-1) - 1).abs() < 1e-12).all())


def test_auroc_ood_closed_form():
    state, Z, model_type, X, y, alpha = _case("xor_classifier")
    g = torch.Generator().manual_seed(9)
    X_ood = 6.0 * torch.randn(9, 2, dtype=F64, generator=g)
    id_loader, ood_loader = [(X[:6], y[:6]), (X[6:], y[6:])], [(X_ood, torch.zeros(9, dtype=torch.long))]
    common = (state, id_loader, ood_loader, Z, alpha, N_FULL, model_type)
    for score in ("max_prob", "entropy", "mutual_information"):
        a = auroc_ood_closed_form(*common, link="mc", score=score, num_samples=40, seed=1)
        assert 0.0 <= a <= 1.0 and a == auroc_ood_closed_form(*common, link="mc", score=score, num_samples=40, seed=1)
    for score in ("max_prob", "entropy"):
        assert 0.0 <= auroc_ood_closed_form(*common, link="probit", score=score) <= 1.0
    p_id = eval_dataset_closed_form(state, id_loader, Z, alpha, N_FULL, model_type, link="probit")[4]
    p_ood = eval_dataset_closed_form(state, ood_loader, Z, alpha, N_FULL, model_type, link="probit")[4]
    want = roc_auc(torch.cat([torch.zeros(11), torch.ones(9)]), torch.cat([ood_scores(p_id), ood_scores(p_ood)]))
    assert auroc_ood_closed_form(*common, link="probit", score="max_prob") == want
    with pytest.raises(ValueError, match="mutual_information"):
        auroc_ood_closed_form(*common, link="probit", score="mutual_information")
