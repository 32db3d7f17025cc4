"""CPU checks of the eigenvalue-corrected Kronecker-factored posterior: the package's host algebra (``ekfac.py``) fed the
float64 helper's factors and second moments (``tests/ekfac_ref.py``) against the helper's dense route, the optimality
property the method rests on, and the refusals that return before any GPU work.

Everything is float64 on the host; the bound 1e-11 max|ref| is that of tests/test_kfac_cpu.py (alpha keeps the condition
of every block at most 1002).
"""
import ctypes
import functools

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import ekfac, kfac
from lip_amd.distributions import KFACNormal, KroneckerNormal
from lip_amd.lla import posterior_lla_ekfac, predict_lla_ekfac
from lip_amd.prior import GroupedPrior
from lip_amd.utils import flatten_nn_params

F64 = torch.float64
TOL = 1e-11
N_FULL = kf.N_FULL


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


@functools.lru_cache(maxsize=None)
def _fitted(name, grouped, one_example=False):
    state, Z, model_type = kf.make_case(name)
    Z = Z[:1] if one_example else Z
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    D = a.numel()
    table = kfac.block_table(state)
    rows = [kfac.block_prior_rows(prior, b, D) for b in table]
    recal = ref.recal(state, M, model_type, N_FULL)
    kfits = kfac.fit_blocks(table, As, Ss, rows, recal, M, model_type != "regressor")
    _, J, H = er.jacobian(state, Z, model_type)
    bases = [(f[0], f[2]) for f in kfits]
    Lams = er.scales_ref(J, H, state, bases)
    fits = ekfac.corrected_fits(kfits, Lams, recal)
    rem = kf.remainder_of(state)
    rem_var = 1.0 / (a[rem] + kf.ggn_diag_ref(state, Z, model_type, N_FULL)[rem])
    post = ekfac.posterior_from_fit(torch.zeros(D, dtype=F64), table, fits, rem, rem_var, a[rem])
    return dict(state=state, Z=Z, model_type=model_type, a=a, table=table, kfits=kfits, bases=bases, Lams=Lams, fits=fits,
                recal=recal, rem=rem, rem_var=rem_var, post=post, J=J, H=H, As=As, Ss=Ss, M=M)


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", ["sine_regressor", "xor_classifier", "mlp_ragged", "flat_head", "stem_net"])
def test_assembled_posterior_matches_the_dense_route(name, grouped):
    """``corrected_fits`` and ``posterior_from_fit`` on CPU tensors: the variance, every block's covariance and the
    log-determinant against (V (x) Ub) diag(1 / (recal Lam + 1)) (V (x) Ub)^T built with ``torch.kron``; and the
    derivation itself: the block's precision in the basis V (x) Ub has the diagonal recal Lam + 1"""
    h = _fitted(name, grouped)
    post, a = h["post"], h["a"]
    assert isinstance(post, KFACNormal) and all(isinstance(kn, KroneckerNormal) and kn.spectrum is None for _, kn in post.blocks)
    cov_blocks = er.covariance_blocks(h["state"], h["bases"], h["Lams"], h["recal"])
    e_var = _err(post.variance(), kf.variance_ref(h["state"], cov_blocks, h["rem"], h["rem_var"]))
    e_cov = max(_err(kn.covariance(), S) for (_, kn), (_, S) in zip(post.blocks, cov_blocks))
    logdet = float(-torch.log(a[h["rem"]] * h["rem_var"]).sum())
    e_diag = 0.0
    for (off, S), (V, Ub), Lam in zip(cov_blocks, h["bases"], h["Lams"]):
        al = a[off:off + S.shape[0]]
        logdet += float(-torch.logdet(S) - torch.log(al).sum())
        Mt, N = Lam.shape
        G = h["recal"] * er.exact_block(h["J"], h["H"], off, Mt, N)
        W = torch.kron(V, Ub)
        e_diag = max(e_diag, _err(torch.diagonal(W.T @ (G + torch.diag(al)) @ W), (h["recal"] * Lam + 1.0).reshape(-1)))
    e_ld = abs(float(post.log_det_precision_ratio()) - logdet) / abs(logdet)
    print(f"{name} {'grouped' if grouped else 'scalar'}: variance {e_var:.2e} block covariance {e_cov:.2e} logdet {e_ld:.2e} "
          f"diagonal of the precision in the basis {e_diag:.2e}")
    assert max(e_var, e_cov, e_ld, e_diag) <= TOL


@pytest.mark.parametrize("name", kf.DENSE_ONLY)
def test_one_example_on_a_dense_net_gives_the_kfac_posterior(name):
    """where KFAC is exact (M = 1, every T_l = 1) the corrected eigenvalues are KFAC's: recal Lam = c lam (x) mu"""
    h = _fitted(name, False, True)
    for (V, R, Ub), (_, Rk, _, lam, mu, c), Lam in zip(h["fits"], h["kfits"], h["Lams"]):
        want = c * torch.outer(lam, mu)
        assert float((h["recal"] * Lam - want).abs().max()) <= 1e-12 * float(want.max())
        assert float((R - Rk).abs().max()) <= 1e-12


def test_diagonal_in_the_eigenbasis_minimises_the_frobenius_error():
    """random small problems in float64: with G = sum_r w_r w_r^T and Q = U_A (x) U_S orthonormal, s* = diag(Q^T G Q) (the
    helper's ``best_diagonal``, equal to the sum of squared rotated rows) is no worse than the Kronecker product of the
    factors, and every perturbed s is worse: ||G - Q diag(s* + e) Q^T||_F^2 = ||G - Q diag(s*) Q^T||_F^2 + ||e||^2"""
    g = torch.Generator().manual_seed(0)
    for Mt, N, R in [(1, 1, 1), (3, 2, 5), (5, 4, 2), (4, 6, 30)]:
        Wr = torch.randn(R, Mt, N, dtype=F64, generator=g)
        Wf = Wr.reshape(R, Mt * N)
        G = Wf.T @ Wf
        A = torch.einsum("rfk,rgk->fg", Wr, Wr)
        S = torch.einsum("rfk,rfl->kl", Wr, Wr)
        lam, Ua = torch.linalg.eigh(A)
        mu, Us = torch.linalg.eigh(S)
        Q = torch.kron(Ua, Us)
        s = er.best_diagonal(G, Q)
        assert _err(s, ((Ua.T @ Wr @ Us) ** 2).sum(0).reshape(-1)) <= 1e-13
        e_best = er.frobenius_error(G, Q, s)
        c = float(torch.trace(G) / (torch.trace(A) * torch.trace(S)))
        assert e_best <= er.frobenius_error(G, Q, c * torch.outer(lam, mu).reshape(-1)) * (1 + 1e-12)
        for _ in range(5):
            e = 0.1 * float(s.max()) * torch.randn(s.shape, dtype=F64, generator=g)
            worse = er.frobenius_error(G, Q, s + e)
            assert worse > e_best
            assert abs(worse ** 2 - e_best ** 2 - float((e ** 2).sum())) <= 1e-10 * worse ** 2


def test_prior_varying_inside_a_row_is_refused_before_any_engine_is_bound():
    state, Z, model_type = kf.make_case("flat_head")
    D = flatten_nn_params(state.params)[0].numel()
    for b in kfac.block_table(state):
        cut = b.off + (1 if b.bias else 0) * b.N + 1                  # inside the first kernel row
        prior = GroupedPrior.from_table([("a", [(0, cut)]), ("b", [(cut, D - cut)])], [1.0, 2.0], D)
        with pytest.raises(ValueError, match="constant along"):       # runs without a GPU
            posterior_lla_ekfac(state, Z, model_type, prior)
        with pytest.raises(ValueError, match="constant along"):
            predict_lla_ekfac(state, Z[:2], Z, model_type, prior, cov="diag")


def test_cov_argument_is_checked():
    state, Z, model_type = kf.make_case("xor_classifier")
    with pytest.raises(ValueError, match="'diag' or 'full'"):
        predict_lla_ekfac(state, Z[:2], Z, model_type, 1.0, cov="dense")


def test_sqsum_refusals_return_before_any_launch():
    """a null pointer or a non-positive extent is LIP_ERR_ARG; the pointers are host buffers no kernel ever sees"""
    lib = nv.load()
    R, off, Mt, N = 3, 2, 4, 5
    ldw = off + Mt * N
    W = (ctypes.c_float * (R * ldw))()
    V, Ub, Lam = (ctypes.c_double * (Mt * Mt))(), (ctypes.c_double * (N * N))(), (ctypes.c_double * (Mt * N))()
    scratch = (ctypes.c_double * (2 * Mt * N))()
    adr = ctypes.addressof
    good = [adr(W), ldw, R, off, Mt, N, adr(V), adr(Ub), adr(Lam), adr(scratch), 2 * Mt * N, None]
    for i, v in [(0, None), (6, None), (7, None), (8, None), (9, None), (2, 0), (2, -1), (4, 0), (4, -3), (5, 0), (5, -1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_eigen_sqsum(*args) == 1, (i, v)
        assert b"lip_kfac_eigen_sqsum" in lib.lip_last_error()
    d = ctypes.c_int64(-7)
    for args in [(0, Mt, N), (R, 0, N), (R, Mt, 0), (-1, Mt, N), (R, 1 << 16, 1 << 15)]:
        assert lib.lip_kfac_eigen_sqsum_scratch(*args, ctypes.byref(d)) == 1 and d.value == -7
    assert lib.lip_kfac_eigen_sqsum_scratch(R, Mt, N, None) == 1
    assert all(x == 0.0 for x in Lam)
    assert lib.lip_kfac_eigen_sqsum_scratch(R, Mt, N, ctypes.byref(d)) == 0 and d.value >= (R + 1) * Mt * N
