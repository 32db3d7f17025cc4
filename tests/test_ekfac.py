"""GPU checks of the eigenvalue-corrected Kronecker-factored posterior (EKFAC): the kernel ``lip_kfac_eigen_sqsum`` on
synthetic operands through ctypes, then ``LinearizedNet.kfac_eigen_sqsums`` and the public surface (``ekfac.py``) on the
nets of tests/kfac_ref.py.

Kernel level: the reference is a float64 product of the up-cast float32 rows, and the bound is the standard float64
summation bound on the absolute-value twin of the reference with a factor 4 for the reference's own rounding (the
convention of tests/test_kfac.py): 4 (2 (Mt + N) + R + 8) 2^-53 sum_r (|V|^T |J_r| |Ub|)^2, 2 (Mt + N) for the two
products of a square and R for the sum over the rows.  It holds for any summation order.

Engine level: the factor rows come from the float32 passes, so no bound is derivable; every bound there is 4 x the worst
error measured on MI355X against the float64 helper (``tests/ekfac_ref.py``), with the measured figure next to it.  The
helper always works in the product's own basis (V, Ub): eigenvectors of near-degenerate eigenvalues are never compared
across implementations.
"""
import ctypes
import functools

import pytest
import torch

import ekfac_ref as er
import kfac_ref as kf
import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import _native as nv
from lip_amd import ekfac, kfac
from lip_amd.distributions import KFACNormal, MultivariateNormalFullCovariance
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache, compute_ekfac_scales, compute_ggn_diag, compute_kfac_factors, get_engine
from lip_amd.lla import (posterior_lla_ekfac, predict_lla_ekfac, predict_lla_ekfac_scalable, predict_lla_kfac)
from lip_amd.train_alpha import fit_alpha_ekfac, log_marginal_likelihood_ekfac
from lip_amd.utils import flatten_nn_params

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
U = 2.0 ** -53
DEV = "cuda"
N_FULL = kf.N_FULL
CONV_NETS = ["resnet_tiny", "resnet50_tiny", "flat_head", "stem_net"]          # every net with a block of T_l > 1


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


# ------------------------------------------------------------------------------------------------ kernel level
SQSUM_BLOCKS = [(1, 1), (9, 3), (37, 5), (33, 33), (28, 10), (70, 130)]
SQSUM_ROWS = [1, 3, 50, 257]


def _scratch_query(R, Mt, N):
    d = ctypes.c_int64(0)
    nv.check(nv.load().lip_kfac_eigen_sqsum_scratch(R, Mt, N, ctypes.byref(d)), "lip_kfac_eigen_sqsum_scratch")
    return d.value


def _run_sqsum(W, ldw, R, off, Mt, N, V, Ub, Lam, scratch_doubles=None):
    doubles = _scratch_query(R, Mt, N) if scratch_doubles is None else scratch_doubles
    scratch = torch.empty(doubles, device=DEV, dtype=F64)
    nv.check(nv.load().lip_kfac_eigen_sqsum(W.data_ptr(), ldw, R, off, Mt, N, V.data_ptr(), Ub.data_ptr(), Lam.data_ptr(),
                                            scratch.data_ptr(), doubles, nv.stream_ptr()), "lip_kfac_eigen_sqsum")
    torch.cuda.synchronize()
    return Lam


@pytest.mark.parametrize("Mt,N", SQSUM_BLOCKS)
def test_sqsum_against_float64_product(Mt, N):
    g = torch.Generator().manual_seed(Mt * 1000 + N)
    off = 5
    ldw = off + Mt * N + 3
    V = torch.randn(Mt, Mt, generator=g, dtype=F64).to(DEV)
    Ub = torch.randn(N, N, generator=g, dtype=F64).to(DEV)
    Lam0 = torch.rand(Mt, N, generator=g, dtype=F64).to(DEV) + 0.5             # non-zero: the call adds
    for R in SQSUM_ROWS:
        W = torch.randn(R, ldw, generator=g, dtype=F32).to(DEV)
        J = W[:, off:off + Mt * N].double().reshape(R, Mt, N)
        want = ((V.T @ J @ Ub) ** 2).sum(0)
        bound = 4 * (2 * (Mt + N) + R + 8) * U * ((V.abs().T @ J.abs() @ Ub.abs()) ** 2).sum(0)
        # the sums themselves, added into zeros, against the bound; then into Lam0: one float64 addition of the same sums
        # (Lam0 + sums, rounded once), so the pre-filled result is known bitwise and no rounding of Lam0 enters the bound
        sums = _run_sqsum(W, ldw, R, off, Mt, N, V, Ub, torch.zeros(Mt, N, device=DEV, dtype=F64))
        err = (sums - want).abs()
        print(f"sqsum Mt={Mt} N={N} R={R}: max err / bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all())
        got = _run_sqsum(W, ldw, R, off, Mt, N, V, Ub, Lam0.clone())
        assert torch.equal(got, Lam0 + sums) and not torch.equal(got, sums)
        assert torch.equal(got, _run_sqsum(W, ldw, R, off, Mt, N, V, Ub, Lam0.clone()))          # bitwise reproducible
        if R > 2:
            # a scratch for two rows (4 Mt N doubles: chunks of two rows in two groups, a ragged last chunk where R is
            # odd) and the smallest the call takes, one row (2 Mt N doubles: chunks of one row)
            for rows in (2, 1):
                small = _run_sqsum(W, ldw, R, off, Mt, N, V, Ub, torch.zeros(Mt, N, device=DEV, dtype=F64),
                                   scratch_doubles=rows * 2 * Mt * N)
                assert bool(((small - want).abs() <= bound).all()), rows


def test_sqsum_scratch_query_and_row_groups():
    """the query covers the rows and one partial sum per row group; (577, 64) has 19 blocks, so 257 rows run in 52 groups
    of 5 rows (the last of 2), and a block with many tiles runs in few groups"""
    assert _scratch_query(1, 9, 3) == 2 * 27
    assert _scratch_query(257, 577, 64) == (257 + 52) * 577 * 64
    assert _scratch_query(257, 70, 130) == (257 + 129) * 70 * 130
    assert _scratch_query(50, 1024, 1024) == (50 + 4) * 1024 * 1024


def test_sqsum_status_codes_leave_the_sums_untouched():
    lib = nv.load()
    R, off, Mt, N = 4, 4, 9, 3
    ldw = off + Mt * N
    W = torch.randn(R, ldw, dtype=F32).to(DEV)
    V, Ub = (torch.randn(s, dtype=F64).to(DEV) for s in ((Mt, Mt), (N, N)))
    Lam0 = torch.full((Mt, N), 3.0, device=DEV, dtype=F64)
    Lam = Lam0.clone()
    scratch = torch.empty(_scratch_query(R, Mt, N), device=DEV, dtype=F64)
    good = [W.data_ptr(), ldw, R, off, Mt, N, V.data_ptr(), Ub.data_ptr(), Lam.data_ptr(), scratch.data_ptr(), scratch.numel(),
            nv.stream_ptr()]
    for i, v in [(0, 0), (6, 0), (7, 0), (8, 0), (9, 0), (2, 0), (2, -1), (4, 0), (5, 0), (5, -2), (3, -1), (1, ldw - 1),
                 (10, 2 * Mt * N - 1)]:
        args = list(good)
        args[i] = v
        assert lib.lip_kfac_eigen_sqsum(*args) == 1, (i, v)
    # Mt N >= 2^31 is refused before any launch (nothing of that size exists)
    big = list(good)
    big[1], big[4], big[5] = 1 << 40, 1 << 16, 1 << 15
    assert lib.lip_kfac_eigen_sqsum(*big) == 1
    torch.cuda.synchronize()
    assert torch.equal(Lam, Lam0)
    assert lib.lip_kfac_eigen_sqsum(*good) == 0
    torch.cuda.synchronize()
    assert not torch.equal(Lam, Lam0)


# ------------------------------------------------------------------------------------------------ engine level
@functools.lru_cache(maxsize=None)
def _helper(name):
    """everything of the float64 helper, built once per net and never written to"""
    state, Z, model_type = kf.make_case(name)
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    Xnew = kref.new_points(Z, 5, 7)
    f_new, J_new = ref.jac64(state, Xnew, model_type)
    _, J, H = er.jacobian(state, Z, model_type)
    return dict(state=state, Z=Z, model_type=model_type, As=As, Ss=Ss, M=M, alpha=alpha, Xnew=Xnew, f_new=f_new, J_new=J_new,
                J=J, H=H, diag=kf.ggn_diag_ref(state, Z, model_type, N_FULL), diag1=kf.ggn_diag_ref(state, Z, model_type, None),
                rem=kf.remainder_of(state), recal=ref.recal(state, M, model_type, N_FULL))


def _rel(v, r):
    r = r.to(v.device)
    return ((v.double() - r).abs().max() / r.abs().max()).item()


def _cpu(bases):
    return [(V.cpu(), Ub.cpu()) for V, Ub in bases]


def _orthonormal(h):
    """the product's orthonormal bases (device) and its factors"""
    blocks, As, Ss, M = compute_kfac_factors(h["state"], h["Z"], h["model_type"])
    return blocks, ekfac.orthonormal_bases(blocks, As, Ss, h["model_type"] != "regressor")


# measured on MI355X, worst over the blocks of a net of max|Lam_l - ref| / max|ref| against the float64 helper in the
# product's own basis (the fitted basis (V, Ub) of the scalar prior and the orthonormal basis gave the same figures):
#   sine_regressor 3.68e-7   xor_classifier 3.92e-8   mlp_ragged 1.98e-8   resnet_tiny 3.99e-7
#   resnet50_tiny  2.62e-7   flat_head      1.04e-7   stem_net   8.67e-8
SCALES_TOL = 1.6e-6            # 4 x 3.99e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_scales_match_the_float64_helper(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, h["alpha"], N_FULL, None)
    fitted = [(V, Ub) for V, _, Ub in fits]
    blocks, ortho = _orthonormal(h)
    worst = []
    for bases in (fitted, ortho):
        Lams = compute_ekfac_scales(state, Z, model_type, bases)
        want = er.scales_ref(h["J"], h["H"], state, _cpu(bases))
        assert len(Lams) == len(blocks) == len(want)
        for b, Lam in zip(blocks, Lams):
            assert Lam.dtype == F64 and Lam.is_cuda and Lam.shape == (b.Mt, b.N) and float(Lam.min()) >= 0.0
        worst.append(max(_rel(Lam, w) for Lam, w in zip(Lams, want)))
    print(f"{name}: scales fitted basis {worst[0]:.2e}  orthonormal basis {worst[1]:.2e}")
    assert max(worst) <= SCALES_TOL
    # R of the fit is 1 / (recal Lam + 1): recal Lam recovered from it is these scales (from a pass of its own)
    Lams = compute_ekfac_scales(state, Z, model_type, fitted)
    for (_, R, _), Lam in zip(fits, Lams):
        assert R.shape == Lam.shape and float(R.min()) > 0.0 and float(R.max()) <= 1.0
        assert _rel(1.0 / R - 1.0, (h["recal"] * Lam).cpu()) <= SCALES_TOL


# measured on MI355X, max|. - ref| / max|ref| of the posterior variance / predictive covariance / mean, scalar prior
# (two-group prior); the diag form of the predictive is within 2 % of the full form's figure everywhere but flat_head
# (7.16e-8, 5.56e-8):
#   sine_regressor 1.33e-7 / 3.04e-7 / 3.20e-7 (1.33e-7 / 3.07e-7 / 3.20e-7)
#   xor_classifier 3.04e-8 / 6.36e-8 / 1.01e-7 (3.04e-8 / 6.53e-8 / 1.01e-7)
#   mlp_ragged     2.20e-8 / 1.13e-7 / 2.18e-7 (2.02e-8 / 1.16e-7 / 2.18e-7)
#   resnet_tiny    1.54e-7 / 4.21e-8 / 1.14e-7 (1.54e-7 / 4.05e-8 / 1.14e-7)
#   resnet50_tiny  2.80e-7 / 1.24e-7 / 2.47e-7 (2.80e-7 / 1.40e-7 / 2.47e-7)
#   flat_head      4.51e-8 / 9.02e-8 / 1.72e-7 (5.17e-8 / 6.67e-8 / 1.72e-7)
#   stem_net       7.31e-8 / 3.68e-8 / 2.06e-7 (7.31e-8 / 3.74e-8 / 2.06e-7)
VARIANCE_TOL = 1.2e-6          # 4 x 2.80e-7
PREDICT_TOL = 1.3e-6           # 4 x 3.07e-7
MEAN_TOL = 1.3e-6              # 4 x 3.20e-7


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kf.NETS)
def test_posterior_and_predictive_match_the_float64_helper(name, grouped):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    post = posterior_lla_ekfac(state, Z, model_type, prior, full_set_size=N_FULL)
    assert isinstance(post, KFACNormal) and all(kn.spectrum is None for _, kn in post.blocks)
    theta = flatten_nn_params(state.params)[0]
    assert post.mean().dtype == F64 and torch.equal(post.mean().cpu(), theta.double())
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, prior, N_FULL, None)
    bases = _cpu([(V, Ub) for V, _, Ub in fits])
    cov_blocks = er.covariance_blocks(state, bases, er.scales_ref(h["J"], h["H"], state, bases), h["recal"])
    rem = h["rem"]
    rem_var = 1.0 / (a[rem] + h["diag"][rem])
    e_var = _rel(post.variance(), kf.variance_ref(state, cov_blocks, rem, rem_var))
    K = h["f_new"].shape[1]
    cov_ref = kf.predict_dense(h["J_new"], cov_blocks, rem, rem_var)
    full = predict_lla_ekfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="full", batch=3)
    mean, var = predict_lla_ekfac(state, h["Xnew"], Z, model_type, prior, full_set_size=N_FULL, cov="diag", batch=3)
    assert isinstance(full, MultivariateNormalFullCovariance)
    if model_type == "regressor":
        assert full.mean().shape == (5,) and full.covariance().shape == (5, 5) and mean.shape == var.shape == (5,)
        cov = torch.diagonal(full.covariance())[:, None, None]
    else:
        assert full.mean().shape == (5, K) and full.covariance().shape == (5, K, K) and mean.shape == var.shape == (5, K)
        cov = full.covariance()
        assert torch.equal(cov, cov.transpose(1, 2))
    var_ref = torch.diagonal(cov_ref, dim1=1, dim2=2).to(DEV)
    e_diag = ((var.reshape(5, K) - var_ref).abs().max() / cov_ref.abs().max()).item()
    e_cov = _rel(cov, cov_ref)
    e_mean = _rel(mean.reshape(5, K), h["f_new"])
    print(f"{name} {'grouped' if grouped else 'scalar'}: variance {e_var:.2e} predictive {e_cov:.2e} (diag form {e_diag:.2e}) "
          f"mean {e_mean:.2e}")
    assert e_var <= VARIANCE_TOL and e_cov <= PREDICT_TOL and e_diag <= PREDICT_TOL and e_mean <= MEAN_TOL


# measured on MI355X, per block |Lam0_l.sum() - sum of compute_ggn_diag over the block's slice| / that sum (both the
# trace of the exact block at N/M = 1, from two independent kernels), worst block of a net, and [either side against the
# helper's ggn_diag_ref]:
#   sine_regressor 8.32e-8 [3.32e-7]   xor_classifier 4.26e-8 [3.98e-8]   mlp_ragged 7.57e-9 [2.78e-8]
#   resnet_tiny    2.49e-8 [1.10e-7]   resnet50_tiny  6.19e-8 [2.34e-7]   flat_head  1.47e-8 [5.64e-8]
#   stem_net       2.73e-8 [1.09e-7]
TRACE_TOL = 1.4e-6             # 4 x 3.32e-7, the float32 sweep against the helper


@pytest.mark.parametrize("name", kf.NETS)
def test_scales_sum_to_the_trace_of_the_exact_block(name):
    """Q orthonormal: sum(diag(Q^T G Q)) = tr G = the sum of the GGN diagonal over the block's slice, which
    ``compute_ggn_diag`` forms with the square-sum sweep, a kernel that shares nothing with this one.  Lam0 is summed over
    the M examples, as the diagonal at N/M = 1 is; the regressor's exp(-logvar) goes on Lam0."""
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    blocks, ortho = _orthonormal(h)
    Lams = compute_ekfac_scales(state, Z, model_type, ortho)
    diag = compute_ggn_diag(state, Z, model_type).double()
    scale = ref.recal(state, h["M"], model_type, None)
    worst, worst_ref = 0.0, 0.0
    for b, Lam in zip(blocks, Lams):
        sl = slice(b.off, b.off + b.Mt * b.N)
        got, other, want = scale * float(Lam.sum()), float(diag[sl].sum()), float(h["diag1"][sl].sum())
        worst = max(worst, abs(got - other) / want)
        worst_ref = max(worst_ref, abs(got - want) / want, abs(other - want) / want)
    print(f"{name}: trace against compute_ggn_diag {worst:.2e}  [against the helper {worst_ref:.2e}]")
    assert worst <= TRACE_TOL and worst_ref <= TRACE_TOL


@pytest.mark.parametrize("name", kf.NETS)
def test_corrected_block_is_never_further_from_the_exact_block_than_kfac(name):
    """||G_l - Q diag(recal Lam0) Q^T||_F <= ||G_l - c_l A_l (x) S_l||_F (1 + 1e-10) for every block of at most 4096
    parameters, G_l the exact block from the float64 Jacobian, Q the product's orthonormal basis, Lam0 the product's
    scales, A_l and S_l the helper's float64 factors; on the conv nets strictly, by more than 1e-6 relative, on a block
    with T_l > 1.  One kind of block is exempt from the inequality, because there it compares two rounding errors: the
    final Dense of a Gaussian head, where G_l = c_l A_l (x) S_l identically (S_l = M I).  There both errors are asked to
    be rounding: at most SCALES_TOL ||G_l||_F (measured on MI355X, sine_regressor: EKFAC 5.1e-8, KFAC 0).

    Measured on MI355X, errors as fractions of ||G_l||_F, EKFAC / KFAC: the conv blocks (T_l > 1) between 0.026 / 0.906
    (resnet50_tiny, 1x1 16 -> 4) and 0.899 / 1.008 (stem_net, first conv), every one strict; the narrowest margins are
    final Dense blocks, 1.116e-4 / 1.120e-4 (stem_net) and 1.153e-2 / 1.166e-2 (flat_head)."""
    h = _helper(name)
    state, Z, model_type, M = h["state"], h["Z"], h["model_type"], h["M"]
    blocks, ortho = _orthonormal(h)
    Lams = compute_ekfac_scales(state, Z, model_type, ortho)
    recal = ref.recal(state, M, model_type, None)
    covered, strict, skipped = [], [], []
    for b, (u, off, Mt, N, T, _), (Ut, Ub), Lam, A, S in zip(blocks, kf.blocks_of(state), _cpu(ortho), Lams, h["As"], h["Ss"]):
        if Mt * N > er.DENSE_CAP:
            skipped.append((off, Mt, N))
            continue
        G = recal * er.exact_block(h["J"], h["H"], off, Mt, N)
        Q = torch.kron(Ut, Ub)
        e_ek = er.frobenius_error(G, Q, recal * Lam.cpu().reshape(-1))
        e_kf = float(torch.linalg.norm(G - recal / (M * T) * torch.kron(A, kf.head_factor(state, u, S, model_type))))
        nG = float(torch.linalg.norm(G))
        print(f"{name} block at {off} ({Mt}, {N}) T={T}: EKFAC {e_ek / nG:.3e}  KFAC {e_kf / nG:.3e}  of ||G||_F")
        covered.append(T)
        if model_type == "regressor" and b.final:
            assert e_ek <= SCALES_TOL * nG and e_kf <= SCALES_TOL * nG
            continue
        assert e_ek <= e_kf * (1 + 1e-10)
        if T > 1 and e_ek < e_kf * (1 - 1e-6):
            strict.append(off)
    # nothing is skipped that kfac_ref.covariance_blocks could build (it builds every block of these nets)
    assert not skipped, skipped
    if name in CONV_NETS:
        assert any(T > 1 for T in covered) and strict


# measured on MI355X on one bound example of the dense nets: max|recal Lam - c lam (x) mu| / max(c lam (x) mu), and
# max|predict_lla_ekfac - predict_lla_kfac| / max|.| (full covariance):
#   sine_regressor 6.42e-8, 2.24e-11   xor_classifier 1.16e-8, 2.23e-12   mlp_ragged 6.45e-9, 6.76e-12
# The scales differ from KFAC's eigenvalue products by the float32 rounding of the rows against that of the factors.  The
# predictives agree far below that: with one example the corrected entries of R are the few with c lam mu >> 1, whose
# directions the prior (alpha = 1e-3 of the top curvature) leaves about 1e-3 of the predictive variance.
EXACT_TOL = 2.6e-7             # 4 x 6.42e-8
EXACT_PREDICT_TOL = 9.0e-11    # 4 x 2.24e-11


@pytest.mark.parametrize("name", kf.DENSE_ONLY)
def test_one_example_on_a_dense_net_reproduces_kfac(name):
    h = _helper(name)
    state, model_type, alpha = h["state"], h["model_type"], h["alpha"]
    Z1 = h["Z"][:1]
    blocks, As, Ss, M = compute_kfac_factors(state, Z1, model_type)
    D = flatten_nn_params(state.params)[0].numel()
    recal = ref.recal(state, 1, model_type, N_FULL)
    kfits = kfac.fit_blocks(blocks, As, Ss, [kfac.block_prior_rows(alpha, b, D) for b in blocks], recal, M, model_type != "regressor")
    Lams = compute_ekfac_scales(state, Z1, model_type, [(f[0], f[2]) for f in kfits])
    e_l = max(_rel(recal * Lam, (c * torch.outer(lam, mu)).cpu()) for Lam, (_, _, _, lam, mu, c) in zip(Lams, kfits))
    ek = predict_lla_ekfac(state, h["Xnew"], Z1, model_type, alpha, full_set_size=N_FULL, cov="full")
    kk = predict_lla_kfac(state, h["Xnew"], Z1, model_type, alpha, full_set_size=N_FULL, cov="full")
    e_p = _rel(ek.covariance(), kk.covariance().cpu())
    print(f"{name}: one example  recal Lam against c lam (x) mu {e_l:.2e}  predictive against KFAC {e_p:.2e}")
    assert e_l <= EXACT_TOL and e_p <= EXACT_PREDICT_TOL


@pytest.mark.parametrize("name", kref.NETS)
def test_final_dense_block_in_closed_form(name):
    """Lam[j][l] = sum_i (V^T phit_i)_j^2 (Ub^T H_i Ub)_{ll} from the float64 features and probabilities alone"""
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    _, fits, *_ = ekfac._cached_fit(state, Z, model_type, h["alpha"], N_FULL, None)
    bases = [(V, Ub) for V, _, Ub in fits]
    Lam = compute_ekfac_scales(state, Z, model_type, bases)[-1]
    V, Ub = _cpu(bases)[-1]
    e = _rel(Lam, er.scales_final_dense(state, Z, model_type, V, Ub))
    print(f"{name}: final Dense block against the closed form {e:.2e}")
    assert e <= SCALES_TOL


# The float32 factor rows of an example do not depend on how the examples and classes are chunked, so a chunked pass is
# the same float64 squares in another grouping: the order of tests/test_kfac.py's SPLIT_TOL.  Measured on MI355X, worst
# block, example chunks / class chunks: sine_regressor 3.60e-16 / 0, xor_classifier 3.54e-16 / 3.54e-16, mlp_ragged
# 5.51e-16 / 3.67e-16, resnet_tiny 2.58e-16 / 4.07e-16, resnet50_tiny 4.11e-16 / 3.36e-16, flat_head 3.80e-16 / 3.80e-16,
# stem_net 2.17e-16 / 2.17e-16
SPLIT_TOL = 1e-12


@pytest.mark.parametrize("name", kf.NETS)
def test_example_and_class_chunks_agree_with_the_unsplit_pass(name):
    h = _helper(name)
    state, Z, model_type = h["state"], h["Z"], h["model_type"]
    M, K = h["M"], h["f_new"].shape[1]
    _, ortho = _orthonormal(h)
    Lams = compute_ekfac_scales(state, Z, model_type, ortho)
    Le = compute_ekfac_scales(state, Z, model_type, ortho, example_chunk=max(1, M // 2))
    Lc = compute_ekfac_scales(state, Z, model_type, ortho, class_chunk=max(1, K // 2))
    e_e = max(_rel(a, r) for a, r in zip(Le, Lams))
    e_c = max(_rel(a, r) for a, r in zip(Lc, Lams))
    print(f"{name}: chunked against unsplit  examples {e_e:.2e}  classes {e_c:.2e}")
    assert e_e <= SPLIT_TOL and e_c <= SPLIT_TOL


# measured on MI355X: max|. - ref| / max|ref| of the draws f + J dtheta against the helper's, same seeded dtheta:
# sine_regressor 8.50e-7, xor_classifier 2.46e-7, mlp_ragged 4.20e-7, resnet_tiny 2.60e-7, resnet50_tiny 3.79e-7,
# flat_head 1.74e-7, stem_net 1.83e-7
SCALABLE_TOL = 3.4e-6          # 4 x 8.50e-7


@pytest.mark.parametrize("name", kf.NETS)
def test_scalable_draws_match_the_helper_for_the_same_seeded_draws(name):
    h = _helper(name)
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    out = predict_lla_ekfac_scalable(state, h["Xnew"], Z, model_type, alpha, key=5, full_set_size=N_FULL, num_samples=4)
    K = h["f_new"].shape[1]
    assert out.shape == (4, 5, K) and out.is_cuda and out.dtype == F32
    post = posterior_lla_ekfac(state, Z, model_type, alpha, full_set_size=N_FULL)
    d_theta = (post.sample((4,), seed=5, dtype=F64) - post.mean()).cpu()
    want = h["f_new"][None] + torch.einsum("bkd,sd->sbk", h["J_new"], d_theta)
    e = _rel(out, want)
    print(f"{name}: scalable draws {e:.2e}")
    assert e <= SCALABLE_TOL


# measured on MI355X: |got - want| / |want| of the evidence against the helper's spectrum in the product's basis:
# sine_regressor 3.07e-8 (-41.2472873009 against -41.2472860345), xor_classifier 1.46e-8 (-51.6105058164 against
# -51.610505061), mlp_ragged 3.13e-8 (-176.456678462 against -176.456672947), resnet_tiny 2.62e-8 (-419.765050884 against
# -419.765061866), resnet50_tiny 2.58e-8 (-253.402629709 against -253.402636234), flat_head 1.28e-8 (-73.2662010089
# against -73.2662019455), stem_net 1.19e-8 (-45.1826427976 against -45.1826422622)
LML_TOL = 1.3e-7               # 4 x 3.13e-8


@pytest.mark.parametrize("name", kf.NETS)
def test_evidence_matches_the_helper_spectrum_and_the_fit_does_not_lose_evidence(name, monkeypatch):
    h = _helper(name)
    state, Z, model_type, alpha, M = h["state"], h["Z"], h["model_type"], h["alpha"], h["M"]
    seen = []
    inner = ekfac.compute_ekfac_scales
    monkeypatch.setattr(ekfac, "compute_ekfac_scales", lambda s, z, m, bases, **kw: (seen.append(bases), inner(s, z, m, bases, **kw))[1])
    got = log_marginal_likelihood_ekfac(alpha, Z, state, model_type, full_set_size=N_FULL)
    assert len(seen) == 1                                           # the basis the product used: orthonormal
    for Ut, Ub in seen[0]:
        assert _rel(Ut.T @ Ut, torch.eye(Ut.shape[0], dtype=F64)) <= 1e-12 and _rel(Ub.T @ Ub, torch.eye(Ub.shape[0], dtype=F64)) <= 1e-12
    spec = er.spectrum_ref(state, er.scales_ref(h["J"], h["H"], state, _cpu(seen[0])), model_type, h["diag1"])
    theta = flatten_nn_params(state.params)[0].double()
    want = ref.lml_ref(alpha, spec, theta.numel(), float((theta ** 2).sum()), N_FULL / M)
    e = abs(got - want) / abs(want)
    print(f"{name}: evidence got {got:.12g} want {want:.12g} rel {e:.2e}")
    assert e <= LML_TOL
    a_fit, hist = fit_alpha_ekfac(Z, state, model_type, full_set_size=N_FULL, alpha0=alpha, steps=20)
    assert len(hist) == 20 and abs(hist[0][0] - alpha) <= 1e-14 * alpha and abs(hist[0][1] - got) <= 1e-9 * abs(got)
    assert a_fit > 0 and a_fit == a_fit and a_fit != float("inf")
    assert log_marginal_likelihood_ekfac(a_fit, Z, state, model_type, full_set_size=N_FULL) >= hist[0][1]


def test_eval_dataset_probit_fits_the_posterior_once(monkeypatch):
    h = _helper("xor_classifier")
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    calls = []
    inner = ekfac.compute_ekfac_scales
    monkeypatch.setattr(ekfac, "compute_ekfac_scales", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    nll, acc, brier, ece_, probs, labels = eval_dataset_probit(state, [(X[:8], y[:8]), (X[8:], y[8:])], Z, alpha, N_FULL,
                                                               model_type, posterior="ekfac")
    assert len(calls) == 1                                          # one fit for both batches
    assert probs.shape == (16, 2) and labels.shape == (16,)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), (nll, acc, brier, ece_)))
    assert bool(torch.isfinite(probs).all()) and bool(((probs.sum(-1) - 1).abs() < 1e-9).all())
    assert ekfac._FIT_CACHE
    clear_engine_cache()
    assert not ekfac._FIT_CACHE                                     # clear_engine_cache drops the fit


def test_engine_method_checks_its_operands():
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    blocks = eng.kfac_blocks()
    bases = [(torch.eye(b.Mt, device=DEV, dtype=F64), torch.eye(b.N, device=DEV, dtype=F64)) for b in blocks]
    Lams = [torch.zeros(b.Mt, b.N, device=DEV, dtype=F64) for b in blocks]
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_eigen_sqsums(bases[:1], Lams)
    with pytest.raises(ValueError, match="layer blocks need"):
        eng.kfac_eigen_sqsums(bases, Lams[:1])
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_eigen_sqsums([(bases[0][0].float(), bases[0][1]), bases[1]], Lams)
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_eigen_sqsums([bases[0], (bases[1][0], bases[1][1].cpu())], Lams)
    with pytest.raises(ValueError, match="contiguous float64 device matrix"):
        eng.kfac_eigen_sqsums(bases, [Lams[0].T, Lams[1]])
    with pytest.raises(ValueError, match="class_chunk must be positive"):
        eng.kfac_eigen_sqsums(bases, Lams, class_chunk=0)
    assert all(float(Lam.abs().sum()) == 0.0 for Lam in Lams)
    # the identity basis: the squares of the factor rows themselves, i.e. the GGN diagonal of the square-sum sweep
    eng.kfac_eigen_sqsums(bases, Lams)
    diag = compute_ggn_diag(h["state"], h["Z"], h["model_type"]).double()
    worst = max(_rel(Lam.reshape(-1), diag[b.off:b.off + b.Mt * b.N].cpu()) for b, Lam in zip(blocks, Lams))
    print(f"flat_head: identity basis against compute_ggn_diag {worst:.2e}")
    assert worst <= TRACE_TOL
