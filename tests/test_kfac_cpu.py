"""CPU checks of the Kronecker-factored posterior over all layers: the float64 helper (``tests/kfac_ref.py``) against
the autograd Jacobian and the oracle's dense GGN, then the package's host algebra (``kfac.py``,
``distributions.KFACNormal``), fed the helper's factors on the CPU, against the helper's dense route, and the refusals.

Everything is float64 on the host.  alpha = 1e-3 max_l c_l lam_max(A_l) mu_max(S_l) keeps the condition of every
block's dense solve at most 1002 (asserted by the helper), so the bound 1e-11 max|ref| is 100 cond 2^-53, as in
tests/test_last_layer_kron_cpu.py.
"""
import functools

import pytest
import torch

import kfac_ref as kf
import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd import distributions, kfac
from lip_amd.distributions import KFACNormal, KroneckerNormal
from lip_amd.lla import posterior_lla_kfac, predict_lla_kfac
from lip_amd.netspec import NetSpec
from lip_amd.prior import GroupedPrior
from lip_amd.toymodels import create_state
from lip_amd.utils import flatten_nn_params
from oracle.ggn import compute_ggn_dense

F64 = torch.float64
TOL = 1e-11
N_FULL = kf.N_FULL


@functools.lru_cache(maxsize=None)
def _helper(name):
    state, Z, model_type = kf.make_case(name)
    f, ats, Gs = kf.patches_and_cotangents(state, Z)
    As, Ss, M = kf.factors_from(f, ats, Gs, model_type)
    return state, Z, model_type, ats, Gs, As, Ss, M


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", kf.NETS)
def test_patches_and_cotangents_reproduce_the_autograd_jacobian(name):
    """sum_t at_t G_t^T is the layer block of the Jacobian: pins the patch order, the padding side and the BN scale"""
    state, Z, model_type, ats, Gs, *_ = _helper(name)
    _, J = ref.jac64(state, Z, model_type)
    n, K, D = J.shape
    table = kfac.block_table(state)
    assert [(b.off, b.Mt, b.N, b.T, b.bias) for b in table] == [t[1:] for t in kf.blocks_of(state)]
    worst = 0.0
    for (u, off, Mt, N, T, _), at, G in zip(kf.blocks_of(state), ats, Gs):
        got = torch.einsum("ite,iktn->iken", at, G).reshape(n, K, Mt * N)
        want = J[:, :, off:off + Mt * N]
        e = _err(got, want)
        worst = max(worst, e)
        assert e <= 1e-12, (name, u.kernel, e)
    print(f"{name}: worst block against the autograd Jacobian {worst:.2e}")
    # the blocks and the remainder cover the vector exactly once
    rem = kfac.remainder_indices(table, D)
    assert torch.equal(rem, kf.remainder_of(state))
    assert rem.numel() + sum(b.Mt * b.N for b in table) == D


@pytest.mark.parametrize("name", kf.DENSE_ONLY)
def test_kronecker_curvature_is_exact_for_one_example_of_a_dense_net(name):
    """M = 1 and every T_l = 1: c_l A_l (x) S_l is the diagonal block of the oracle's dense GGN"""
    state, Z, model_type = kf.make_case(name)
    Z = Z[:1]
    As, Ss, M = kf.factors_ref(state, Z, model_type)
    G = compute_ggn_dense(state, Z, model_type, full_set_size=N_FULL)[0]
    c = ref.recal(state, 1, model_type, N_FULL)
    for (u, off, Mt, N, T, _), A, S in zip(kf.blocks_of(state), As, Ss):
        assert T == 1
        sl = slice(off, off + Mt * N)
        assert _err(c * torch.kron(A, S), G[sl, sl]) <= 1e-12


@pytest.mark.parametrize("name", kref.NETS)
def test_final_block_is_the_last_layer_kron_factor_pair(name):
    state, Z, model_type, ats, Gs, As, Ss, M = _helper(name)
    A, Bf, M2 = kref.factors_ref(state, Z, model_type)
    assert M == M2 and _err(As[-1], A) <= 1e-12 and _err(Ss[-1], Bf) <= 1e-12
    assert kfac.block_table(state)[-1].final and not any(b.final for b in kfac.block_table(state)[:-1])


@functools.lru_cache(maxsize=None)
def _fitted(name, grouped):
    state, Z, model_type, ats, Gs, As, Ss, M = _helper(name)
    alpha = kf.alpha_for(state, As, Ss, M, model_type, N_FULL)
    prior = kf.split_prior(state, alpha) if grouped else alpha
    a = kf.prior_vector(state, alpha, grouped)
    D = a.numel()
    table = kfac.block_table(state)
    rows = [kfac.block_prior_rows(prior, b, D) for b in table]
    for b, r in zip(table, rows):
        assert torch.equal(r.repeat_interleave(b.N), a[b.off:b.off + b.Mt * b.N])
    fits = kfac.fit_blocks(table, As, Ss, rows, ref.recal(state, M, model_type, N_FULL), M, model_type != "regressor")
    rem = kf.remainder_of(state)
    rem_var = 1.0 / (a[rem] + kf.ggn_diag_ref(state, Z, model_type, N_FULL)[rem])
    post = kfac.posterior_from_fit(torch.zeros(D, dtype=F64), table, fits, rem, rem_var, a[rem])
    cov_blocks, logdet = kf.covariance_blocks(state, As, Ss, M, model_type, a, N_FULL)
    logdet += float(-torch.log(a[rem] * rem_var).sum())
    return state, Z, model_type, post, fits, cov_blocks, logdet, rem, rem_var


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", kf.NETS)
def test_factored_algebra_matches_the_dense_route(name, grouped):
    state, Z, model_type, post, fits, cov_blocks, logdet, rem, rem_var = _fitted(name, grouped)
    assert isinstance(post, KFACNormal) and all(isinstance(kn, KroneckerNormal) for _, kn in post.blocks)
    e_var = _err(post.variance(), kf.variance_ref(state, cov_blocks, rem, rem_var))
    e_cov = max(_err(kn.covariance(), S) for (_, kn), (_, S) in zip(post.blocks, cov_blocks) if S.shape[0] <= 8192)
    e_ld = abs(float(post.log_det_precision_ratio()) - logdet) / abs(logdet)
    # the closed-form predictive in torch: sum_l sum_{j,l} R T_k T_m with T = V^T J Ub, plus the remainder
    _, J = ref.jac64(state, kref.new_points(Z, 3, 7), model_type)
    want = kf.predict_dense(J, cov_blocks, rem, rem_var)
    got = torch.einsum("bkd,d,bmd->bkm", J[:, :, rem], rem_var, J[:, :, rem])
    for b, (V, R, Ub, *_r) in zip(kfac.block_table(state), fits):
        Tm = V.T @ J[:, :, b.off:b.off + b.Mt * b.N].reshape(J.shape[0], J.shape[1], b.Mt, b.N) @ Ub
        got = got + torch.einsum("jl,bkjl,bmjl->bkm", R, Tm, Tm)
    e_pred = _err(got, want)
    print(f"{name} {'grouped' if grouped else 'scalar'}: variance {e_var:.2e} block covariance {e_cov:.2e} "
          f"logdet {e_ld:.2e} predictive {e_pred:.2e}")
    assert post.variance().shape == post.mean().shape and torch.equal(post.stddev(), torch.sqrt(post.variance()))
    assert max(e_var, e_cov, e_ld, e_pred) <= TOL


def test_sample_applied_to_a_fixed_E_reproduces_the_square_root(monkeypatch):
    """with E the identity, block by block, the D draws minus the mean are the rows of (Sigma^(1/2))^T: X^T X = Sigma"""
    state, Z, model_type, post, fits, cov_blocks, logdet, rem, rem_var = _fitted("stem_net", True)
    D = post.mean().numel()
    spans = [(off, kn.R.shape[0] * kn.R.shape[1]) for off, kn in post.blocks] + [None]
    calls = []

    def fixed(shape, **kw):
        span = spans[len(calls)]
        calls.append(shape)
        cols = torch.arange(span[0], span[0] + span[1]) if span is not None else rem
        return torch.eye(D, dtype=F64)[:, cols].reshape(shape)

    monkeypatch.setattr(distributions.torch, "randn", fixed)
    X = post.sample((D,), seed=0, dtype=F64) - post.mean()
    monkeypatch.undo()
    assert len(calls) == len(spans) and X.shape == (D, D)
    Sigma = torch.diag(kf.variance_ref(state, [], rem, rem_var))
    for off, S in cov_blocks:
        Sigma[off:off + S.shape[0], off:off + S.shape[0]] = S
    assert _err(X.T @ X, Sigma) <= TOL
    # seeded draws repeat, in the dtype asked for
    x = post.sample((4,), seed=3)
    assert x.shape == (4, D) and x.dtype == torch.float32 and torch.equal(x, post.sample(4, seed=3))


def test_prior_varying_inside_a_row_is_refused():
    state, Z, model_type = kf.make_case("flat_head")
    D = flatten_nn_params(state.params)[0].numel()
    table = kfac.block_table(state)
    for b in table:
        cut = b.off + (1 if b.bias else 0) * b.N + 1                  # inside the first kernel row
        prior = GroupedPrior.from_table([("a", [(0, cut)]), ("b", [(cut, D - cut)])], [1.0, 2.0], D)
        with pytest.raises(ValueError, match="constant along"):
            kfac.block_prior_rows(prior, b, D)
        with pytest.raises(ValueError, match="constant along"):       # before any engine is bound: runs without a GPU
            posterior_lla_kfac(state, Z, model_type, prior)
        same = GroupedPrior.from_table([("a", [(0, cut)]), ("b", [(cut, D - cut)])], [1.5, 1.5], D)
        assert bool((kfac.block_prior_rows(same, b, D) == 1.5).all())
    state, _, _ = kf.make_case("resnet_tiny")                          # blocks without a bias row
    D = flatten_nn_params(state.params)[0].numel()
    tensor = GroupedPrior(state.params, 2.0, "tensor")
    for b in kfac.block_table(state):
        assert bool((kfac.block_prior_rows(tensor, b, D) == 2.0).all())
    nb = next(b for b in kfac.block_table(state) if not b.bias)
    assert kfac.prior_rows_no_bias(3.0, nb.off, nb.Mt, nb.N, D).shape == (nb.Mt,)


def test_bias_and_kernel_that_are_not_adjacent_are_refused():
    net = NetSpec((4,))
    net.dense(net.dense(0, "Dense_0", 5, act="relu"), "Dense_1", 3)
    state = create_state(net, 0, dtype=F64)
    assert [b.off for b in kfac.block_table(state)] == [0, 25]
    u = net.units[0]
    state.params["params"]["Z_0"] = {"bias": state.params["params"]["Dense_0"].pop("bias")}
    u.bias = ("params", "Z_0", "bias")
    with pytest.raises(ValueError, match="directly before its kernel"):
        kfac.block_table(state)
    with pytest.raises(ValueError, match="directly before its kernel"):
        posterior_lla_kfac(state, torch.zeros(2, 4, dtype=F64), "classifier", 1.0)


def test_cov_argument_is_checked():
    state, Z, model_type = kf.make_case("xor_classifier")
    with pytest.raises(ValueError, match="'diag' or 'full'"):
        predict_lla_kfac(state, Z[:2], Z, model_type, 1.0, cov="dense")


def test_kfac_normal_checks_its_cover():
    kn = KroneckerNormal(torch.zeros(6, dtype=F64), torch.eye(3, dtype=F64), torch.ones(3, 2, dtype=F64), torch.eye(2, dtype=F64))
    with pytest.raises(ValueError, match="exactly once"):
        KFACNormal(torch.zeros(8, dtype=F64), [(0, kn)], (torch.tensor([5, 6]), torch.ones(2, dtype=F64)))
    with pytest.raises(ValueError, match="exactly once"):           # a repeated remainder index counts twice
        KFACNormal(torch.zeros(8, dtype=F64), [(2, kn)], (torch.tensor([0, 0, 1]), torch.ones(3, dtype=F64)))
    post = KFACNormal(torch.zeros(8, dtype=F64), [(2, kn)], (torch.tensor([0, 1]), torch.full((2,), 0.5, dtype=F64)), 1.0)
    assert torch.equal(post.variance(), torch.tensor([0.5, 0.5, 1, 1, 1, 1, 1, 1], dtype=F64))
    assert abs(float(post.log_det_precision_ratio()) - 2 * 0.6931471805599453) < 1e-15
