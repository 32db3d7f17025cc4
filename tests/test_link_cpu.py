"""CPU: the replay of the Monte-Carlo link (tests/link_ref.py) pinned against facts that do not depend on it, and the
closed-form links and refusals of ``lip_amd.link`` that need no device.

The Monte-Carlo band is |p_mc - p_quadrature| <= 5 * 0.5 / sqrt(S): the standard deviation of a probability is at most
1/2, five of them at S = 4096 draws; the seeds are fixed here.  Worst measured |p_mc - p_quadrature| / band over the
18 (mean, variance, seed) cases: 0.22.
"""
import math

import numpy as np
import pytest
import torch

import krylov_harness as kh
import link_ref as lr
from lip_amd.distributions import MultivariateNormalFullCovariance
from lip_amd.link import bridge_predictive, link_predictive
from lip_amd.lla import probit_predictive

F64 = torch.float64


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 11])
def test_box_muller_moments(seed):
    eps = lr.normals(4, 64, 256, seed, example_offset=7).reshape(-1)
    N = eps.size
    assert N == 2 ** 16 and np.isfinite(eps).all()
    assert abs(eps.mean()) <= 5 / math.sqrt(N)
    assert abs(eps.var() - 1.0) <= 5 * math.sqrt(2.0 / N)


def test_replay_is_chunk_invariant():
    g = np.random.default_rng(3)
    mean, var = g.uniform(-8, 8, (7, 10)), g.uniform(0, 4, (7, 10))
    A = g.standard_normal((7, 10, 10))
    L = np.stack([lr.cholesky_semidefinite(a @ a.T)[0] for a in A])
    for kw in (dict(var=var), dict(L=L)):
        whole = lr.replay(mean, S=9, seed=5, example_offset=11, **kw)
        for a, b in ((0, 3), (2, 5), (6, 7)):
            part = lr.replay(mean[a:b], S=9, seed=5, example_offset=11 + a, **{k: v[a:b] for k, v in kw.items()})
            assert np.array_equal(part[0], whole[0][a:b]) and np.array_equal(part[1], whole[1][a:b])


def test_link_stream_differs_from_the_head_sampler():
    """same (g, s, seed): the link's counter (g, s, 0, 0x4C4E4B31) and the head sampler's (g, s, 0x9E3779B9, 0xBB67AE85)
    give different first words, draw for draw"""
    g, s = np.meshgrid(np.arange(5, 37, dtype=np.uint64), np.arange(33, dtype=np.uint64), indexing="ij")
    g, s = g.reshape(-1), s.reshape(-1)
    for seed in (0, 1234, 2 ** 63 + 11):
        link = lr.first_words(g, s, seed)[0]
        head = lr.first_words(g, s, seed, c2=0x9E3779B9, tag=lr.HEAD_TAG)[0]
        assert (link != head).all()
        assert np.array_equal(head, kh._lib_words((s << np.uint64(32)) | g, seed)[0])        # that IS the head sampler's call


def test_cholesky_rule():
    g = np.random.default_rng(0)
    v = g.standard_normal(9)
    L, dead = lr.cholesky_semidefinite(np.outer(v, v))
    sign = np.sign(v[0])                                                   # L_00 = |v_0| > 0 fixes the sign of the column
    assert dead == 0 and np.allclose(L[:, 0], sign * v, rtol=1e-14, atol=0) and not L[:, 1:].any()
    u = v / np.linalg.norm(v)                                              # unit vector: the first column is v / |v|
    L1, dead = lr.cholesky_semidefinite(np.outer(u, u))
    assert dead == 0 and np.allclose(L1[:, 0], sign * u, rtol=1e-13, atol=0) and not L1[:, 1:].any()
    A = g.standard_normal((12, 12))
    C = A @ A.T + 0.1 * np.eye(12)
    L, dead = lr.cholesky_semidefinite(C)
    ref = np.linalg.cholesky(C)
    assert dead == 0 and np.abs(L - ref).max() <= 1e-12 * np.abs(ref).max()
    C[3, 3] = -1.0
    L, dead = lr.cholesky_semidefinite(C)
    assert dead == 1 and not L.any()
    C[3, 3] = 1.0
    C[5, 2] = np.nan
    assert lr.cholesky_semidefinite(C)[1] == 1
    C[5, 2], C[2, 5] = 0.0, np.nan                                         # the upper triangle is not read
    assert lr.cholesky_semidefinite(C)[1] == 0
    Z, dead = lr.cholesky_semidefinite(np.zeros((4, 4)))
    assert dead == 0 and not Z.any()


def test_rank_one_first_column_is_v_over_its_norm():
    v = np.array([2.0, -1.0, 0.5, 3.0])
    L, dead = lr.cholesky_semidefinite(np.outer(v, v))
    assert dead == 0
    assert np.allclose(L[:, 0] / np.linalg.norm(L[:, 0]), v / np.linalg.norm(v), rtol=1e-15, atol=0)
    assert np.allclose(L[:, 0], v, rtol=1e-15, atol=0) and not L[:, 1:].any()


MC_S = 4096


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 63 + 11])
def test_mc_replay_against_quadrature(seed):
    cases = [(m, v) for m in (0.0, 1.0, -3.0) for v in (0.25, 4.0)]
    mean = np.array([[m, 0.0] for m, _ in cases])
    var = np.array([[v, 0.25] for _, v in cases])
    probs, _ = lr.replay(mean, var=var, S=MC_S, seed=seed)
    band = 5 * 0.5 / math.sqrt(MC_S)
    worst = 0.0
    for i, (m, v) in enumerate(cases):
        want = lr.sigmoid_expectation(m, v + 0.25)
        assert abs(want - lr.sigmoid_expectation(m, v + 0.25, nodes=160)) <= 1e-6      # the quadrature has converged
        worst = max(worst, abs(probs[i, 0] - want) / band)
        assert abs(probs[i, 0] - want) <= band, (m, v, probs[i, 0], want)
        assert abs(probs[i].sum() - 1.0) <= 1e-12
    print(f"seed {seed}: worst |p_mc - p_quadrature| / band {worst:.3f}")


def test_bridge_anchors():
    probs, a = bridge_predictive(torch.zeros(1, 2, dtype=F64), torch.ones(1, 2, dtype=F64), return_alpha=True)
    assert a.tolist() == [[0.5, 0.5]] and probs.tolist() == [[0.5, 0.5]]
    # by hand, K = 2, m = (log 3, 0), v = (1, 2): sum_l exp(-m_l) = 4/3; a_0 = (0 + 3 * (4/3) / 4) / 1 = 1,
    # a_1 = (0 + 1 * (4/3) / 4) / 2 = 1/6; probs = (6/7, 1/7)
    m = torch.tensor([[math.log(3.0), 0.0]], dtype=F64)
    v = torch.tensor([[1.0, 2.0]], dtype=F64)
    probs, a = bridge_predictive(m, v, return_alpha=True)
    assert torch.allclose(a, torch.tensor([[1.0, 1.0 / 6.0]], dtype=F64), rtol=1e-14, atol=0)
    assert torch.allclose(probs, torch.tensor([[6.0 / 7.0, 1.0 / 7.0]], dtype=F64), rtol=1e-14, atol=0)
    assert torch.equal(link_predictive(m, v, link="bridge"), probs)
    # K = 3 keeps the constant term: m = 0, v = 1 -> a_k = 1 - 2/3 + 3/9 = 2/3
    _, a3 = bridge_predictive(torch.zeros(1, 3, dtype=F64), torch.ones(1, 3, dtype=F64), return_alpha=True)
    assert torch.allclose(a3, torch.full((1, 3), 2.0 / 3.0, dtype=F64), rtol=1e-15, atol=0)


def test_bridge_norm_is_scale_invariant():
    g = torch.Generator().manual_seed(1)
    m = torch.randn(5, 7, dtype=F64, generator=g)
    v = torch.rand(5, 7, dtype=F64, generator=g) + 0.1
    base = link_predictive(m, v, link="bridge_norm")
    assert bool(((base.sum(-1) - 1).abs() < 1e-14).all())
    for c in (0.25, 3.0, 40.0):
        assert torch.allclose(link_predictive(c * m, c * c * v, link="bridge_norm"), base, rtol=1e-12, atol=0)
    assert not torch.allclose(link_predictive(3.0 * m, 9.0 * v, link="bridge"), link_predictive(m, v, link="bridge"))


def test_probit_link_is_probit_predictive():
    g = torch.Generator().manual_seed(2)
    m = torch.randn(6, 5, dtype=F64, generator=g)
    A = torch.randn(6, 5, 5, dtype=F64, generator=g)
    cov = A @ A.transpose(-1, -2)
    v = torch.diagonal(cov, dim1=-2, dim2=-1)
    want = probit_predictive(m, v)
    assert torch.equal(link_predictive(m, v), want) and torch.equal(link_predictive(m, v, link="probit"), want)
    dist = MultivariateNormalFullCovariance(loc=m, covariance_matrix=cov)
    assert torch.equal(link_predictive(dist, link="probit"), want)         # a full covariance contributes its diagonal
    assert torch.equal(link_predictive(m, cov, link="probit"), want)
    one = MultivariateNormalFullCovariance(loc=m[:1].squeeze(), covariance_matrix=cov[:1])    # loc of one point comes squeezed
    assert torch.equal(link_predictive(one), want[:1])


def test_refusals():
    m, v = torch.zeros(4, dtype=F64), torch.ones(4, dtype=F64)
    for link in ("probit", "mc", "bridge", "bridge_norm"):
        with pytest.raises(ValueError, match="classifier"):
            link_predictive(m, v, link=link)                               # a regressor's (B,) mean and variances
        with pytest.raises(ValueError, match="classifier"):
            link_predictive(MultivariateNormalFullCovariance(loc=m, covariance_matrix=torch.diag(v)), link=link)
    wide = MultivariateNormalFullCovariance(loc=torch.zeros(2, 65, dtype=F64),
                                            covariance_matrix=torch.eye(65, dtype=F64).expand(2, 65, 65))
    with pytest.raises(ValueError, match='cov="diag"'):
        link_predictive(wide, link="mc")
    m2, v2 = torch.zeros(2, 3, dtype=F64), torch.ones(2, 3, dtype=F64)
    v2[1, 2] = 0.0
    for link in ("bridge", "bridge_norm"):
        with pytest.raises(ValueError, match="positive"):
            link_predictive(m2, v2, link=link)
    with pytest.raises(ValueError, match="link must be"):
        link_predictive(m2, v2, link="logit")
    with pytest.raises(ValueError, match="return_uncertainty"):
        link_predictive(m2, v2, link="probit", return_uncertainty=True)
    with pytest.raises(ValueError):
        link_predictive(m2, torch.ones(2, 4, dtype=F64))


def test_mutual_information_is_not_negative_on_the_replay():
    g = np.random.default_rng(5)
    mean, var = g.uniform(-8, 8, (6, 10)), g.uniform(0, 4, (6, 10))
    var[0] = 0.0                                                           # no spread: no epistemic part at all
    probs, ment, p = lr.replay(mean, var=var, S=65, seed=9, return_draws=True)
    epistemic = lr.entropy(probs) - ment
    assert (epistemic >= -1e-12).all() and abs(epistemic[0]) <= 1e-12 and epistemic[1:].min() > 0
    assert np.allclose(probs[0], lr.softmax(mean[0]), rtol=1e-13, atol=0)    # a float64 mean of 65 equal rows
