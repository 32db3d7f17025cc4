"""CPU checks of the GGN-diagonal surface: the square-sum entry points answer with status codes (never a crash) before
an engine is usable, and the diagonal-Gaussian posterior object computes what it says."""
import ctypes

import torch

from lip_amd import _native as nv
from lip_amd.distributions import MultivariateNormalDiag

LIP_ERR_ARG = 1          # include/lip.h


def test_vjp_sqsum_errors_are_status_codes_not_crashes():
    lib = nv.load()
    n = ctypes.c_int64(-1)
    assert lib.lip_vjp_sqsum(None, None, None, 1, nv.HEAD_L, 1.0, None, 0, None) == LIP_ERR_ARG   # null engine
    assert b"null engine" in lib.lip_last_error()
    assert lib.lip_vjp_sqsum_scratch(None, 1, ctypes.byref(n)) == LIP_ERR_ARG
    assert n.value == -1
    h = ctypes.c_void_p()
    assert lib.lip_engine_create(ctypes.byref(h), 10, 2, 3) == 0
    try:
        assert lib.lip_vjp_sqsum(h, None, None, 1, nv.HEAD_L, 1.0, None, 0, None) != 0          # not bound
        assert b"not bound" in lib.lip_last_error()
        assert lib.lip_vjp_sqsum_scratch(h, 1, None) == LIP_ERR_ARG                           # null output
        assert lib.lip_vjp_sqsum_scratch(h, 4, ctypes.byref(n)) != 0                              # no tape yet
    finally:
        assert lib.lip_engine_destroy(h) == 0


def test_multivariate_normal_diag_moments_and_seeded_samples():
    loc = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    var = torch.tensor([4.0, 0.25, 1.0], dtype=torch.float64)
    d = MultivariateNormalDiag(loc, variance=var)
    assert torch.equal(d.mean(), loc)
    assert torch.equal(d.variance(), var)
    assert torch.allclose(d.stddev(), torch.tensor([2.0, 0.5, 1.0], dtype=torch.float64))
    assert not hasattr(d, "covariance")
    a = d.sample(5, seed=7)
    b = d.sample((5,), seed=7)
    assert a.shape == (5, 3) and torch.equal(a, b)
    assert not torch.equal(a, d.sample(5, seed=8))
    s = d.sample(20000, seed=1)
    assert torch.allclose(s.mean(0), loc, atol=4 * 2.0 / 20000 ** 0.5)
    assert torch.allclose(s.var(0), var, rtol=4 * (2 / 20000) ** 0.5)
    e = MultivariateNormalDiag(loc, scale_diag=torch.sqrt(var))
    assert torch.allclose(e.variance(), var)
