"""CPU checks of the closed-form predictive surface: the weighted-norm entry points answer with status codes (never a
crash) before an engine is usable, the probit predictive computes the formula it names, and the polarisation identity
recovers a quadratic form from the weighted norms of the probes e_k + e_k'."""
import ctypes
import math

import torch

from lip_amd import _native as nv
from lip_amd.lla import covariance_from_polarisation, polarisation_probes, probit_predictive

LIP_ERR_ARG, LIP_ERR_STATE = 1, 3         # include/lip.h


def test_vjp_wnorm_errors_are_status_codes_not_crashes():
    lib = nv.load()
    n = ctypes.c_int64(-1)
    assert lib.lip_vjp_wnorm(None, None, None, None, 1, nv.HEAD_L, 1.0, None, 0, None) == LIP_ERR_ARG   # null engine
    assert b"null engine" in lib.lip_last_error()
    assert lib.lip_vjp_wnorm_scratch(None, 1, ctypes.byref(n)) == LIP_ERR_ARG
    assert n.value == -1
    h = ctypes.c_void_p()
    assert lib.lip_engine_create(ctypes.byref(h), 10, 2, 3) == 0
    try:
        assert lib.lip_vjp_wnorm(h, None, None, None, 1, nv.HEAD_L, 1.0, None, 0, None) != 0          # not bound
        assert b"not bound" in lib.lip_last_error()
        assert lib.lip_vjp_wnorm_scratch(h, 1, None) == LIP_ERR_ARG                                   # null output
        assert lib.lip_vjp_wnorm_scratch(h, 0, ctypes.byref(n)) == LIP_ERR_ARG                        # no probes
        assert lib.lip_vjp_wnorm_scratch(h, 4, ctypes.byref(n)) != 0                                  # no tape yet
        assert b"tape" in lib.lip_last_error()
        assert n.value == -1
    finally:
        assert lib.lip_engine_destroy(h) == 0


def test_every_sweep_entry_point_refuses_a_null_then_an_unbound_engine_by_name():
    """The seven sweeps and the two scratch queries share their checks: a null engine is LIP_ERR_ARG and an engine that
    is neither bound nor given a tape is LIP_ERR_STATE, before any other argument is looked at, and the message names
    the entry point that was called."""
    lib = nv.load()
    n = ctypes.c_int64(-1)
    calls = {
        "lip_ggn_vp": lambda e: lib.lip_ggn_vp(e, None, None, 1, 1.0, 0.0, None),
        "lip_ggn_vp_diag": lambda e: lib.lip_ggn_vp_diag(e, None, None, 1, 1.0, None, None),
        "lip_jvp": lambda e: lib.lip_jvp(e, None, None, 1, nv.HEAD_LT, 1.0, None),
        "lip_vjp": lambda e: lib.lip_vjp(e, None, None, 1, nv.HEAD_L, 1.0, None),
        "lip_vjp_rows": lambda e: lib.lip_vjp_rows(e, None, None, 1, nv.HEAD_L, 1.0, None),
        "lip_vjp_sqsum": lambda e: lib.lip_vjp_sqsum(e, None, None, 1, nv.HEAD_L, 1.0, None, 0, None),
        "lip_vjp_wnorm": lambda e: lib.lip_vjp_wnorm(e, None, None, None, 1, nv.HEAD_L, 1.0, None, 0, None),
        "lip_vjp_sqsum_scratch": lambda e: lib.lip_vjp_sqsum_scratch(e, 1, ctypes.byref(n)),
        "lip_vjp_wnorm_scratch": lambda e: lib.lip_vjp_wnorm_scratch(e, 1, ctypes.byref(n)),
    }
    h = ctypes.c_void_p()
    assert lib.lip_engine_create(ctypes.byref(h), 10, 2, 3) == 0
    try:
        for name, call in calls.items():
            for engine, status in ((None, LIP_ERR_ARG), (h, LIP_ERR_STATE)):
                assert call(engine) == status, (name, status)
                assert lib.lip_last_error().startswith(name.encode() + b":"), (name, lib.lip_last_error())
        assert n.value == -1
    finally:
        assert lib.lip_engine_destroy(h) == 0


def test_wnorm_census_is_a_table_of_its_own():
    lib = nv.load()
    n = lib.lip_debug_wnorm_route_count()
    counts, names = (ctypes.c_int64 * n)(), (ctypes.c_char_p * n)()
    assert lib.lip_debug_wnorm_routes(counts, n, names) == 0
    mine = {names[i].decode() for i in range(n)}
    assert len(mine) == n and all("wnorm" in r for r in mine)
    assert {"wgrad_wnorm_dense", "reduce_wnorm", "wnorm_finish"} <= mine
    assert sum(r.startswith("wgrad_wnorm<") for r in mine) == 6
    assert all(counts[i] == 0 for i in range(n))             # nothing has been launched on this machine
    assert lib.lip_debug_wnorm_routes(None, -1, None) == LIP_ERR_ARG
    # ... and none of them is a route of the conv / square-sum census
    m = lib.lip_debug_route_count()
    rn = (ctypes.c_char_p * m)()
    assert lib.lip_debug_routes(None, m, rn) == 0
    assert not ({rn[i].decode() for i in range(m)} & mine)


def test_probit_predictive_against_the_formula_in_float64():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(7, 5, dtype=torch.float64, generator=g) * 3
    v = torch.rand(7, 5, dtype=torch.float64, generator=g) * 10
    got = probit_predictive(f, v)
    for b in range(7):
        z = [f[b, k].item() / math.sqrt(1.0 + math.pi / 8.0 * v[b, k].item()) for k in range(5)]
        top = max(z)
        e = [math.exp(t - top) for t in z]
        for k in range(5):
            assert abs(got[b, k].item() - e[k] / sum(e)) <= 1e-14
    assert torch.allclose(got.sum(-1), torch.ones(7, dtype=torch.float64), atol=1e-14)
    # zero variance: the plain softmax; a large variance flattens the probabilities
    assert torch.allclose(probit_predictive(f, torch.zeros_like(v)), torch.softmax(f, -1), atol=1e-15)
    assert (probit_predictive(f, 1e6 * torch.ones_like(v)).max(-1).values < got.max(-1).values).all()
    # regressor: the mean, and the variance plus the observation noise
    m, s2 = probit_predictive(f[:, 0], v[:, 0], logvar=-0.3)
    assert torch.equal(m, f[:, 0])
    for b in range(7):
        assert abs(s2[b].item() - (v[b, 0].item() + math.exp(-0.3))) <= 1e-14


def test_polarisation_recovers_the_quadratic_form():
    g = torch.Generator().manual_seed(1)
    B, K, D = 3, 6, 40
    J = torch.randn(B, K, D, dtype=torch.float64, generator=g)
    w = torch.rand(D, dtype=torch.float64, generator=g) + 0.1
    ref = (J * w) @ J.transpose(-1, -2)                      # J diag(w) J^T
    E, ks, kps = polarisation_probes(K)
    assert E.shape == (K * (K + 1) // 2, K) and bool((ks <= kps).all())
    assert torch.equal(E.sum(-1), torch.full((E.shape[0],), 2.0))
    rows = torch.einsum("pk,bkd->bpd", E.double(), J)        # the rows of the probes e_k + e_k'
    q = (rows ** 2 * w).sum(-1)                              # their weighted square norms (B, P)
    S = covariance_from_polarisation(q, ks, kps, K)
    assert S.shape == (B, K, K) and S.dtype == torch.float64
    assert torch.equal(S, S.transpose(-1, -2))
    assert ((S - ref).abs().max() / ref.abs().max()).item() <= 1e-14
