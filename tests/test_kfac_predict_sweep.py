"""GPU checks of the row-free Kronecker-factored predictive: the ``EWNORM`` sweep (``lip_vjp_eigen_wnorm``,
``LinearizedNet.kfac_predict_sweep``) and the public surface (``route="sweep"``) on the nets of tests/kfac_ref.py with
one and three test points, and ResNet-50 with K = 1000.

The nets are the smallest bindings that reach every branch of the sweep: Dense layers (OH OW = 1: the bilinear route),
SAME 3x3, stride 2 with unequal padding, 1x1, the 7x7 stem, row counts Mt that are no multiple of 4, blocks with and
without a bias row, BN-scaled blocks (whose BN scale and bias are the remainder) and a flat head.

The operands come from the float32 passes, so no bound is derivable: every bound is 4 x the worst error measured on
MI355X, as max|got - want| / max|want| over a net's outputs, with the measured figures next to it (the convention of
tests/test_ekfac_sweep.py), and never above SWEEP_CAP = 1e-5 of the maximum, the bound tests/test_ggn_diag.py holds the
sweeps to.  The float64 helper (``tests/kfac_predict_sweep_ref.py``) works in the product's own fitted (V, R, Ub).
"""
import ctypes
import functools

import pytest
import torch

import kfac_predict_sweep_ref as pr
import kfac_ref as kf
from lip_amd import _native as nv
from lip_amd import kfac
from lip_amd.engine import LinearizedNet
from lip_amd.evaluate import eval_dataset_probit
from lip_amd.ggn import clear_engine_cache, get_engine
from lip_amd.lla import predict_lla_ekfac, predict_lla_kfac
from lip_amd.scalemodels import ResNet50
from lip_amd.toymodels import create_state
from test_ekfac import _helper, _rel
from test_ekfac_sweep import CANARY, _canaries_intact, _guarded, _householder

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
DEV = "cuda"
N_FULL = kf.N_FULL
NETS = list(dict.fromkeys(kf.NETS + ["stem_net"]))
POINTS = (1, 3)
SWEEP_CAP = 1e-5


@pytest.fixture(autouse=True)
def _fresh_cache():
    yield
    clear_engine_cache()


def _census(lib, wnorm=False):
    """{route: launches} since the last read of ``lip_debug_routes`` (``wnorm``: of ``lip_debug_wnorm_routes``)"""
    n = lib.lip_debug_wnorm_route_count() if wnorm else lib.lip_debug_route_count()
    counts, names = (ctypes.c_int64 * n)(), (ctypes.c_char_p * n)()
    nv.check((lib.lip_debug_wnorm_routes if wnorm else lib.lip_debug_routes)(counts, n, names), "census")
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


def _prior(h, grouped):
    return kf.split_prior(h["state"], h["alpha"]) if grouped else h["alpha"]


def _fit(h, grouped):
    """(triples, (rem_idx, rem_var)) of ``posterior_lla_kfac``'s fit, on the device"""
    _, fits, rem_idx, rem_var, _ = kfac._cached_fit(h["state"], h["Z"], h["model_type"], _prior(h, grouped), N_FULL, None)
    return [f[:3] for f in fits], (rem_idx, rem_var)


@functools.lru_cache(maxsize=None)
def _reference(name, grouped):
    """(3, K, K) float64 CPU: the helper's predictive of the first three new points under the product's own fit; built
    once per net and prior and never written to (a point's predictive does not depend on the other points bound)"""
    h = _helper(name)
    triples, (rem_idx, rem_var) = _fit(h, grouped)
    cpu = [tuple(t.cpu() for t in f) for f in triples]
    return pr.predict_ref(h["state"], h["Xnew"][:3], cpu, h["J_new"][:3], rem_idx.cpu(), rem_var.cpu())


def _diag(cov):
    return torch.diagonal(cov, dim1=1, dim2=2)


# measured on MI355X, worst of n = 1 and n = 3 and of the scalar and the two-group prior, max|. - ref| / max|ref|:
# diag=True against the float64 helper / against the rows route, diag=False against the helper / against the rows route,
# and the diagonal of diag=False against diag=True:
#   sine_regressor 1.89e-7 / 8.03e-8, 1.89e-7 / 8.03e-8, 0   xor_classifier 1.82e-7 / 9.46e-8, 3.05e-7 / 2.54e-7, 0
#   mlp_ragged     1.02e-7 / 1.01e-7, 1.69e-7 / 1.68e-7, 0   resnet_tiny    1.44e-7 / 1.42e-7, 2.41e-7 / 2.24e-7, 0
#   resnet50_tiny  1.55e-7 / 1.90e-7, 2.66e-7 / 3.11e-7, 0   flat_head      1.66e-7 / 1.83e-7, 1.66e-7 / 2.47e-7, 0
#   stem_net       1.49e-7 / 1.46e-7, 1.56e-7 / 1.57e-7, 0
# (the probe e_k + e_k is 2 e_k, whose norm is 4 times that of e_k exactly, so the diagonal of the polarised form is the
# diag form bitwise; it is held to the diag bound all the same).  Every bound is below SWEEP_CAP.
DIAG_TOL = 7.6e-7              # 4 x 1.89e-7
DIAG_ROWS_TOL = 7.6e-7         # 4 x 1.90e-7
FULL_TOL = 1.3e-6              # 4 x 3.05e-7 (polarisation cancels)
FULL_ROWS_TOL = 1.3e-6         # 4 x 3.11e-7
assert max(DIAG_TOL, DIAG_ROWS_TOL, FULL_TOL, FULL_ROWS_TOL) <= SWEEP_CAP


@pytest.mark.parametrize("grouped", [False, True], ids=["scalar", "grouped"])
@pytest.mark.parametrize("name", NETS)
def test_sweep_matches_the_float64_helper_and_the_rows_route(name, grouped):
    h = _helper(name)
    state, model_type = h["state"], h["model_type"]
    want3 = _reference(name, grouped)
    triples, rem = _fit(h, grouped)
    K = want3.shape[1]
    worst = [0.0] * 5
    for n in POINTS:
        want = want3[:n]
        top = want.abs().max().item()
        eng = get_engine(state, h["Xnew"][:n], model_type)
        var = eng.kfac_predict_sweep(triples, rem)                                           # diag=True is the default
        rows = eng.kfac_predict(triples, rem, diag=True)
        assert var.shape == (n, K) and var.dtype == F64 and var.is_cuda and float(var.min()) >= 0.0
        full = eng.kfac_predict_sweep(triples, rem, diag=False)
        rows_full = eng.kfac_predict(triples, rem, diag=False)
        assert full.shape == (n, K, K) and full.dtype == F64 and torch.equal(full, full.transpose(1, 2))
        errs = [(var.cpu() - _diag(want)).abs().max().item() / top, (var - rows).abs().max().item() / top,
                (full.cpu() - want).abs().max().item() / top, (full - rows_full).abs().max().item() / top,
                (_diag(full) - var).abs().max().item() / top]
        worst = [max(a, b) for a, b in zip(worst, errs)]
        assert torch.equal(var, eng.kfac_predict_sweep(triples, rem, diag=True))             # bitwise reproducible
    print(f"{name} {'grouped' if grouped else 'scalar'}: diag against the helper {worst[0]:.2e} / the rows route {worst[1]:.2e}  "
          f"full against the helper {worst[2]:.2e} / the rows route {worst[3]:.2e}  diagonal of full against diag {worst[4]:.2e}")
    assert worst[0] <= DIAG_TOL and worst[1] <= DIAG_ROWS_TOL and worst[2] <= FULL_TOL and worst[3] <= FULL_ROWS_TOL
    assert worst[4] <= DIAG_TOL


# measured on MI355X, max|. - ref| / max|ref| against eng.vjp_wnorm(E, w, "raw"), worst of n = 1 and n = 3:
#   sine_regressor 1.09e-7  xor_classifier 1.12e-7  mlp_ragged 1.74e-7  resnet_tiny 3.01e-8  resnet50_tiny 2.64e-8
#   flat_head 6.96e-8  stem_net 8.69e-8
IDENTITY_TOL = DIAG_TOL        # held to the bound of the sweep against the helper


@pytest.mark.parametrize("name", NETS)
def test_identity_bases_give_the_weighted_norm_sweep(name):
    """V = I, Ub = I, R_l the block's slice of a positive (D,) vector w and the remainder's variances w itself: the sum
    is sum_d w_d (J_i^T e_k)_d^2, what ``lip_vjp_wnorm`` forms from the unprojected operands"""
    h = _helper(name)
    state, model_type = h["state"], h["model_type"]
    worst = 0.0
    for n in POINTS:
        eng = get_engine(state, h["Xnew"][:n], model_type)
        blocks, K = eng.kfac_blocks(), eng.K
        w = (torch.rand(eng.D, generator=torch.Generator().manual_seed(23), dtype=F64) + 0.5).to(DEV)
        triples = [(torch.eye(b.Mt, device=DEV, dtype=F64), w[b.off:b.off + b.Mt * b.N].reshape(b.Mt, b.N).contiguous(),
                    torch.eye(b.N, device=DEV, dtype=F64)) for b in blocks]
        rem_idx = kfac.remainder_indices(blocks, eng.D).to(DEV)
        got = eng.kfac_predict_sweep(triples, (rem_idx, w[rem_idx]))
        E = torch.eye(K, device=DEV, dtype=F32)[:, None, :].expand(K, n, K).contiguous()
        want = eng.vjp_wnorm(E, w.float(), "raw").T.double()
        worst = max(worst, _rel(got, want))
    print(f"{name}: identity bases against vjp_wnorm {worst:.2e}")
    assert worst <= IDENTITY_TOL


# The class blocks of a chunked call are sweeps of their own, and a binding with fewer probes per pass runs more passes.
# Unlike the pair-summed second moments of tests/test_ekfac_sweep.py, nothing here is summed across pairs: every
# (probe, example) pair has its own projected rows, its own tile sums and its own output float, formed in an order that
# does not depend on which other probes share the pass.  Measured on MI355X, max|. - unsplit| / max|unsplit|, for
# class_chunk = 1 / about K / 2 / an engine of two probes per pass: 0 / 0 / 0 on all seven nets (bitwise equal), so the
# 4 x rule gives 0 and the test asks for equality.
SPLIT_TOL = 0.0                # 4 x 0


@pytest.mark.parametrize("name", NETS)
def test_probe_chunks_agree_with_the_unsplit_sweep(name):
    h = _helper(name)
    state, model_type = h["state"], h["model_type"]
    triples, rem = _fit(h, False)
    eng = get_engine(state, h["Xnew"][:3], model_type)
    K = eng.K
    whole = eng.kfac_predict_sweep(triples, rem)
    one = eng.kfac_predict_sweep(triples, rem, class_chunk=1)
    half = eng.kfac_predict_sweep(triples, rem, class_chunk=max(1, K // 2))
    assert torch.equal(whole, eng.kfac_predict_sweep(triples, rem))                          # bitwise reproducible
    assert torch.equal(one, eng.kfac_predict_sweep(triples, rem, class_chunk=1))
    # the engine's own passes: the same binding with at most two probes per pass writes disjoint slices of one output
    small = LinearizedNet(state, h["Xnew"][:3], model_type, workspace_bytes=1 << 28, max_chunk=2)
    passes = small.kfac_predict_sweep(triples, rem)
    assert torch.equal(passes, small.kfac_predict_sweep(triples, rem))
    e = [_rel(one, whole), _rel(half, whole), _rel(passes, whole)]
    print(f"{name}: class_chunk=1 {e[0]:.2e}  class_chunk={max(1, K // 2)} {e[1]:.2e}  two probes per pass {e[2]:.2e}")
    assert max(e) <= SPLIT_TOL
    with pytest.raises(ValueError, match="class_chunk must be positive"):
        eng.kfac_predict_sweep(triples, rem, class_chunk=0)


# measured on MI355X, max|sweep - rows| / max|rows| of the public predictives, KFAC diag / full, EKFAC with its default
# fit (moments="rows") diag / full, EKFAC with moments="sweep" diag / full:
#   resnet_tiny    1.42e-7 / 2.24e-7, 1.78e-7 / 3.55e-7, 1.79e-7 / 3.54e-7
#   xor_classifier 7.35e-8 / 2.40e-7, 1.03e-7 / 1.45e-7, 4.54e-8 / 1.47e-7
#   sine_regressor 2.72e-8 / 2.72e-8, 6.12e-8 / 6.12e-8, 4.50e-8 / 4.50e-8
SURFACE_TOL = 1.5e-6           # 4 x 3.55e-7


@pytest.mark.parametrize("name", ["resnet_tiny", "xor_classifier", "sine_regressor"])
def test_public_predictives_on_the_sweep_route(name):
    h = _helper(name)
    state, Z, model_type, alpha, X = h["state"], h["Z"], h["model_type"], h["alpha"], h["Xnew"]
    K = h["f_new"].shape[1]
    errs = []
    # the route is independent of the fit: EKFAC with its default moments (the rows fit) and with the sweep's
    for predict, kw in ((predict_lla_kfac, {}), (predict_lla_ekfac, {}), (predict_lla_ekfac, {"moments": "sweep"})):
        for cov in ("diag", "full"):
            a = predict(state, X, Z, model_type, alpha, full_set_size=N_FULL, cov=cov, batch=3, route="sweep", **kw)
            b = predict(state, X, Z, model_type, alpha, full_set_size=N_FULL, cov=cov, batch=3, route="rows", **kw)
            if cov == "diag":
                assert a[0].shape == b[0].shape == ((5,) if model_type == "regressor" else (5, K)) and a[1].shape == b[1].shape
                assert a[1].dtype == F64 and a[0].dtype == F64
                errs.append(_rel(a[1], b[1]))
            else:
                assert type(a) is type(b) and a.covariance().shape == b.covariance().shape
                assert a.covariance().shape == ((5, 5) if model_type == "regressor" else (5, K, K))
                assert a.mean().shape == b.mean().shape
                assert torch.equal(a.covariance(), a.covariance().transpose(-1, -2))
                errs.append(_rel(a.covariance(), b.covariance()))
    print(f"{name}: sweep against rows  KFAC diag {errs[0]:.2e} full {errs[1]:.2e}  EKFAC diag {errs[2]:.2e} full {errs[3]:.2e}  "
          f"EKFAC (moments='sweep') diag {errs[4]:.2e} full {errs[5]:.2e}")
    assert max(errs) <= SURFACE_TOL


def test_eval_dataset_probit_on_the_sweep_route_fits_once_and_asks_for_no_rows(monkeypatch):
    h = _helper("xor_classifier")
    state, Z, model_type, alpha = h["state"], h["Z"], h["model_type"], h["alpha"]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(16, 2, dtype=F64, generator=g)
    y = torch.randint(0, 2, (16,), generator=g)
    data = [(X[:8], y[:8]), (X[8:], y[8:])]
    want = eval_dataset_probit(state, data, Z, alpha, N_FULL, model_type, posterior="kfac", route="rows")
    clear_engine_cache()
    calls = []
    inner = kfac._fit
    monkeypatch.setattr(kfac, "_fit", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])

    def refuse(*a, **kw):
        raise AssertionError("a D-wide row block was asked for")
    monkeypatch.setattr(LinearizedNet, "vjp_rows", refuse)
    got = eval_dataset_probit(state, data, Z, alpha, N_FULL, model_type, posterior="kfac", route="sweep")
    assert len(calls) == 1                                          # one fit for both batches
    for a, b in zip(got[:4], want[:4]):
        assert abs(a - b) <= 1e-6
    assert got[4].shape == (16, 2) and float((got[4] - want[4]).abs().max()) <= 1e-6 and torch.equal(got[5], want[5])
    with pytest.raises(ValueError, match="route"):
        eval_dataset_probit(state, data, Z, alpha, N_FULL, model_type, posterior="diag", route="sweep")


def _block_order(eng):
    lib, C = eng.lib, ctypes
    cap = len(eng.kfac_blocks())
    koff, ooff, Ns = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
    count, total = C.c_int32(0), C.c_int64(0)
    assert lib.lip_vjp_kron_layout(eng.h, cap, koff, ooff, Ns, C.byref(count), C.byref(total)) == 0 and count.value == cap
    return {int(koff[i]): i for i in range(cap)}


def test_sweep_refusals_leave_the_output_untouched():
    """``lip_vjp_eigen_wnorm`` checks every op before its first launch: every refused call returns 1 and writes nothing"""
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    lib, C = eng.lib, ctypes
    blocks = eng.kfac_blocks()
    cap, K, n = len(blocks), eng.K, eng.n
    order = _block_order(eng)
    Vs = [torch.eye(b.Mt, device=DEV, dtype=F64) for b in blocks]
    Us = [torch.eye(b.N, device=DEV, dtype=F64) for b in blocks]
    Rs = [torch.ones(b.Mt, b.N, device=DEV, dtype=F32) for b in blocks]

    def arrays():
        Vp, Up, Rp, Mts = (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_int32 * cap)()
        for b, V, Ub, R in zip(blocks, Vs, Us, Rs):
            k = order[b.kernel_off]
            Vp[k], Up[k], Rp[k], Mts[k] = V.data_ptr(), Ub.data_ptr(), R.data_ptr(), b.Mt
        return Vp, Up, Rp, Mts

    E = torch.eye(K, device=DEV, dtype=F32)[:, None, :].expand(K, n, K).contiguous()
    floats = C.c_int64(0)
    assert lib.lip_vjp_eigen_wnorm_scratch(eng.h, K, C.byref(floats)) == 0 and floats.value > 0
    assert lib.lip_vjp_eigen_wnorm_scratch(eng.h, 0, C.byref(floats)) == 1
    assert lib.lip_vjp_eigen_wnorm_scratch(eng.h, K, None) == 1 and lib.lip_vjp_eigen_wnorm_scratch(None, K, C.byref(floats)) == 1
    scratch = torch.empty(floats.value + 4, device=DEV, dtype=F32)
    w_rem = torch.zeros(eng.D, device=DEV, dtype=F32)
    buf, out = _guarded(K * n)
    Vp, Up, Rp, Mts = arrays()
    good = [eng.h, E.data_ptr(), Vp, Up, Rp, Mts, cap, w_rem.data_ptr(), out.data_ptr(), K, nv.HEAD_IN, 1.0, scratch.data_ptr(),
            floats.value, nv.stream_ptr()]
    # null arguments; a block count that is not the tape's; no probes; a head mode of the forward sweeps; a scratch that
    # is missing, one float short, or not 16-byte aligned
    for i, v in [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, cap - 1), (6, cap + 1), (6, 0), (8, None),
                 (9, 0), (10, nv.HEAD_LT), (12, None), (13, floats.value - 1), (13, 0), (12, scratch.data_ptr() + 4)]:
        args = list(good)
        args[i] = v
        assert lib.lip_vjp_eigen_wnorm(*args) == 1, (i, v)
    for which in range(4):                          # a null block operand; a row count that is not the op's KH KW C (+ 1)
        bad = list(arrays())
        if which < 3:
            bad[which][cap - 1] = None
        else:
            bad[3][0] += 2
        args = list(good)
        args[2:6] = bad
        assert lib.lip_vjp_eigen_wnorm(*args) == 1, which
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    out.zero_()
    assert lib.lip_vjp_eigen_wnorm(*good) == 0
    no_rem = list(good)
    no_rem[7] = None                                # no weight vector: no reduction runs; w_rem = 0 gives the same bitwise
    buf2, out2 = _guarded(K * n)
    out2.zero_()
    no_rem[8] = out2.data_ptr()
    assert lib.lip_vjp_eigen_wnorm(*no_rem) == 0
    torch.cuda.synchronize()
    assert bool((out > 0).all()) and torch.equal(out, out2) and _canaries_intact(buf) and _canaries_intact(buf2)
    once = out.clone()
    assert lib.lip_vjp_eigen_wnorm(*good) == 0     # the call adds: the same sums again, one float32 rounding per op
    torch.cuda.synchronize()
    assert _rel(out, 2.0 * once.double()) <= 8 * 2.0 ** -24


def _wide_head_engine(classes):
    """a Dense head of ``classes`` outputs on a 4-channel 3 x 3 conv: the smallest binding with more than 32 outputs"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((4, 4, 3))
    net.dense(net.conv(0, "Conv_0", 4, 3, act="relu", use_bias=True), "Dense_0", classes)
    state = create_state(net, 1, dtype=F32)
    Z = torch.rand(2, 4, 4, 3, generator=torch.Generator().manual_seed(2))
    return LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 28, max_chunk=8)


def test_engine_method_checks_its_operands():
    lib = nv.load()
    h = _helper("flat_head")
    eng = get_engine(h["state"], h["Z"], h["model_type"])
    blocks = eng.kfac_blocks()
    triples = [(torch.eye(b.Mt, device=DEV, dtype=F64), torch.ones(b.Mt, b.N, device=DEV, dtype=F64),
                torch.eye(b.N, device=DEV, dtype=F64)) for b in blocks]
    rem = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=F64))
    wide = _wide_head_engine(33)
    wt = [(torch.eye(b.Mt, device=DEV, dtype=F64), torch.ones(b.Mt, b.N, device=DEV, dtype=F64),
           torch.eye(b.N, device=DEV, dtype=F64)) for b in wide.kfac_blocks()]
    torch.cuda.synchronize()
    _census(lib), _census(lib, wnorm=True)                                                   # reading clears the counts
    (V0, R0, U0), t1 = triples
    for bad in ([triples[0]], [(V0.float(), R0, U0), t1], [(V0, R0.T, U0), t1], [(V0, R0, U0.cpu()), t1],
                [(V0, R0[:-1].contiguous(), U0), t1]):
        with pytest.raises(ValueError, match="layer blocks need|contiguous float64 device matrix"):
            eng.kfac_predict_sweep(bad, rem)
    with pytest.raises(ValueError, match="probes must be"):
        eng.kfac_predict_sweep(triples, rem, probes=torch.zeros(2, eng.n + 1, eng.K))
    with pytest.raises(ValueError, match="one variance per index"):
        eng.kfac_predict_sweep(triples, (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=F64)))
    with pytest.raises(ValueError, match="K = 33"):
        wide.kfac_predict_sweep(wt, rem, diag=False)
    assert not _census(lib) and not _census(lib, wnorm=True)                                 # every refusal came before a launch
    assert wide.kfac_predict_sweep(wt, rem, diag=True).shape == (2, 33)                      # the diag form has no such limit


def test_census_shows_known_labels_only():
    lib = nv.load()
    h = _helper("resnet_tiny")
    triples, rem = _fit(h, False)
    eng = get_engine(h["state"], h["Xnew"][:3], h["model_type"])
    assert eng.chunk >= eng.K                                                                # one pass
    torch.cuda.synchronize()
    known = lib.lip_debug_route_count()
    _census(lib), _census(lib, wnorm=True)                                                   # reading clears the counts
    eng.kfac_predict_sweep(triples, rem)
    torch.cuda.synchronize()
    routes, wn = _census(lib), _census(lib, wnorm=True)
    assert lib.lip_debug_route_count() == known                                             # no new route name appeared
    assert not any(name.startswith(("wgrad", "reduce")) for name in routes), routes          # no parameter cotangent is formed
    n = lib.lip_debug_wnorm_route_count()
    names = (ctypes.c_char_p * n)()
    nv.check(lib.lip_debug_wnorm_routes(None, n, names), "lip_debug_wnorm_routes")
    labels = {names[i].decode() for i in range(n)}
    blocks = eng.kfac_blocks()
    assert set(wn) <= labels and wn["wgrad_wnorm_dense"] == sum(b.T == 1 for b in blocks)
    assert sum(c for name, c in wn.items() if name.startswith("wgrad_wnorm")) == len(blocks)
    assert rem[0].numel() > 0 and wn["reduce_wnorm"] > 0 and wn["wnorm_finish"] == len(blocks) + wn["reduce_wnorm"]
    print(f"resnet_tiny: routes of one sweep {sorted(routes)}; wnorm census {wn}")


# measured on MI355X (ResNet-50, K = 1000, 64 x 64, two images, eight one-hot probes, 54 blocks), max|. - ref| / max|ref|
# against r0 * vjp_wnorm(probes, None, "raw"):
#   8.54e-7 (the bases of the largest blocks are 4608 x 4608 reflectors: the projections add float32 roundings of
#   their own, which the unprojected sweep does not have)
R50_TOL = 3.5e-6               # 4 x 8.54e-7, below SWEEP_CAP


def test_resnet50_k1000_without_rows(monkeypatch):
    """Householder reflectors as orthonormal bases and every R_l and remainder variance equal to r0: the Frobenius norm
    is invariant, sum R T^2 = r0 ||mat_l(J^T u)||_F^2, so the result is r0 times the unweighted norm sweep"""
    def refuse(*a, **kw):
        raise AssertionError("a D-wide row block was asked for")
    monkeypatch.setattr(LinearizedNet, "vjp_rows", refuse)
    net = ResNet50(1000, input_shape=(64, 64, 3))
    state = create_state(net, 5, dtype=F64)
    Z = torch.rand(2, 64, 64, 3, generator=torch.Generator().manual_seed(6), dtype=F64)
    eng = get_engine(state, Z, "classifier")
    blocks = eng.kfac_blocks()
    assert len(blocks) == 54 and eng.K == 1000
    g = torch.Generator().manual_seed(8)
    r0 = 0.37
    triples = [(_householder(b.Mt, g), torch.full((b.Mt, b.N), r0, device=DEV, dtype=F64), _householder(b.N, g)) for b in blocks]
    rem_idx = kfac.remainder_indices(blocks, eng.D).to(DEV)
    rem = (rem_idx, torch.full((rem_idx.numel(),), r0, device=DEV, dtype=F64))
    classes = torch.randperm(1000, generator=g)[:8]
    probes = torch.zeros(8, 2, 1000, dtype=F32)
    probes[torch.arange(8), :, classes] = 1.0
    got = eng.kfac_predict_sweep(triples, rem, probes=probes)
    want = r0 * eng.vjp_wnorm(probes.to(DEV), None, "raw").double()
    assert got.shape == (8, 2) and got.dtype == F32 and bool(torch.isfinite(got).all()) and float(got.min()) > 0.0
    e = _rel(got, want)
    print(f"resnet50 K=1000 predictive sweep, 8 probes, {len(blocks)} blocks, D = {eng.D}: against r0 x vjp_wnorm {e:.2e}")
    assert e <= R50_TOL
