"""GPU: every code path of the non-GEMM engine kernels (csrc/lip_small.hip), op by op against float64.

Each row of tests/small_op_cases.py is one synthetic op run through lip_engine_run_op.  The test asserts that the route
census of that call is exactly the expected label, then checks every output element against the float64 emulator
(tests/op_harness.py: bound on Mag or bitwise, RMS, NaN canaries, accumulation prefill, determinism).  The coverage
test asserts that the table reaches every small-op label the library lists; the per-example forms (lip_vjp_rows,
lip_vjp_sqsum), which lip_engine_run_op cannot reach, run through two small nets.
"""
import math

import pytest
import torch

from lip_amd import _native as nv
from op_harness import U24, TINY, Harness, check, all_routes
from small_op_cases import CASES, ROWS_ROUTES, SMALL_ROUTES
from small_op_harness import FLT_MIN, build_small, region
from test_kernel_routes import K_SQ, _bind, _census, _per_tensor

pytestmark = pytest.mark.gpu

# error constants, in units of 2^-24 * Mag (Mag: small_op_harness.MagMachine), measured on an MI355X over the table and
# set to 4 x the worst:
#   tanh (a and 1 - a^2): worst measured 1.66, RMS 0.43; GELU (a and its derivative): worst measured 2.03, RMS 0.57;
#   softmax (p and sqrt p, Mag = value x (1 + |f - max f|)): worst measured 3.06 (K = 1000, logits x 30), RMS 0.57
K_MEASURED = {"tanh": 6.65, "gelu": 8.12, "softmax": 12.25}
#   RMS of the normalised error of the sums (REDUCE, the pools and their red0 / red1, HEAD) over sqrt(reduction length):
#   worst measured 0.38 (HEAD, K = 2); bound 1.52.  (The worst element of any sum was 0.36 of its bound: the 2 x 3 window
#   average's cotangent on the 6 x 16 map, an_mpb_avg_C64_6x16; 0.29 on the square maps.)
RMS_SUM = 1.52
#   ReLU: the derivative is not compared where |y| <= 8 * 2^-24 * Mag_y (y may round to the other side of 0); at most
#   1e-4 of a case's elements and never more than 16
RELU_SKIP_SHARE, RELU_SKIP_MAX = 1e-4, 16

_H = None
LIP_ERR_ARG = 1


def harness():
    global _H
    if _H is None:
        _H = Harness(max_chunk=256)
    return _H


def k_of_case(case, measure=False):
    def k_of(name):
        t = case.tol[name]
        if isinstance(t, str):
            k = 1e30 if measure else K_MEASURED[t]
            return k, 1, k
        k, kref = t
        return (k, kref, RMS_SUM if kref > 1 else k) if not measure else (k, kref, 1e30)
    return k_of


def relu_skip_mask(h, case, op, host, outs, mag):
    """elements whose pre-activation lies within its own rounding of 0 (from the float64 reference alone)"""
    import copy
    op0 = copy.copy(op)
    op0.act = 0
    y = h.emulate(op0, host, 1)
    o = next(t for t in outs if t[0] == "out")
    yr, my = region(y[o[1]], o).reshape(-1), region(mag[o[1]], o).reshape(-1)
    skip = yr.abs() <= 8 * U24 * my
    n = int(skip.sum())
    assert n <= RELU_SKIP_MAX and n <= RELU_SKIP_SHARE * skip.numel(), \
        f"{case.name}: {n} of {skip.numel()} pre-activations within rounding of 0: choose another seed"
    return {"out2": skip}


def run_case(case, seed=0, measure=False):
    """run one case; returns (census of the first run, stats {output: (max err, rms / sqrt(K))})."""
    h = harness()
    spec = case.spec
    op, L, host, outs = build_small(h, spec, seed)
    P = spec.P
    dev = h.upload(host)
    h.routes()                                   # clear
    if case.refuse:
        rc = h.run_rc(op, dev, P, spec.head_mode, spec.head_c)
        torch.cuda.synchronize()
        assert rc == LIP_ERR_ARG, f"{case.name}: lip_engine_run_op returned {rc}, expected LIP_ERR_ARG"
        got = h.download(dev)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), host[k].view(torch.int32)), f"{case.name}: a refused op wrote to space {k}"
        return h.routes(), {}
    h.run(op, dev, P, spec.head_mode, spec.head_c)
    census = h.routes()
    got = h.download(dev)
    dev = h.upload(host)
    h.run(op, dev, P, spec.head_mode, spec.head_c)
    again = h.download(dev)
    ref = h.emulate(op, host, P, head_mode=spec.head_mode, head_c=spec.head_c)
    exact = {n for n, t in case.tol.items() if t == "exact"}
    if exact == set(case.tol) and not case.relu_skip:
        mag = ref                                 # every output bitwise: no Mag needed
    else:
        mag = h.emulate(op, host, P, absolute=True, head_mode=spec.head_mode, head_c=spec.head_c)
    skip = relu_skip_mask(h, case, op, host, outs, mag) if case.relu_skip else None
    floor = {"out": FLT_MIN, "out2": math.sqrt(FLT_MIN)} if spec.kind == nv.OP_SOFTMAX else None
    stats = check(got, ref, mag, host, outs, k_of_case(case, measure), 1.0, what=case.name, exact=exact, skip=skip, floor=floor)
    # a second run: every `out` tensor bitwise, everything when no float atomics feed an output
    for name, sp, base, count, ps, Pn, pre in outs:
        if case.det or name not in ("red0", "red1"):
            a, b = region(got[sp], (base, count, ps, Pn)), region(again[sp], (base, count, ps, Pn))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{case.name}: {name} differs in a second run"
    if case.extra:
        EXTRA[case.extra](case, host, outs, got, ref, mag, stats, measure)
    return census, stats


def _out(outs, name):
    return next(t for t in outs if t[0] == name)


def extra_softmax(case, host, outs, got, ref, mag, stats, measure):
    """sum_k p_k = 1 and sqrtp^2 = p to the bound of the elements"""
    n, K = case.spec.n_img, case.spec.N
    k = 1e30 if measure else K_MEASURED["softmax"]
    o, o2 = _out(outs, "out"), _out(outs, "out2")
    p, s = region(got[o[1]], o).double().reshape(n, K), region(got[o2[1]], o2).double().reshape(n, K)
    mp, ms = region(mag[o[1]], o).reshape(n, K), region(mag[o2[1]], o2).reshape(n, K)
    e1 = (p.sum(-1) - 1).abs() / (U24 * mp.sum(-1) + K * FLT_MIN)
    e2 = ((s * s - p).abs() - FLT_MIN - 2 * s * math.sqrt(FLT_MIN)).clamp_min(0) / (U24 * (mp + 2 * s * ms) + TINY)
    stats["sum_p"] = (e1.max().item(), 0.0)
    stats["sqrtp_sq"] = (e2.max().item(), 0.0)
    assert e1.max() <= k, f"{case.name}: |sum p - 1| is {e1.max().item():.3g} x the bound unit (> {k})"
    assert e2.max() <= k, f"{case.name}: |sqrtp^2 - p| is {e2.max().item():.3g} x the bound unit (> {k})"


def extra_softmax_shift(case, host, outs, got, ref, mag, stats, measure):
    """row 1 = row 0 + 1e4 exactly: its probabilities must match the reference of row 0 to the bound"""
    extra_softmax(case, host, outs, got, ref, mag, stats, measure)
    K = case.spec.N
    k = 1e30 if measure else K_MEASURED["softmax"]
    for name, fl in (("out", FLT_MIN), ("out2", math.sqrt(FLT_MIN))):
        o = _out(outs, name)
        y, r, m = region(got[o[1]], o).double().reshape(2, K), region(ref[o[1]], o).reshape(2, K), region(mag[o[1]], o).reshape(2, K)
        e = ((y[1] - r[0]).abs() - fl).clamp_min(0) / (U24 * m[0] + TINY)
        stats["shift_" + name] = (e.max().item(), 0.0)
        assert e.max() <= k, f"{case.name}: {name} of the row offset by 1e4 is {e.max().item():.3g} units from the plain row's reference"


def extra_relu_zeros(case, host, outs, got, ref, mag, stats, measure):
    """z = 0 exactly, no bias / BatchNorm: a = 0 and dphi = 0 exactly"""
    a_in = case.spec.refs["a"]
    o, o2 = _out(outs, "out"), _out(outs, "out2")
    a, d = region(got[o[1]], o).reshape(-1), region(got[o2[1]], o2).reshape(-1)
    z = region(ref[o[1]], o).reshape(-1)           # relu(z): 0 where z <= 0
    zero = torch.nonzero(z == 0).flatten()
    assert zero.numel() > a_in.count // 4
    assert (a[zero] == 0).all() and (d[zero] == 0).all(), f"{case.name}: a or dphi not exactly 0 where z <= 0"


EXTRA = {"softmax": extra_softmax, "softmax_shift": extra_softmax_shift, "relu_zeros": extra_relu_zeros}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_small_op(case):
    census, stats = run_case(case)
    for name, (worst, rms) in stats.items():
        print(f"{case.name}: {name}: worst {worst:.4g}, rms/sqrt(K) {rms:.4g}")
    want = {} if case.refuse else {case.route: 1}
    assert census == want, f"{case.name}: expected the census {want}, the library counted {census}"


def test_table_reaches_every_small_route():
    lib = nv.load()
    every = set(all_routes(lib))
    small = {r for r in every if r.split("/")[0] in {"reduce", "pool_fwd", "pool_bwd", "maxpool_primal", "maxpool_fwd",
                                                      "maxpool_bwd", "primal_post", "softmax", "head"}}
    table = {c.route for c in CASES if c.route}
    assert len(small) >= 35, sorted(small)
    missing = small - table - ROWS_ROUTES
    assert not missing, f"small-op labels without a case in small_op_cases.py: {sorted(missing)}"
    assert table <= small, sorted(table - small)
    assert SMALL_ROUTES == table | ROWS_ROUTES and ROWS_ROUTES <= small


# ---------------------------------------------------------------------------------------------- per-example forms
def _net_bn_maxpool():
    """BatchNorm (red1 live) and a 3 x 3 / 2 max pool at 64 channels"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((12, 12, 3))
    x = net.conv(0, "Conv_0", 64, 3, 1, padding=1, bn="BatchNorm_0", act="relu")
    x = net.maxpool(x, 3, 2, padding=1)                                      # 12 x 12 -> 6 x 6
    x = net.conv(x, "Conv_1", 24, 3, 1, padding=1, bn="BatchNorm_1", act="relu")
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 5)
    net.model_type = "classifier"
    return net


def _net_lenet():
    """LeNet style: 2 x 2 average pools and a mean pool at a channel count that is not a multiple of 4"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((16, 16, 1))
    x = net.conv(0, "Conv_0", 6, 5, 1, padding=2, act="tanh", use_bias=True)
    x = net.avgpool(x, 2, 2)
    x = net.conv(x, "Conv_1", 10, 3, 1, padding=1, act="tanh", use_bias=True)
    x = net.avgpool(x, 2, 2)
    x = net.meanpool(x)
    x = net.dense(x, "Dense_0", 12, act="tanh")
    net.dense(x, "Dense_1", 5)
    net.model_type = "classifier"
    return net


@pytest.mark.parametrize("which", ["bn_maxpool", "lenet"])
def test_rows_and_sqsum(which):
    """lip_vjp_rows (rows_reduce and the per-example form of reduce_kernel) and lip_vjp_sqsum (reduce_sqsum) per parameter
    tensor against the emulator's per-example rows in float64"""
    net = _net_bn_maxpool() if which == "bn_maxpool" else _net_lenet()
    n, P = 3, 2
    eng, tm, slices = _bind(net, n, 9, P)
    U = torch.randn(P, n, eng.K, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    rows = torch.zeros(P, n, eng.D, dtype=torch.float64)
    for i in range(n):
        Ui = torch.zeros_like(U)
        Ui[:, i] = U[:, i]
        rows[:, i] = tm.vjp(Ui, nv.HEAD_L, 0.7)
    lib = eng.lib
    all_routes(lib)                                  # clear the census
    r = eng.vjp_rows(U, "l", 0.7)
    torch.cuda.synchronize()
    census = set(_census(lib))
    _per_tensor(r, rows.reshape(P * n, -1), slices, 2e-5, f"rows net {which}")
    assert "reduce/rows" in census, f"net {which}: the per-example reduce did not run (census {sorted(census)})"
    ref = (rows ** 2).sum((0, 1))
    y0 = (torch.rand(eng.D, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * ref).float().cuda()
    got = eng.vjp_sqsum(U, "l", 0.7, out=y0.clone())
    torch.cuda.synchronize()
    census = set(_census(lib))
    want = y0.double().cpu() + ref
    _per_tensor(got, want[None], slices, 1e-5, f"sqsum net {which}")
    err = (got.double().cpu() - want).abs()
    unit = torch.zeros_like(want)
    sabs = rows.abs().sum((0, 1))
    for name, a, b in slices:
        unit[a:b] = 2.0 ** -24 * sabs[a:b] * rows[:, :, a:b].abs().max()
    worst = ((err - 2.0 ** -24 * 4 * want).clamp_min(0) / unit.clamp_min(1e-300)).max().item()
    assert (err <= K_SQ * unit + 2.0 ** -24 * 4 * want + 1e-30).all(), \
        f"sqsum net {which}: worst error {worst:.3g} x 2^-24 sum|r| max|r| > {K_SQ}"
    assert "reduce_sqsum" in census, f"net {which}: reduce_sqsum did not run (census {sorted(census)})"
