"""GPU: every launch route of the conv GEMM dispatchers (launch_igemm, launch_wgrad), op by op against float64.

Each row of tests/kernel_route_cases.py is one synthetic IGEMM / WGRAD op run through lip_engine_run_op.  The test
asserts that the route census of that call is exactly the expected route, then checks every output element against
the float64 emulator (tests/op_harness.py: bound on Mag, RMS, canaries, accumulation, determinism).  The coverage
test asserts that the table reaches every route the library lists except the A/B-only ones below, and that each of
those is an expected route of tests/ab_switch_cases.py (run by tests/test_ab_switches.py in child processes).
"""
import pytest
import torch

from lip_amd import _native as nv
from kernel_route_cases import CASES
from op_harness import Harness, check, emulate, all_routes
from small_op_cases import SMALL_ROUTES      # labels of the non-GEMM kernels: tests/test_small_ops.py reaches each of them
from krylov_cases import KRYLOV_ROUTES       # labels of the Krylov primitives: tests/test_krylov_ops.py reaches each of them

pytestmark = pytest.mark.gpu

MI355X_CUS = 256

# routes reachable only through an A/B environment switch (read once per process: tests/test_ab_switches.py runs each of
# them in a child process of its own, from the table tests/ab_switch_cases.py)
AB_ONLY = {
    "igemm_fast<4,1,1,2>", "igemm_fast<4,1,1,2>/bv4",      # LIP_NOADIRECT: the 128-row f32 tiles take igemm_adirect
    "igemm_fast<4,1,1,1>", "igemm_fast<4,1,1,1>/bv4",      # (same switch)
    "wgrad_pb<3,1,1,4>",                                   # LIP_WGRAD3: the three-wave 96-row tile in f32 mode
}
# routes of the per-example square-sum path (lip_vjp_sqsum), reached by the nets of test_sqsum_and_rows_routes below
SQSUM_NETS = {"a": {"wgrad_sqsum<2,2,1,2>", "wgrad_sqsum<4,1,1,2>", "wgrad_sqsum<2,2,2,2>", "wgrad_sqsum<4,1,1,1>",
                    "wgrad_sqsum_dense", "reduce_sqsum"},
              "b": {"wgrad_sqsum<4,1,1,1>", "wgrad_sqsum<2,2,1,1>", "wgrad_sqsum<2,1,1,1>", "wgrad_sqsum_dense",
                    "reduce_sqsum"},
              # non-square inputs (aniso_nets.per_example_nets): between them every tile and the dense form
              "c": {"wgrad_sqsum<2,2,1,2>", "wgrad_sqsum<4,1,1,2>", "wgrad_sqsum<2,2,2,2>", "wgrad_sqsum<4,1,1,1>",
                    "wgrad_sqsum_dense", "reduce_sqsum"},
              "d": {"wgrad_sqsum<2,2,1,1>", "wgrad_sqsum<4,1,1,1>", "wgrad_sqsum<2,1,1,1>", "wgrad_sqsum_dense",
                    "reduce_sqsum"}}
SQSUM_ROUTES = set().union(*SQSUM_NETS.values())

# error constants, in units of 2^-24 * Mag (Mag: the emulator's result on |every operand|); "RMS" is the RMS of the
# normalised error over an output divided by sqrt(K), K the reduction length (Ktot; WGRAD: R; red0 / red1: + R)
#   exact f32 routes: worst case Ktot + 16 for any summation order (worst measured 0.10 (Ktot + 16)); RMS measured 0.24
#   (the anisotropic rows: 0.094 (Ktot + 16) and 0.13)
RMS_EXACT = 1.0
#   Winograd F(2x2, 3x3): the transforms add and subtract up to 16 input and weight terms in f32: worst measured 4.04
#   (an_wg_wino_8x12; 3.9 on the square maps); bound 16.  RMS measured 0.075; bound 0.3
K_WINO, RMS_WINO = 16.0, 0.3
#   bf16x3 split precision (~1e-5 relative per product): worst measured 219 (stride-2 data gradients, square and
#   non-square alike), 141 on an (even, odd) output without the parity-class order, 86 elsewhere; bound 1024.  RMS
#   measured 2.1 (an_wg_4111_x3); bound 8
K_X3, RMS_X3 = 1024.0, 8.0
#   square sums (lip_vjp_sqsum): per element, in units of 2^-24 sum_{p,i} |r_pij| max_tensor |r| (r: the per-example
#   rows): worst measured 4.2; bound 16
K_SQ = 16.0

_H = None


def harness():
    global _H
    if _H is None:
        _H = Harness(max_chunk=256)
    return _H


def _ktot(spec):
    return spec.R if spec.kind == nv.OP_WGRAD else sum(s.Ktot for s in spec.segs)


def tolerances(case):
    """k_of(output name) -> (worst-case k, RMS reference length), and the RMS constant of the route class."""
    spec = case.spec
    kt = _ktot(spec)

    def k_of(name):
        kk = kt + (spec.R if name in ("red0", "red1") else 0)
        if case.tol == "wino":
            return K_WINO * (1 + (spec.R if name in ("red0", "red1") else 0) / 16), kk
        if case.tol == "x3":
            return K_X3 * (1 + (spec.R if name in ("red0", "red1") else 0) / 16), kk
        return kk + 16, kk

    rms_c = {"exact": RMS_EXACT, "wino": RMS_WINO, "x3": RMS_X3}[case.tol]
    return k_of, rms_c


def set_modes(lib, case):
    prev = (lib.lip_get_precision(), lib.lip_get_winograd())
    nv.check(lib.lip_set_precision(case.prec), "lip_set_precision")
    nv.check(lib.lip_set_winograd(case.wino), "lip_set_winograd")
    nv.check(lib.lip_set_split_k(case.split_k), "lip_set_split_k")
    return prev


def restore_modes(lib, prev):
    lib.lip_set_precision(prev[0])
    lib.lip_set_winograd(prev[1])
    lib.lip_set_split_k(1)


def run_case(case, seed=0, shared=None):
    """run one case; returns (census of the first run, stats {output: (max err, rms / sqrt(K))}).  shared: a dict that
    keeps the laid-out op, its host buffers and the two float64 emulations for the next run of the same case."""
    h = harness()
    shared = {} if shared is None else shared
    if not shared:
        op, L, host, outs = h.build(case.spec, seed)
        shared.update(op=op, host=host, outs=outs)
    op, host, outs = shared["op"], shared["host"], shared["outs"]
    P = case.spec.P
    prev = set_modes(h.lib, case)
    try:
        dev = h.upload(host)
        h.routes()                                   # clear
        h.run(op, dev, P)
        census = h.routes()
        got = h.download(dev)
        if case.det:
            dev = h.upload(host)
            h.run(op, dev, P)
            again = h.download(dev)
    finally:
        restore_modes(h.lib, prev)
    if "ref" not in shared:
        shared["ref"] = emulate(h.eng.cn, h.chunk, op, host, P)
        shared["mag"] = emulate(h.eng.cn, h.chunk, op, host, P, absolute=True)
    k_of, rms_c = tolerances(case)
    stats = check(got, shared["ref"], shared["mag"], host, outs, k_of, rms_c, what=case.name)
    if case.det:
        for k in got:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), \
                f"{case.name}: a second run differs in space {k} (route without float atomics)"
    return census, stats


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_route(case):
    census, _ = run_case(case)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if case.cu and cus != MI355X_CUS:
        pytest.skip(f"route of {case.name} assumes {MI355X_CUS} CUs, this device has {cus} (numbers checked)")
    assert census == {case.route: 1}, f"{case.name}: expected the route {case.route}, the census shows {census}"


# One stream's float scratch serves the split-K planes, the transformed Winograd weights and the transformed Winograd
# activations in turn (stream_scratch of lip_mfma.hip).  The harness launches on torch's current stream, so the sequence
# runs on the default stream and then on a second one, which gets a scratch record and geometry tables of its own.
# Floats needed: 18 816 (3 planes), 16 384, 32 768 (grows), 40 960 (grows), then two smaller needs of the grown buffer.
SCRATCH_SEQUENCE = ["ks_2211_bv4", "wino_8x8", "wino_12x12", "wg_wino_12", "ks_2211_bv4", "wino_8x8"]


def test_users_of_one_streams_scratch_back_to_back():
    by_name = {c.name: c for c in CASES}
    shared = {name: {} for name in SCRATCH_SEQUENCE}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    harness()
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for step, name in enumerate(SCRATCH_SEQUENCE):
                case = by_name[name]
                census, _ = run_case(case, shared=shared[name])          # (its own row's bounds, determinism included)
                if not case.cu or cus == MI355X_CUS:
                    assert census == {case.route: 1}, f"step {step} ({name}): expected {case.route}, the census shows {census}"
        torch.cuda.synchronize()


def test_table_reaches_every_route():
    lib = nv.load()
    every = set(all_routes(lib))
    table = {c.route for c in CASES}
    assert AB_ONLY <= every and SQSUM_ROUTES <= every and SMALL_ROUTES <= every and KRYLOV_ROUTES <= every
    assert {r for r in every if "sqsum" in r} == SQSUM_ROUTES
    assert not (table & AB_ONLY), sorted(table & AB_ONLY)
    from ab_switch_cases import ENTRIES
    switched = {route for e in ENTRIES for _, route in e.rows}
    assert AB_ONLY <= switched, f"A/B-only routes without a row in ab_switch_cases.py: {sorted(AB_ONLY - switched)}"
    missing = every - AB_ONLY - SQSUM_ROUTES - SMALL_ROUTES - KRYLOV_ROUTES - table
    assert not missing, f"routes without a case in kernel_route_cases.py: {sorted(missing)}"
    assert table <= every, sorted(table - every)


# ---------------------------------------------------------------------------------------------- paths run_op cannot reach
def _net_a():
    """square-sum tiles <2,2,1,2>, <4,1,1,2>, <2,2,2,2>, <4,1,1,1>, the dense square sum and the bias reduce"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((6, 6, 3))
    x = net.conv(0, "Conv_0", 72, 3, 1, padding=1, act="relu", use_bias=True)       # M = 27, N = 72
    x = net.conv(x, "Conv_1", 40, 3, 1, padding=1, act="relu")                      # M = 648, N = 40
    x = net.conv(x, "Conv_2", 80, 3, 1, padding=1, act="relu")                      # M = 360, N = 80
    x = net.conv(x, "Conv_3", 20, 3, 1, padding=1, act="relu")                      # M = 720, N = 20
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 5)
    net.model_type = "classifier"
    return net


def _net_b():
    """square-sum tiles <2,2,1,1>, <2,1,1,1>; in lip_ggn_vp the fused-overwrite weight gradients of the 3 x 3 layer
    (Winograd, one split) and of the last dense layer (skinny)"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((8, 8, 32))
    x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, act="relu", use_bias=True)       # M = 288, N = 32
    x = net.conv(x, "Conv_1", 48, 1, 1, padding=0, act="relu")                      # M = 32, N = 48
    x = net.conv(x, "Conv_2", 16, 1, 1, padding=0, act="relu")                      # M = 48, N = 16
    x = net.meanpool(x)
    x = net.dense(x, "Dense_0", 40, act="relu")
    net.dense(x, "Dense_1", 5)                                                       # M = 40, R = n
    net.model_type = "classifier"
    return net


def _net_c():
    """lip_ggn_vp on a 3 x 3 layer whose Winograd weight gradient splits (float atomics into the initialised block)"""
    from lip_amd.netspec import NetSpec
    net = NetSpec((32, 32, 32))
    x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, act="relu")
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 3)
    net.model_type = "classifier"
    return net


def _census(lib):
    import ctypes as C
    n = lib.lip_debug_route_count()
    counts, names = (C.c_int64 * n)(), (C.c_char_p * n)()
    nv.check(lib.lip_debug_routes(counts, n, names), "lip_debug_routes")
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


def _tensor_slices(params):
    from lip_amd.utils import _walk, nn_param_tree
    out, o = [], 0
    for name, leaf in _walk(nn_param_tree(params)):
        n = torch.as_tensor(leaf).numel()
        out.append((name, o, o + n))
        o += n
    return out


def _per_tensor(got, ref, slices, tol, what):
    """max |got - ref| over each parameter tensor, scaled by that tensor's max |ref|"""
    got = got.double().cpu().reshape(-1, ref.shape[-1])
    ref = ref.reshape(-1, ref.shape[-1])
    for name, a, b in slices:
        s = ref[:, a:b].abs().max().item()
        err = (got[:, a:b] - ref[:, a:b]).abs().max().item()
        assert err <= tol * s + 1e-30, f"{what}: parameter tensor {name}: max err {err:.3e} > {tol} x {s:.3e}"


def _bind(net, n, seed, P):
    from lip_amd.engine import LinearizedNet, build_consts
    from lip_amd.toymodels import create_state
    from lip_amd.utils import flatten_nn_params
    from tape_emulator import TapeMachine
    state = create_state(net, seed, dtype=torch.float64)
    Z = torch.rand(n, *net.tensors[0], dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    eng = LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 28, max_chunk=P)
    flat, _ = flatten_nn_params(state.params)
    tm = TapeMachine(eng.cn, flat, build_consts(eng.cn, state.params, state.batch_stats, "cpu", torch.float64), Z, chunk=eng.chunk)
    tm.primal()
    return eng, tm, _tensor_slices(state.params)


def _net_of(which):
    if which in ("c", "d"):
        from aniso_nets import per_example_nets
        return per_example_nets()[which]
    return _net_a() if which == "a" else _net_b()


def test_every_sqsum_route_runs_on_a_non_square_map():
    assert SQSUM_NETS["c"] | SQSUM_NETS["d"] == SQSUM_ROUTES
    for which in ("c", "d"):
        net = _net_of(which)
        assert all(net.tensors[u.src][0] != net.tensors[u.src][1] for u in net.units if u.kind == "conv" and u.kh > 1)


def _emulator_rows(tm, U):
    """the float64 per-example rows (P, n, D) of the tape emulator, one example at a time"""
    P, n = U.shape[:2]
    rows = torch.zeros(P, n, tm.cn.D, dtype=torch.float64)
    for i in range(n):
        Ui = torch.zeros_like(U)
        Ui[:, i] = U[:, i]
        rows[:, i] = tm.vjp(Ui, nv.HEAD_L, 0.7)
    return rows


def _check_sqsum(eng, U, rows, slices, what):
    """lip_vjp_sqsum ADDED to a pre-filled buffer, element by element against the float64 squares of `rows`, and a
    second run bitwise equal"""
    ref = (rows ** 2).sum((0, 1))
    y0 = (torch.rand(eng.D, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * ref).float().cuda()
    got = eng.vjp_sqsum(U, "l", 0.7, out=y0.clone())  # the square sum is ADDED to y0
    torch.cuda.synchronize()
    want = y0.double().cpu() + ref
    _per_tensor(got, want[None], slices, 1e-5, what)
    # element by element: a row element r with error e <= k 2^-24 max|r| (its tensor's rows) moves r^2 by ~2 |r| e, so
    # |y_j - want_j| <= 2^-24 (K_SQ sum_{p,i} |r_pij| max_t|r| + 4 want_j)
    err = (got.double().cpu() - want).abs()
    unit = torch.zeros_like(want)
    sabs = rows.abs().sum((0, 1))
    for name, a, b in slices:
        unit[a:b] = 2.0 ** -24 * sabs[a:b] * rows[:, :, a:b].abs().max()
    worst = ((err - 2.0 ** -24 * 4 * want).clamp_min(0) / unit.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error {worst:.3g} x 2^-24 sum|r| max|r|")
    assert (err <= K_SQ * unit + 2.0 ** -24 * 4 * want + 1e-30).all(), \
        f"{what}: worst error {worst:.3g} x 2^-24 sum|r| max|r| > {K_SQ}"
    again = eng.vjp_sqsum(U, "l", 0.7, out=y0.clone())
    assert torch.equal(again, got), "lip_vjp_sqsum is not bitwise reproducible"


@pytest.mark.parametrize("which", ["a", "b", "c", "d"])
def test_sqsum_and_rows_routes(which):
    """lip_vjp_sqsum element by element against float64 squares of the emulator's per-example rows, lip_vjp_rows
    against those rows; the census shows the square-sum routes."""
    net = _net_of(which)
    n, P = 3, 2
    eng, tm, slices = _bind(net, n, 7, P)
    U = torch.randn(P, n, eng.K, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    rows = _emulator_rows(tm, U)
    lib = eng.lib
    all_routes(lib)                                  # clear the census
    _check_sqsum(eng, U, rows, slices, f"sqsum net {which}")
    census = set(_census(lib))
    r = eng.vjp_rows(U, "l", 0.7)
    _per_tensor(r, rows.reshape(P * n, -1), slices, 2e-5, f"rows net {which}")
    want = SQSUM_NETS[which]
    assert want <= census, f"net {which}: square-sum routes {sorted(want - census)} not taken (census {sorted(census)})"


# ---- several pairs per block: the in-block loop over (probe, example) pairs of the per-pair kernels ----------------
# At n = 3, P = 2 every group of the nets above holds ONE pair.  47 probes of 11 examples are 517 pairs: with the grouping
# rule of lip_internal.h every grouped launch of nets a and b then walks 2, 4 or 7 pairs per block and ends on a short
# group (blocks per group 1: per 2, G 259, last 1; 3: per 4, G 130, last 1; 6: per 7, G 74, last 6).
MANY_P, MANY_N = 47, 11
SQ_TARGET_BLOCKS = 512                              # lip_internal.h


def _pair_groups(blocks, pairs):
    """pair_groups of lip_internal.h: (per, G)"""
    g = max(1, min(pairs, -(-SQ_TARGET_BLOCKS // blocks)))
    per = -(-pairs // g)
    return per, -(-pairs // per)


def _grouped_launches(net):
    """(label, blocks per group) of every grouped launch of the per-pair kernels on `net`: the weight-gradient tile
    of each conv with more than one output pixel (with_wgrad_tile of lip_mfma.hip) and the bias reduces (sq_cb of
    lip_small.hip)"""
    for u in net.units:
        if u.kind != "conv":
            continue
        name = u.kernel[-2]
        M, N = u.kh * u.kw * u.cin, u.cout
        oh, ow, _ = net.tensors[u.dst]
        if oh * ow > 1:
            bm, bn = (64 if M <= 64 else 128), (128 if N > 64 else 64 if N > 32 else 32)
            yield f"{name} wgrad", -(-M // bm) * -(-N // bn)
        if u.bias is not None:
            cb = 64
            while cb > 1 and cb // 2 >= N:
                cb //= 2
            yield f"{name} bias", -(-N // cb)


def assert_several_pairs_per_group(net, pairs):
    launches = list(_grouped_launches(net))
    assert any(l.endswith("wgrad") for l, _ in launches) and any(l.endswith("bias") for l, _ in launches)
    for label, blocks in launches:
        per, G = _pair_groups(blocks, pairs)
        assert per >= 2 and pairs % per != 0 and G > 1, f"{label}: {blocks} blocks per group, per {per}, G {G}"


_MANY = {}


def many_pairs(which):
    """(engine, parameter slices, U, float64 emulator rows) of net `which` at 517 pairs; computed once, shared with
    tests/test_wnorm.py.  The emulator runs a tape compiled for ONE example on each example in turn (nothing in these
    nets couples the examples), which costs 1 / n of walking the n-example tape n times."""
    if which not in _MANY:
        from lip_amd.engine import LinearizedNet, build_consts, compile_net
        from lip_amd.toymodels import create_state
        from lip_amd.utils import flatten_nn_params
        from tape_emulator import TapeMachine
        net, P, n = _net_of(which), MANY_P, MANY_N
        state = create_state(net, 7, dtype=torch.float64)
        Z = torch.rand(n, *net.tensors[0], dtype=torch.float64, generator=torch.Generator().manual_seed(7))
        eng = LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 28, max_chunk=P)
        assert eng.chunk == P, eng.chunk                # one pass: every launch sees all 517 pairs
        U = torch.randn(P, n, eng.K, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        cn1 = compile_net(net, 1, state.params)
        flat, _ = flatten_nn_params(state.params)
        consts = build_consts(cn1, state.params, state.batch_stats, "cpu", torch.float64)
        rows = torch.zeros(P, n, eng.D, dtype=torch.float64)
        for i in range(n):
            tm = TapeMachine(cn1, flat, consts, Z[i:i + 1], chunk=P)
            tm.primal()
            rows[:, i] = tm.vjp(U[:, i:i + 1].contiguous(), nv.HEAD_L, 0.7)
        slices = _tensor_slices(state.params)
        # the reference is usable: finite, and every parameter tensor gets a non-zero row from every pair
        assert bool(rows.isfinite().all())
        for name, a, b in slices:
            assert bool((rows[:, :, a:b].abs().amax(-1) > 0).all()), f"{name}: a pair with an all-zero reference row"
        _MANY[which] = (eng, slices, U, rows)
    return _MANY[which]


@pytest.mark.parametrize("which", ["a", "b"])
def test_sqsum_several_pairs_per_group_last_group_short(which):
    """every tile, the dense form and the reduce with 2, 4 or 7 pairs per block and a short last group, element by
    element against float64 squares of the emulator's per-example rows"""
    assert_several_pairs_per_group(_net_of(which), MANY_P * MANY_N)
    eng, slices, U, rows = many_pairs(which)
    all_routes(eng.lib)                              # clear the census
    _check_sqsum(eng, U, rows, slices, f"sqsum net {which}, {MANY_P * MANY_N} pairs")
    census = set(_census(eng.lib))
    assert SQSUM_NETS[which] <= census, sorted(SQSUM_NETS[which] - census)


def test_sqsum_single_group_adds_into_y():
    """P = 1, n = 1 on net b: one pair, G = 1 — the kernels add into the pre-filled y directly, no finish kernel"""
    eng, tm, slices = _bind(_net_b(), 1, 7, 1)
    U = torch.randn(1, 1, eng.K, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    rows = _emulator_rows(tm, U)
    all_routes(eng.lib)                              # clear the census
    _check_sqsum(eng, U, rows, slices, "sqsum net b, one pair")
    census = set(_census(eng.lib))
    assert SQSUM_NETS["b"] <= census, sorted(SQSUM_NETS["b"] - census)


@pytest.mark.parametrize("which", ["b", "c"])
def test_ggn_vp_fused_overwrite(which):
    """lip_ggn_vp with alpha != 0: the weight gradients that WRITE y = s acc + alpha v (skinny, Winograd with one split)
    and the Winograd gradient with several splits that adds into the alpha v block, per parameter tensor vs float64"""
    net = _net_b() if which == "b" else _net_c()
    n, P = (3, 2) if which == "b" else (4, 2)
    eng, tm, slices = _bind(net, n, 11, P)
    V = torch.randn(P, eng.D, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    all_routes(eng.lib)
    Y = eng.ggn_vp(V, 1.7, 0.37)
    torch.cuda.synchronize()
    census = _census(eng.lib)
    ref = tm.ggn_vp(V, 1.7, 0.37)
    _per_tensor(Y, ref, slices, 2e-5, f"ggn_vp net {which}")
    want = {"b": {"wgrad_wino/rowq", "wgrad_skinny<2,8>"}, "c": {"wgrad_wino/rowq"}}[which]
    assert want <= set(census), f"net {which}: routes {sorted(want - set(census))} not taken (census {census})"
