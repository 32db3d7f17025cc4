"""The probe walk of the Winograd conv kernel (igemm_wino_kernel): a block handles W consecutive probes of its
(tile block, column block), W in {1, 2, 4} (lip_set_wino_walk; 0 = the automatic rule, lip_wino_walk_plan).

GPU: every shape below is run at P in {1, 3, 4, 5, 9} with the walk forced to 1, 2 and 4 — a full walk, short last
walks and P < W.  The forced walks are checked against the float64 emulator at the bounds of the Winograd class, bit by
bit against W = 1 (every output but the float-atomic column sums red0 / red1), for determinism, and probe by probe
against a one-probe launch on that probe's operands.  CPU: the automatic rule and the setter.

Each (shape, P) is laid out, emulated and run once; the tests share those runs.
"""
import copy

import pytest
import torch

from lip_amd import _native as nv
from kernel_route_cases import Case, conv
from op_harness import U24, TINY, check, emulate
from test_kernel_routes import K_WINO, RMS_WINO, harness, restore_modes, set_modes, tolerances

gpu = pytest.mark.gpu

WALK_K = 8                                   # WINO_WALK_K of csrc/lip_mfma.hip: blocks per resident slot the rule keeps
SLOTS_PER_CU = 3                             # resident blocks of the kernel per CU
RED = {"red0": "", "red1": "", "xhat2": "shared"}

# the smallest shapes that reach each path of the kernel: (name, route, spec at P probes, atomic-free)
SHAPES = {
    # single tile block, shared scale + per-probe e0
    "8x8": ("igemm_wino/vepi", lambda P: conv(1, 8, 32, 32, P, epi={"scale": "shared", "e0": "probe"}), True),
    # three images, the last image block half empty, two segments, per-probe column sums
    "12x12_nseg2_red": ("igemm_wino/vepi", lambda P: conv(3, 12, 32, 32, P, nseg=2, epi=RED), False),
    # two chunks per probe, per-probe weights: the tail request switches the B pointer to the next probe
    "24x24_t_bpp": ("igemm_wino/vepi", lambda P: conv(1, 24, 64, 32, P, mode=1, OH=24, s=1, b_pp=True), True),
    # misaligned output: the accumulator-layout epilogue
    "8x8_misaligned_out": ("igemm_wino", lambda P: conv(1, 8, 32, 32, P, out_shift=1, epi={"e1": "shared", "xhat": "shared"}), True),
    # per-probe activations
    "6x6_app": ("igemm_wino/vepi", lambda P: conv(1, 6, 32, 32, P, a_pp=True), True),
    # two column blocks, anisotropic, shared act' + per-probe residual
    "12x20_N64": ("igemm_wino/vepi", lambda P: conv(2, 12, 32, 64, P, W=20, epi={"dphi": "shared", "res": "probe"}), True),
    # anisotropic, ragged in both axes, two segments
    "6x28_nseg2_red": ("igemm_wino/vepi", lambda P: conv(3, 6, 32, 32, P, W=28, nseg=2, epi=RED), False),
}
PROBES = (1, 3, 4, 5, 9)
WALKS = (2, 4)

_RUNS = {}


def _case(shape, P):
    route, spec, det = SHAPES[shape]
    return Case(f"walk_{shape}_P{P}", route, spec(P), tol="wino", det=det)


def _launch(h, case, op, host, P, walk):
    """one run with the walk forced: (census, downloaded buffers)"""
    lib = h.lib
    prev = set_modes(lib, case)
    before = lib.lip_get_wino_walk()
    try:
        nv.check(lib.lip_set_wino_walk(walk), "lip_set_wino_walk")
        dev = h.upload(host)
        h.routes()                                   # clear
        h.run(op, dev, P)
        census = h.routes()
        return census, h.download(dev)
    finally:
        lib.lip_set_wino_walk(before)
        restore_modes(lib, prev)


def runs(shape, P):
    """the laid-out op of (shape, P), its float64 emulations and its runs at W = 1, 2, 4 (each twice)"""
    key = (shape, P)
    if key not in _RUNS:
        h = harness()
        case = _case(shape, P)
        op, L, host, outs = h.build(case.spec, seed=3)
        r = dict(case=case, op=op, host=host, outs=outs, got={}, again={}, census={})
        for w in (1,) + WALKS:
            r["census"][w], r["got"][w] = _launch(h, case, op, host, P, w)
            _, r["again"][w] = _launch(h, case, op, host, P, w)
        r["ref"] = emulate(h.eng.cn, h.chunk, op, host, P)
        r["mag"] = emulate(h.eng.cn, h.chunk, op, host, P, absolute=True)
        _RUNS[key] = r
    return _RUNS[key]


def _region(buf, base, count, ps, p):
    return buf[base + p * ps: base + p * ps + count]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


SHAPE_P = [(s, P) for s in SHAPES for P in PROBES]
SHAPE_P_IDS = [f"{s}-P{P}" for s, P in SHAPE_P]


@gpu
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("shape,P", SHAPE_P, ids=SHAPE_P_IDS)
def test_forced_walk_against_float64(shape, P, walk):
    """every output within the float64-emulator bounds of the Winograd class (K_WINO, RMS_WINO), canaries and inputs
    untouched, the route census unchanged"""
    r = runs(shape, P)
    case = r["case"]
    assert case.tol == "wino" and (K_WINO, RMS_WINO) == (16.0, 0.3)
    assert r["census"][walk] == {case.route: 1} == r["census"][1], (r["census"][walk], r["census"][1])
    k_of, rms_c = tolerances(case)
    stats = check(r["got"][walk], r["ref"], r["mag"], r["host"], r["outs"], k_of, rms_c, what=f"{case.name} W={walk}")
    print(f"{case.name} W={walk}: " + ", ".join(f"{n} max {a:.3g} rms {b:.3g}" for n, (a, b) in stats.items()))


@gpu
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("shape,P", SHAPE_P, ids=SHAPE_P_IDS)
def test_forced_walk_bit_identical_to_one_probe_per_block(shape, P, walk):
    """every output except red0 / red1 (float atomics) has the bits of the W = 1 launch; so has every other float"""
    r = runs(shape, P)
    one, got = r["got"][1], r["got"][walk]
    keep = {k: torch.ones(one[k].numel(), dtype=torch.bool) for k in one}
    for name, sp, base, count, ps, Pn, pre in r["outs"]:
        if name in ("red0", "red1"):
            for p in range(Pn):
                _region(keep[sp], base, count, ps, p).fill_(False)
    for k in one:
        a, b = one[k].view(torch.int32)[keep[k]], got[k].view(torch.int32)[keep[k]]
        ne = a != b
        assert not ne.any(), f"{r['case'].name} W={walk}: space {k}: {int(ne.sum())} floats differ from the W = 1 launch"


@gpu
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("shape,P", SHAPE_P, ids=SHAPE_P_IDS)
def test_forced_walk_is_deterministic(shape, P, walk):
    """a second run gives equal bits on the atomic-free outputs"""
    r = runs(shape, P)
    got, again = r["got"][walk], r["again"][walk]
    for name, sp, base, count, ps, Pn, pre in r["outs"]:
        if name in ("red0", "red1"):
            continue
        for p in range(Pn):
            assert _bits_equal(_region(got[sp], base, count, ps, p), _region(again[sp], base, count, ps, p)), \
                f"{r['case'].name} W={walk}: {name} of probe {p} differs between two runs"


def _one_probe_op(op, j):
    """the op of probe j alone: every per-probe operand and output moved to that probe's slice"""
    q = copy.deepcopy(op)
    refs = [getattr(q, f) for f in nv.REF_FIELDS]
    for s in range(q.nseg):
        refs += [q.seg[s].a, q.seg[s].b]
    for ref in refs:
        if ref.space != nv.SP_NONE and ref.pstride:
            ref.off += j * ref.pstride
    return q


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_probes_of_a_walk_are_isolated(shape):
    """P = 9, W = 4: probes 0 (first), 3 (last of a walk), 4 (first of the next walk) and 8 (a one-probe walk) equal,
    bit for bit, a one-probe launch on that probe's operands.  The column sums go through float atomics: both launches
    are within k 2^-24 Mag of the float64 sum, so they differ by at most twice that — a share of the previous probe's
    sums left in the block's buffer would be of the size of Mag itself."""
    P, walk = 9, 4
    r = runs(shape, P)
    h, case, got = harness(), r["case"], r["got"][walk]
    k_of, _ = tolerances(case)
    for j in (0, 3, 4, 8):
        _, single = _launch(h, case, _one_probe_op(r["op"], j), r["host"], 1, 0)
        for name, sp, base, count, ps, Pn, pre in r["outs"]:
            a, b = _region(got[sp], base, count, ps, j), _region(single[sp], base, count, ps, j)
            if name in ("red0", "red1"):
                mag = _region(r["mag"][sp], base, count, ps, j)
                err = ((a.double() - b.double()).abs() / (U24 * mag + TINY)).max().item()
                assert err <= 2 * k_of(name)[0], f"{case.name}: {name} of probe {j}: {err:.3g} x 2^-24 Mag from the one-probe launch"
            else:
                assert _bits_equal(a, b), f"{case.name}: {name} of probe {j} differs from the one-probe launch"


# ---------------------------------------------------------------------------------------------- the rule (no GPU)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_walk_plan():
    lib = nv.load()
    need = WALK_K * SLOTS_PER_CU * _cus()
    for gx in (1, 100, 200, 400):
        prev = 1
        for P in range(1, 600):
            w = lib.lip_wino_walk_plan(gx, P)
            assert w in (1, 2, 4), (gx, P, w)
            if P <= 8:
                assert w == 1, (gx, P, w)
            assert w >= prev, f"gx {gx}: the walk falls from {prev} to {w} at P = {P}"
            if w > 1:
                assert -(-P // w) * gx >= need, (gx, P, w)
            prev = w
    assert lib.lip_wino_walk_plan(400, 256) == 4            # the 32-channel stage of the headline step
    assert lib.lip_wino_walk_plan(1, 9) == 1


def test_walk_setter_round_trips():
    lib = nv.load()
    before = lib.lip_get_wino_walk()
    try:
        for w in (0, 1, 2, 4):
            assert lib.lip_set_wino_walk(w) == 0
            assert lib.lip_get_wino_walk() == w
        for bad in (-1, 3, 5, 8):
            assert lib.lip_set_wino_walk(bad) != 0
            assert lib.lip_get_wino_walk() == 4
    finally:
        lib.lip_set_wino_walk(before)
    assert lib.lip_get_wino_walk() == before
