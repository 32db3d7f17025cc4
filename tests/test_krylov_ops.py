"""GPU: every code path of the Krylov / trace primitives (csrc/lip_krylov.hip, lip_gemm_nt and lip_gemm_nn_axpy of
csrc/lip_mfma.hip), call by call against float64.

Each row of tests/krylov_cases.py is one call of a ``lip_*`` entry point through ``_native`` on operands placed by
tests/krylov_harness.py (bases 0..3 floats off a 16-byte boundary, strides, NaN canaries around and between), once with
exact integer inputs — the result must EQUAL the float64 reference — and once with random inputs, bounded per element on
Mag.  The census label of the call is asserted where the launcher chooses a kernel or a reduction mode.  The fills are
compared with a numpy Philox4x32-10, the refusals of the extern "C" wrappers are called one by one, and the coverage
test asserts that the table reaches every Krylov label except the two behind the LIP_DOT_NT_VALU switch, and that those
two are expected routes of tests/ab_switch_cases.py (run by tests/test_ab_switches.py in a child process).
"""
import numpy as np
import pytest
import torch

from lip_amd import _native as nv
from op_harness import CANARY, all_routes
import krylov_harness as kh
from krylov_cases import (CASES, FILL_CASES, FILL_NORMAL_STRIDE, KRYLOV_ROUTES, REFUSALS, VALU_ONLY, break_args)

pytestmark = pytest.mark.gpu

# The two constants that cannot be derived from the kernel text, measured on an MI355X over all cases of the primitive and
# set to 4 x the worst value (in units of 2^-24 * Mag):
#   scale_store: |Q - w / sqrt(nrm2)| over |w| / sqrt(nrm2) (rsqrtf as compiled for gfx950, then one product):
#   worst measured 2.045 (bound 4 x that); with nrm2 a power of four (exact inputs) every element was exact
K_SCALE_STORE = 8.18
#   fill_normal: |x - rad cos / sin| over rad = sqrt(-2 ln u1), float64 Box-Muller of the same Philox bits (__logf,
#   __fsqrt_rn, __sincosf): worst measured 8.359 over 33.6 M elements (bound 4 x that)
K_FILL_NORMAL = 33.44
MEASURE = False                      # True: print the figures, assert nothing that depends on the two constants


def _det_of_label(census):
    """dot_nt_f64 is repeatable whenever the partial tiles went through the scratch buffer, gemm_nt with one K-range"""
    (label,) = census.keys() or ("",)
    return label.endswith("/part") or label == "gemm_nt/ks1"


def run_case(case, exact, measure=False):
    lib = nv.load()
    call = kh.BUILDERS[case.prim](case.d, exact, seed=1 if exact else 2)
    if case.prim == "scale_store" and not exact:
        call.outs["Q"].k = K_SCALE_STORE
    m = measure and case.prim == "scale_store"
    census, stats = kh.run(lib, call, f"{case.name}[{'exact' if exact else 'random'}]", measure=m, det_of_label=_det_of_label)
    return census, stats


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_krylov_op(case, exact):
    census, stats = run_case(case, exact, MEASURE)
    for name, (worst, rms) in stats.items():
        print(f"STAT {case.name} {'exact' if exact else 'random'} {name}: worst {worst:.4g} of {case.prim}, rms/sqrt(L) {rms:.4g}")
    want = {case.route: 1} if case.route else {}
    assert census == want, f"{case.name}: expected the census {want}, the library counted {census}"


def test_table_reaches_every_krylov_route():
    lib = nv.load()
    every = set(all_routes(lib))
    assert KRYLOV_ROUTES <= every, sorted(KRYLOV_ROUTES - every)
    table = {c.route for c in CASES if c.route} | {"fill_normal", "fill_rademacher"}
    assert table <= KRYLOV_ROUTES
    missing = KRYLOV_ROUTES - table
    assert missing == VALU_ONLY, f"Krylov labels without a case: {sorted(missing - VALU_ONLY)}"
    from ab_switch_cases import ENTRIES
    switched = {route for e in ENTRIES for _, route in e.rows}
    assert VALU_ONLY <= switched, f"labels behind a switch without a row in ab_switch_cases.py: {sorted(VALU_ONLY - switched)}"
    assert not [r for r in every if r.split("/")[0].split("<")[0] in {"dot_nt", "rows_combine", "gemm_nt", "gemm_nn_axpy",
                                                                     "fill_normal", "fill_rademacher"} and r not in KRYLOV_ROUTES]


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("ref", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(ref):
    name, prim, d, how = ref
    lib = nv.load()
    if d is None:                                   # the fills: a null pointer / N = 0
        kh.routes(lib)
        buf = torch.zeros(64, device="cuda")
        rc = getattr(lib, "lip_" + prim)(0 if "null" in name else buf.data_ptr(), 2, 0 if "N0" in name else 8, 0, nv.stream_ptr())
        torch.cuda.synchronize()
        assert not buf.any()
        assert rc == kh.LIP_ERR_ARG and prim.encode() in lib.lip_last_error()
        assert kh.routes(lib) == {}
        return
    call = kh.BUILDERS[prim](d, False, seed=3)
    good = call.args
    call.args = lambda b: break_args(good(b), how)
    kh.run_refused(lib, call, name)


# ---------------------------------------------------------------------------------------------- the fills
def _fill(lib, prim, total, off, seed, P=1):
    """run a fill on a canary arena; returns the (total,) result after checking that nothing else was written"""
    words = torch.full((total + 2 * kh.GUARD + 4,), CANARY, dtype=torch.int32)
    dev = words.cuda()
    base = kh.GUARD + off
    kh.routes(lib)
    assert total % P == 0
    nv.check(getattr(lib, "lip_" + prim)(dev.data_ptr() + 4 * base, P, total // P, seed, nv.stream_ptr()), prim)
    torch.cuda.synchronize()
    assert kh.routes(lib) == {prim: 1}
    got = dev.cpu()
    keep = torch.ones(words.numel(), dtype=torch.bool)
    keep[base: base + total] = False
    assert torch.equal(got[keep], words[keep]), f"{prim}: total {total}, offset {off}: words outside the block changed"
    return got[base: base + total].view(torch.float32).numpy()


@pytest.mark.parametrize("total,off,seed", FILL_CASES)
def test_fill_rademacher_is_philox(total, off, seed):
    lib = nv.load()
    P = 3 if total % 3 == 0 else 1
    got = _fill(lib, "fill_rademacher", total, off, seed, P)
    kh.compare_rademacher(got, total, seed)
    again = _fill(lib, "fill_rademacher", total, off, seed, P)
    assert np.array_equal(got, again)


def _normal_error(got, total, seed):
    ref, rad = kh.ref_normal(total, seed)
    assert np.isfinite(got).all(), "elements not written or not finite"
    return np.abs(got.astype(np.float64) - ref) / (kh.U24 * rad + 1e-30)


@pytest.mark.parametrize("total,off,seed", FILL_CASES + [FILL_NORMAL_STRIDE])
def test_fill_normal_is_box_muller_of_philox(total, off, seed):
    lib = nv.load()
    got = _fill(lib, "fill_normal", total, off, seed)
    e = _normal_error(got, total, seed)
    i = int(np.argmax(e))
    print(f"STAT fill_normal total {total} off {off} seed {seed}: worst {e[i]:.4g} of fill_normal at {i}")
    assert MEASURE or e[i] <= K_FILL_NORMAL, f"element {i}: {e[i]:.4g} x 2^-24 rad from the float64 Box-Muller (> {K_FILL_NORMAL})"
    if total < 10 ** 6:
        assert np.array_equal(got.view(np.int32), _fill(lib, "fill_normal", total, off, seed).view(np.int32))
