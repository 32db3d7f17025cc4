"""GPU: the mean-pool kernels with pixel groups side by side on the quad path, and reduce_kernel's 512-row blocks, against
float64 (tests/test_small_ops.run_case: census label, bound on Mag, RMS, canaries, accumulation prefill, and a second
run whose `out` must be bitwise equal — pool_fwd adds its groups' partial sums in a fixed order).

C = 128 and 64 take the fixed-channel path (256 % C == 0) and C = 12 the quad path with 3 quads x 85 pixel groups;
C = 40 (10 quads x 25 groups) and C = 512 (128 quads x 2 groups) are quad rows with several pixels per group, HW = 49
leaves the groups unequal and is no multiple of pool_bwd's 16-pixel blocks.  A misaligned base keeps the paths it had.
Bounds: those of tests/small_op_cases.py (they count float32 roundings and hold for any summation order).
"""
import pytest

from small_op_cases import pool_bwd, pool_fwd, reduce
from test_small_ops import run_case

pytestmark = pytest.mark.gpu


def _path(C, aligned=True):
    if 256 % C == 0:
        return "fixed"
    return "quad" if C % 4 == 0 and aligned else "atomic"


def _cases():
    cs = []
    for C in (128, 64, 12, 40, 512):
        for HW in (64, 49):
            cs.append(pool_fwd(f"pf_C{C}_HW{HW}", f"pool_fwd/{_path(C)}", C, HW, 3))
            cs.append(pool_bwd(f"pb_C{C}_HW{HW}", f"pool_bwd/{_path(C)}", C, HW, 3, dphi=True, red0=True, red1=True, mask=True))
            cs.append(pool_bwd(f"pb_C{C}_HW{HW}_plain", f"pool_bwd/{_path(C)}", C, HW, 3))
    for C in (128, 12, 40):
        cs.append(pool_fwd(f"pf_C{C}_shift", f"pool_fwd/{_path(C, False)}", C, 49, 3, shift=1))
        cs.append(pool_bwd(f"pb_C{C}_outshift", f"pool_bwd/{_path(C, False)}", C, 49, 3, dphi=True, red0=True, red1=True, shift=1))
    # reduce_kernel: 33 x 64 blocks of 512 rows, the last of one row; and the same rows as 128-row blocks at 16 probes
    cs.append(reduce("red_N4_R16385_P64_rpb512", "reduce/quad", 4, 16385, 64, red1=True))
    cs.append(reduce("red_N12_R16385_P16_rpb128", "reduce/quad", 12, 16385, 16, red1=True))
    cs.append(reduce("red_N128_R1100", "reduce/quad", 128, 1100, 3, red1=True))
    cs.append(reduce("red_N64_R1100_gshift", "reduce/fixed", 64, 1100, 3, red1=True, shift=1))
    return cs


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_path(case):
    census, stats = run_case(case)
    print(f"{case.name}: {stats}")
    assert census == {case.route: 1}, f"{case.name}: expected {case.route}, the census shows {census}"
