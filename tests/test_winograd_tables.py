"""GPU: the geometry table of the Winograd conv kernel (igemm_wino_kernel), op by op against float64.

The kernel reads its staging-slot and tile decode from a per-geometry table that a helper kernel fills at the first
launch of the geometry on a stream.  The shapes are the smallest at which the table or the border tests against the
per-block scalars can go wrong; every op runs as in tests/test_kernel_routes.py (route census, every element against
the float64 emulator at the Winograd constants, canaries, a second run bit for bit where no float atomics take part).
"""
import pytest
import torch

from lip_amd import _native as nv
from kernel_route_cases import Case, conv
from op_harness import check, emulate
from test_kernel_routes import harness, restore_modes, run_case, set_modes, tolerances      # (K_WINO, RMS_WINO live there)

pytestmark = pytest.mark.gpu

VEPI, PLAIN = "igemm_wino/vepi", "igemm_wino"

CASES = [
    # NI = 2 with the second image absent; 3 of 4 tiles per row and column valid; NS = 200 of the 224 slots
    Case("tab_6x6_one_image", VEPI, conv(1, 6, 32, 32, 2)),
    # NI = 2 with an odd image count: the last of the two tile blocks half empty
    Case("tab_8x8_three_images", VEPI, conv(3, 8, 32, 32, 2)),
    # 7 tile blocks per image (odd), two column blocks, ragged tile rows
    Case("tab_28x28", VEPI, conv(1, 28, 32, 64, 2, epi={"res": "probe", "dphi": "shared"})),
    # two chunks x two segments, column sums by float atomics
    Case("tab_12x20_nseg2", VEPI, conv(2, 12, 64, 32, 3, W=20, nseg=2, epi={"red0": "", "red1": "", "xhat2": "shared"}), det=False),
    # the data-gradient form (flipped kernel) on a tall map, per-probe B
    Case("tab_24x8_t", VEPI, conv(2, 24, 64, 32, 2, W=8, mode=1, OH=24, OW=8, s=1, b_pp=True)),
    # the instantiation without 16-byte epilogue accesses
    Case("tab_8x8_misaligned_out", PLAIN, conv(1, 8, 32, 32, 2, out_shift=1)),
]
for _c in CASES:
    _c.tol = "wino"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_table_case(case):
    census, stats = run_case(case)
    print(case.name, stats)
    assert census == {case.route: 1}, f"{case.name}: expected the route {case.route}, the census shows {census}"


def test_first_use_on_two_streams():
    """a geometry no other test has (10 x 14 maps: block rectangle 4 x 8, ragged both ways) launched from two fresh streams
    in turn before either has synchronised — the first use of the geometry on both; each result must equal the
    single-stream one bit for bit and pass the float64 check"""
    case = Case("tab_two_streams", VEPI, conv(2, 10, 32, 32, 2, W=14, epi={"scale": "shared", "e0": "probe"}), tol="wino")
    h = harness()
    op, L, host, outs = h.build(case.spec, 3)
    P = case.spec.P
    prev = set_modes(h.lib, case)
    try:
        devs = [h.upload(host) for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        torch.cuda.synchronize()
        h.routes()
        for dev, st in zip(devs, streams):
            with torch.cuda.stream(st):
                nv.check(h.run_rc(op, dev, P), "lip_engine_run_op")
        torch.cuda.synchronize()
        census = h.routes()
        two = [h.download(dev) for dev in devs]
        dev = h.upload(host)
        h.run(op, dev, P)
        one = h.download(dev)
    finally:
        restore_modes(h.lib, prev)
    assert census == {case.route: 2}, census
    ref = emulate(h.eng.cn, h.chunk, op, host, P)
    mag = emulate(h.eng.cn, h.chunk, op, host, P, absolute=True)
    k_of, rms_c = tolerances(case)
    check(one, ref, mag, host, outs, k_of, rms_c, what=case.name)
    for i, got in enumerate(two):
        for k in one:
            assert torch.equal(got[k].view(torch.int32), one[k].view(torch.int32)), \
                f"stream {i}: space {k} differs from the single-stream result"
