"""The cases of tests/test_wgrad_wino_stage.py and tests/test_wgrad_wino_stage_cpu.py: WGRAD ops that land on
wgrad_wino/rowq, whose cotangent the block stages once through LDS (wgrad_wino_kernel<true, true> of csrc/lip_mfma.hip).

A stage is two groups of 8 tiles; the launcher pads the groups per share (gps) to an even number.  The shapes are the
smallest at which the stage map can go wrong.
"""
from kernel_route_cases import Case, wgrad

ROUTE = "wgrad_wino/rowq"

CASES = [
    # T = 60: the last half-group lies past T, the halves of a group lie in different tile rows (TW = 4), and group 2
    # (tiles 16 .. 23) straddles images 0 and 1 (20 tiles per image)
    Case("stage_10x8_T60", ROUTE, wgrad(3, 10, 32, 32, 2, W=8)),
    # T = 72: 9 groups, gps padded to 10: every unit of the last group is out of range
    Case("stage_12x8_T72", ROUTE, wgrad(3, 12, 32, 32, 2, W=8)),
    # two c tiles x two n tiles: a pixel's channels are 256 B apart, a unit is 8 runs of 128 B
    Case("stage_8x16_N64", ROUTE, wgrad(2, 8, 64, 64, 2, W=16, epi={"scale": "shared"})),
    # the smallest: T = 16, one stage, each buffer written once
    Case("stage_8x8", ROUTE, wgrad(1, 8, 32, 32, 2)),
    # 1 024 tiles split over 8 blocks per (probe, c tile, n tile) on 256 CUs: float atomics into the preset block
    Case("stage_32x32_split", ROUTE, wgrad(4, 32, 32, 32, 2), det=False),
]
for _c in CASES:
    _c.tol = "wino"

DET = [c for c in CASES if c.det]
