"""Case table and runner of tests/test_first_layer.py — TEST INFRASTRUCTURE (a plain helper module).

The first layer of a conv net as one synthetic op each: the tangent igemm_first (3 x 3 x 3 -> 32, pad 1) and the weight
gradient wgrad_first.  R = 2 x 32 x 32 = 2048 is the smallest R wgrad_first takes; R = 3 x 30 x 30 = 2700 ends on a
wave of 12 rows (2700 = 42 x 64 + 12), so the row tail of both kernels is not a multiple of 64.  P = 8 and 9: the
smallest probe count of igemm_first, and an odd one.  run_all() is shared by the test (default routes) and by
first_layer_child.py (the same ops in a process started with LIP_NOFIRST=1: the generic kernels).
"""
from __future__ import annotations

import torch

from kernel_route_cases import Case, conv, wgrad

EPI = {"scale": "shared", "e0": "probe", "e1": "probe", "xhat": "shared", "dphi": "shared"}


def cases():
    cs = []
    for n, H in ((2, 32), (3, 30)):
        for P in (8, 9):
            cs.append(Case(f"tan_n{n}_H{H}_P{P}_plain", "igemm_first<14>", conv(n, H, 3, 32, P, b_pp=True)))
            cs.append(Case(f"tan_n{n}_H{H}_P{P}_bn", "igemm_first<14>", conv(n, H, 3, 32, P, b_pp=True, epi=EPI)))
            for N in (32, 24):
                cs.append(Case(f"wg_n{n}_H{H}_P{P}_N{N}", "wgrad_first<32>", wgrad(n, H, 3, N, P), det=False))
    # an output that is not 16-byte aligned: the same layout with dword accesses
    cs.append(Case("tan_n3_H30_P9_bn_shift", "igemm_first<14>", conv(3, 30, 3, 32, 9, b_pp=True, epi=EPI, out_shift=1)))
    return cs


def output(got, outs):
    """the op's main output as one (P, count) tensor"""
    name, sp, base, count, ps, Pn, pre = outs[0]
    return torch.stack([got[sp][base + p * ps: base + p * ps + count] for p in range(Pn)])
