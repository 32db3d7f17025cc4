"""GPU: the first-layer kernels (igemm_first with its transposed 16-byte-store tile, wgrad_first with two probes per
wave) against float64, and the tangent bit for bit against the generic kernel.

Rows: tests/first_layer_cases.py.  Every row runs through tests/test_kernel_routes.run_case — census, the float64
bound of the exact routes (Ktot + 16) x 2^-24 Mag, RMS, canaries, accumulation prefill, a bitwise second run where the
route has no float atomics — so the tolerances are those of tests/test_kernel_routes.py.  The tangent rows are then run
once more with split-K off and compared bitwise with the same ops in a child process started with LIP_NOFIRST=1
(tests/first_layer_child.py): both kernels form every output element as one sum over k in ascending order followed by
the same epilogue expression, so they must agree to the bit.
"""
import os
import subprocess
import sys

import pytest
import torch

import test_kernel_routes as T
from first_layer_cases import cases
from first_layer_child import run_tangents

pytestmark = pytest.mark.gpu

CASES = cases()
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_first_layer_route_against_float64(case):
    census, stats = T.run_case(case)
    print(f"{case.name}: {stats}")
    assert census == {case.route: 1}, f"{case.name}: expected the route {case.route}, the census shows {census}"


def test_tangent_bitwise_equal_to_the_generic_kernel(tmp_path):
    out = tmp_path / "generic.pt"
    env = dict(os.environ, LIP_NOFIRST="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "first_layer_child.py"), str(out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, f"child failed ({r.returncode}): {r.stderr[-2000:]}"
    generic = torch.load(out)
    mine, census = run_tangents(T.harness(), CASES)
    assert mine, "no tangent rows"
    for name, y in mine.items():
        assert census[name] == {"igemm_first<14>": 1}, f"{name}: census {census[name]}"
        assert not any("first" in k for k in generic["census"][name]), f"{name}: the child took {generic['census'][name]}"
        ne = y.view(torch.int32) != generic[name].view(torch.int32)
        d = (y.double() - generic[name].double()).abs().max().item()
        print(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the generic kernel, max |diff| {d:.3g}")
        assert not ne.any(), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the generic kernel (max |diff| {d:.3g})"
