"""GPU: the staged cotangent of the Winograd weight gradient (wgrad_wino/rowq), op by op against float64.

The block fetches the probe's cotangent once per stage of two tile groups, through two LDS buffers, instead of once per
wave.  Every case runs as in tests/test_kernel_routes.py (route census, every element against the float64 emulator at
the Winograd constants, canaries, accumulation prefill; a second run bit for bit where no float atomics take part).

LIP_WGW_NOSTAGE=1 selects the per-wave loop as a second instantiation of the same route.  Both hand the same operands
to the same MFMAs in the same order, so the deterministic cases must agree BITWISE between a process with the switch
and one without it (read once per process: child processes, as in tests/test_bind_cache.py).
"""
import os
import subprocess
import sys

import pytest
import torch

from test_kernel_routes import run_case
from wgrad_stage_cases import CASES, DET, ROUTE
from wgrad_stage_child import outputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCH = "LIP_WGW_NOSTAGE"
_RUNS = {}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stage_case(case):
    census, stats = run_case(case)
    print(case.name, stats)
    assert census == {ROUTE: 1}, f"{case.name}: expected the route {ROUTE}, the census shows {census}"


def _child(tmp_path_factory, tag, env):
    out = tmp_path_factory.mktemp("wgrad_stage") / f"{tag}.pt"
    r = subprocess.run([sys.executable, os.path.join(HERE, "wgrad_stage_child.py"), str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child {tag} failed ({r.returncode}): {r.stderr[-2000:]}"
    return torch.load(out)


def runs(tmp_path_factory):
    """staged: this process, unless it was started with the switch itself; nostage: a child with the switch"""
    if not _RUNS:
        env = {k: v for k, v in os.environ.items() if k != SWITCH}
        _RUNS["staged"] = outputs() if SWITCH not in os.environ else _child(tmp_path_factory, "staged", env)
        _RUNS["nostage"] = _child(tmp_path_factory, "nostage", dict(env, **{SWITCH: "1"}))
    return _RUNS


@pytest.mark.parametrize("case", DET, ids=[c.name for c in DET])
def test_switch_parity(tmp_path_factory, case):
    r = runs(tmp_path_factory)
    a, b = r["staged"][case.name], r["nostage"][case.name]
    assert a["census"] == {ROUTE: 1} and b["census"] == {ROUTE: 1}, (a["census"], b["census"])
    assert set(a["spaces"]) == set(b["spaces"]) and a["spaces"]
    for sp in a["spaces"]:
        x, y = a["spaces"][sp], b["spaces"][sp]
        ne = x.view(torch.int32) != y.view(torch.int32)
        d = (x.double() - y.double()).abs()
        print(f"{case.name}: space {sp}: {int(ne.sum())} of {ne.numel()} floats differ, max |diff| {d[ne].max().item() if ne.any() else 0.0:.3g}")
        assert not ne.any(), f"{case.name}: space {sp}: {int(ne.sum())} of {ne.numel()} floats differ between the staged and the per-wave loop"
