"""GPU: the kernels that only an A/B environment switch reaches, and the ordinary shapes the switches re-route.

The library reads every ``LIP_...`` switch once per process, so each entry of tests/ab_switch_cases.py runs in a child
process of its own (tests/ab_child.py) with the switch in its environment, strictly one child after another.  For every
row the parent asserts that the census is exactly the expected route, that the float64 check of the op raised nothing
(tests/op_harness.check through test_kernel_routes.run_case; tests/krylov_harness through test_krylov_ops.run_case) and
that the statistics the child printed stay within the bounds of the row's tolerance class — the constants of
tests/test_kernel_routes.py, none of them changed.  Where the entry names them, the start-up getters and the route of
the first launch of the process (before any setter) are asserted too.

A child that dies (status other than 0, a signal, the time limit) ends the launches of this module: every later entry
is skipped, nothing is started again and nothing is retried.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import ab_switch_cases as ab
import krylov_cases as kc
import test_kernel_routes as T
from ab_switch_cases import ENTRIES

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ab_child.py")

# Time limit of a child, in seconds: 4 x (start-up + rows).  Measured on an MI355X, one run of every entry:
#   start-up: wall time of a child less the time of its rows (interpreter, torch, the library, the Harness, the first
#   launch): 2.5 .. 2.84 s over the 24 children, the first GPU process of the machine included
#   rows: the seconds run_case took in the child, summed per entry — the call test_route / test_krylov_op makes for the
#   same row, which the table takes from tests/kernel_route_cases.py and tests/krylov_cases.py unchanged (0.03 .. 0.4 s a
#   row; the six new geometries 1.2 s together)
STARTUP_S = 2.84
ROWS_S = {"defaults": 1.2, "noadirect": 1.9, "wgrad3": 0.5, "generic_igemm": 6.1, "generic_wgrad": 2.8, "nofirst": 1.2, "noskinny": 0.5,
          "nopb": 0.9, "nopb96": 0.3, "nopar": 6.6, "nobv4": 3.4, "wino_novepi": 1.0, "nosmallp": 0.8, "tile2": 0.9, "tile3": 0.5,
          "tile4": 1.2, "tile1": 1.2, "tile1_noadirect": 1.2, "dot_nt_valu": 7.4, "dot_nt_noquad": 6.3, "precision_bf16x3": 0.2,
          "nowino": 0.2, "wino_f": 0.1, "noksplit": 0.2}


def time_limit(entry):
    return int(4 * (STARTUP_S + ROWS_S[entry.name])) + 1


_dead = None                          # "<entry>, status <n>" of the first child that died


def _tokens(entry):
    toks = [f"{row}@startup:{ab.tol_of_route(route)}" for row, route in entry.startup_rows]     # (they come first)
    for row, route in entry.rows:
        tol = ab.tol_of_route(route)
        toks.append(row if row not in ab.CONV_ROWS or tol == ab.CONV_ROWS[row].tol else f"{row}:{tol}")
    return toks + entry.unchanged


def _bounds_hold(row, route, stats):
    """the printed statistics against the class bounds of tests/test_kernel_routes.py (dot_nt_f64: of its builder)"""
    if row in ab.CONV_ROWS:
        import dataclasses
        k_of, rms_c = T.tolerances(dataclasses.replace(ab.CONV_ROWS[row], tol=ab.tol_of_route(route)))
        for name, (worst, rms) in stats.items():
            assert worst <= k_of(name)[0], f"{row}: {name}: worst error {worst:.4g} above {k_of(name)[0]:.4g} x 2^-24 Mag"
            assert rms <= rms_c, f"{row}: {name}: rms / sqrt(K) {rms:.4g} above {rms_c}"
    else:
        import krylov_harness as kh
        outs = kh.BUILDERS["dot_nt_f64"](kc.BY_NAME[row].d, False, seed=2).outs
        for name, (worst, rms) in stats.items():
            assert worst <= outs[name].k, f"{row}: {name}: worst error {worst:.4g} above {outs[name].k:.4g} units of Mag"
            assert rms <= kh.RMS_EXACT, f"{row}: {name}: rms / sqrt(L) {rms:.4g} above {kh.RMS_EXACT}"


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_switch(entry):
    global _dead
    if _dead:
        pytest.skip(f"an earlier child died: {_dead}")
    env = {**os.environ, **entry.env}
    args = [sys.executable, CHILD, ",".join(_tokens(entry))]
    try:
        r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=time_limit(entry))
    except subprocess.TimeoutExpired as e:
        _dead = f"{entry.name}, time limit of {time_limit(entry)} s"
        err = e.stderr.decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        raise AssertionError(f"the child of {entry.name} ran into its time limit of {time_limit(entry)} s; stderr ends:\n{err[-2000:]}")
    if r.returncode != 0:
        _dead = f"{entry.name}, status {r.returncode}"
        raise AssertionError(f"the child of {entry.name} ended with status {r.returncode}; stdout ends:\n{r.stdout[-1000:]}\n"
                             f"stderr ends:\n{r.stderr[-2000:]}")
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    start, got = lines[0]["startup"], {l["row"]: l for l in lines[1:]}
    want = [(row, route, True) for row, route in entry.rows + entry.startup_rows] + \
           [(row, ab.default_route(row), False) for row in entry.unchanged]
    assert len(lines) == 1 + len(want) and set(got) == {w[0] for w in want}, f"{entry.name}: rows reported: {sorted(got)}"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"AB {entry.name} start-up {start}")
    failures, skipped = [], []
    for row, route, _ in want:
        g = got[row]
        print(f"AB {entry.name} {row}: {g['census']} {g['stats']} {g['seconds']:.2f} s")
        if row in ab.CONV_ROWS and ab.CONV_ROWS[row].cu and cus != T.MI355X_CUS:
            skipped.append(row)                    # (numbers still checked)
        elif g["census"] != {route: 1}:
            failures.append(f"{row}: expected the route {route}, the census shows {g['census']}")
        if g["error"]:
            failures.append(f"{row}: {g['error']}")
        else:
            try:
                _bounds_hold(row, route, g["stats"])
            except AssertionError as e:
                failures.append(str(e))
    if entry.precision is not None:
        if start["precision"] != entry.precision:
            failures.append(f"lip_get_precision() at start-up: {start['precision']}, expected {entry.precision}")
        if start["winograd"] != entry.winograd:
            failures.append(f"lip_get_winograd() at start-up: {start['winograd']}, expected {entry.winograd}")
        # (the first launch is the geometry of ks_2211_bv4: its split-K route assumes 256 CUs)
        if cus == T.MI355X_CUS and start["first_launch"] != {entry.first_launch: 1}:
            failures.append(f"first launch of the process: {start['first_launch']}, expected {entry.first_launch}")
    assert not failures, f"{entry.name} ({entry.env}): " + "\n".join(failures)
    if skipped:
        pytest.skip(f"routes of {skipped} assume {T.MI355X_CUS} CUs, this device has {cus} (numbers checked)")

