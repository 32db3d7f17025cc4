"""CPU: the table of tests/test_ab_switches.py (tests/ab_switch_cases.py) checked without a GPU.

* every row name resolves, every expected route differs from the row's default route, every ``unchanged`` row is a row;
* every switch has a square row and an anisotropic ("an_") row, unless its kernel has no spatial axes;
* the new geometries pass the float64-emulator-against-torch check of tests/test_kernel_routes_cpu.py, and the
  anisotropic ones fail check() with the two axes exchanged;
* the ``getenv("LIP_...")`` names of csrc/*.hip are exactly the switches the table covers plus the documented exclusions:
  a switch added later without a row fails here;
* tests/ab_child.py without a GPU ends non-zero with one clear line, not a traceback.
"""
import glob
import os
import re
import subprocess
import sys

import pytest

import ab_switch_cases as ab
import krylov_cases as kc
import test_kernel_routes_cpu as RC
from test_kernel_routes_cpu import cpu_harness  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "laplace-inducing-points_amd", "csrc")
NO_AXES = {"LIP_DOT_NT_VALU", "LIP_DOT_NT_NOQUAD"}          # lip_dot_nt_f64: two matrices, no map


def _all_rows(e):
    return [r for r, _ in e.rows + e.startup_rows] + list(e.unchanged)


def test_rows_resolve_and_routes_differ():
    known = set(ab.CONV_ROWS) | set(ab.DOT_ROWS)
    every = set()
    for e in ab.ENTRIES:
        rows = _all_rows(e)
        assert len(set(rows)) == len(rows), f"{e.name}: a row twice"
        assert set(rows) <= known, f"{e.name}: unknown rows {sorted(set(rows) - known)}"
        assert e.why and (rows or e.first_launch), e.name
        for row, route in e.rows + e.startup_rows:
            assert route != ab.default_route(row), f"{e.name}: {row}: the expected route {route} is the row's default route"
            assert (row in ab.CONV_ROWS) == route.startswith(("igemm", "wgrad")), (e.name, row, route)
            every.add(route)
        for k in e.env:
            assert k.startswith("LIP_")
    # the routes no default launch reaches, and the tiles that exist only behind LIP_TILE
    import test_kernel_routes as T
    assert T.AB_ONLY | kc.VALU_ONLY <= every
    for t in ("1,1,1,1", "1,1,1,2", "1,1,2,1"):
        assert {f"igemm_fast<{t}>", f"igemm_fast<{t}>/bv4", f"igemm<{t}>"} <= every, t
    for t in ("4,1,2,1", "4,1,2,2"):
        assert any(r.startswith(f"igemm_adirect<{t}>") for r in every) and any(r.startswith(f"igemm_fast<{t}>") for r in every), t


def test_every_switch_has_a_square_and_an_anisotropic_row():
    by_switch = {}
    for e in ab.ENTRIES:
        for k in e.env:
            by_switch.setdefault(k, []).extend(_all_rows(e))
    for k, rows in by_switch.items():
        if k in NO_AXES:
            assert all(r in ab.DOT_ROWS for r in rows), k
            continue
        segs = [(ab.CONV_ROWS[r].spec.segs[0], ab.CONV_ROWS[r].spec) for r in rows]
        assert any(g.IH == g.IW and g.KH == g.KW and g.pad == g.pad_w for g, _ in segs), f"{k}: no square row"
        assert any(g.IH != g.IW and s.n_img >= 2 for g, s in segs), f"{k}: no anisotropic row"
        assert any(r.startswith("an_") for r in rows), k


def test_dot_nt_switches_take_every_row():
    rows = {c.name for c in kc.CASES if c.prim == "dot_nt_f64"}
    assert set(_all_rows(ab.BY_ENTRY["dot_nt_valu"])) == rows and not ab.BY_ENTRY["dot_nt_valu"].unchanged
    assert set(_all_rows(ab.BY_ENTRY["dot_nt_noquad"])) == rows
    for e in (ab.BY_ENTRY["dot_nt_valu"], ab.BY_ENTRY["dot_nt_noquad"]):
        for row, route in e.rows:
            d = kc.BY_NAME[row].d
            assert route.rsplit("/", 1)[1] == kc.dot_nt_plan(d["m"], d["n"], d["K"])[0].rsplit("/", 1)[1], row
        assert {r.rsplit("/", 1)[1] for _, r in e.rows} == {"part", "atomic"}, e.name


@pytest.mark.parametrize("case", ab.NEW_CASES, ids=[c.name for c in ab.NEW_CASES])
def test_new_geometry_reference(cpu_harness, case):  # noqa: F811
    RC.test_emulator_matches_torch(cpu_harness, case)
    sg = case.spec.segs[0]
    assert case.name.startswith("an_") == (sg.IH != sg.IW)
    if case.name.startswith("an_"):
        RC.test_axis_swap_fails_the_check(cpu_harness, case)


def test_time_limits_cover_every_entry():
    import test_ab_switches as G
    assert set(G.ROWS_S) == set(ab.BY_ENTRY) and G.STARTUP_S > 0
    assert all(0 < G.time_limit(e) <= 600 for e in ab.ENTRIES)


# ---------------------------------------------------------------------------------------------- completeness
def switches_in(paths):
    """the names of every getenv("LIP_...") of the sources"""
    found = set()
    for p in paths:
        with open(p) as f:
            found |= set(re.findall(r'getenv\(\s*"(LIP_[A-Z0-9_]+)"\s*\)', f.read()))
    return found


def _covered():
    return {k for e in ab.ENTRIES for k in e.env}


def test_every_switch_of_the_sources_is_covered_or_excluded():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(sources) >= 4
    found = switches_in(sources)
    assert not (_covered() & ab.EXCLUDED)
    missing = found - _covered() - ab.EXCLUDED
    assert not missing, f"switches of csrc/*.hip without an entry in ab_switch_cases.py (or a documented exclusion): {sorted(missing)}"
    stale = (_covered() | ab.EXCLUDED) - found
    assert not stale, f"ab_switch_cases.py names switches the sources no longer read: {sorted(stale)}"


def test_the_scan_sees_a_new_switch(tmp_path):
    with open(os.path.join(CSRC, "lip_mfma.hip")) as f:
        text = f.read()
    p = tmp_path / "lip_mfma.hip"
    p.write_text(text + '\nstatic const bool foo = getenv("LIP_FOO") != nullptr;\n')
    assert switches_in([str(p)]) - _covered() - ab.EXCLUDED == {"LIP_FOO"}


# ---------------------------------------------------------------------------------------------- the child
def _no_gpu():
    import torch
    return torch.cuda.device_count() == 0


def test_child_cuts_names_that_hold_commas():
    import ab_child
    known = set(ab.CONV_ROWS) | set(ab.DOT_ROWS)
    got = ab_child.parse_rows("fast2,2,1,2_bv4@startup:x3,wg_skinny8,adirect4,1,1,1:exact,dot_nt_f64/K1", known)
    assert got == [("fast2,2,1,2_bv4", "x3", True), ("wg_skinny8", None, False), ("adirect4,1,1,1", "exact", False),
                   ("dot_nt_f64/K1", None, False)]
    assert ab_child.parse_rows("", known) == []
    with pytest.raises(KeyError):
        ab_child.parse_rows("wg_skinny8,no_such_row", known)


@pytest.mark.skipif(not _no_gpu(), reason="CPU-only behaviour")
def test_child_without_a_gpu_says_so():
    child = os.path.join(ROOT, "tests", "ab_child.py")
    r = subprocess.run([sys.executable, child, ""], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "no GPU" in r.stderr and "Traceback" not in r.stderr, r.stderr[-1000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
