"""Child process of tests/test_ab_switches.py: runs rows of the case tables in THIS process's environment.

    python tests/ab_child.py ROW[,ROW...]

The A/B switches of the library (``LIP_...``) are read once per process, so the parent starts one child per switch with
the switch in the child's environment.  A plain script: not a test module, not a conftest.

ROW is a name of ab_switch_cases.CONV_ROWS (run through test_kernel_routes.run_case: the same float64 check, bounds,
canaries, accumulation prefill and bitwise second run as tests/test_kernel_routes.py) or of a ``dot_nt_f64`` row of
krylov_cases (run through test_krylov_ops.run_case with exact and with random inputs).  Tile names hold commas
("fast2,2,1,2"), so the list is cut greedily at the longest known name.  Two suffixes:

    ROW:TOL        the tolerance class ("exact" | "wino" | "x3") of the kernel the row is expected to land on, where it
                   is not the class of the row's default route
    ROW@startup    run in the precision, Winograd and split-K modes this process STARTED with (LIP_PRECISION, LIP_NOWINO,
                   LIP_WINO, LIP_NOKSPLIT): run_case calls no setter for it.  Such rows come first in the list, since
                   every other row sets the modes and leaves split-K on

Output: one JSON object per line.  First {"startup": {"precision", "winograd", "first_launch"}}: the two getters and the
census of one split-K-eligible launch (ab_switch_cases.KS_ROW), all before any setter is called.  Then per row
{"row", "census", "stats": {output: [max normalised error, rms / sqrt(K)]}, "error": text of the AssertionError or null,
"seconds"}.  Exit status 0 when every row was run, whatever the verdicts; non-zero when the child could not run (no GPU,
no library, an unknown row, a HIP error: nothing more is launched after one).
"""
import dataclasses
import json
import os
import sys
import time

T0 = time.time()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TOLS = ("exact", "wino", "x3")


def die(status, msg):
    print(f"ab_child: {msg}", file=sys.stderr, flush=True)
    sys.exit(status)


def parse_rows(arg, known):
    """[(row, tol or None, startup)] of a comma-separated list whose names may hold commas themselves"""
    pieces = [p for p in arg.split(",")] if arg else []
    out, i = [], 0
    while i < len(pieces):
        for j in range(min(len(pieces), i + 4), i, -1):
            tok = ",".join(pieces[i:j])
            name, _, tol = tok.partition(":")
            name, at, mark = name.partition("@")
            if name in known and (not at or mark == "startup") and (not tol or tol in TOLS):
                out.append((name, tol or None, bool(at)))
                i = j
                break
        else:
            raise KeyError(",".join(pieces[i:i + 4]))
    return out


def emit(obj):
    print(json.dumps(obj), flush=True)


def main(argv):
    if len(argv) != 2:
        die(2, "usage: ab_child.py ROW[,ROW...]   (see the module docstring)")
    import torch
    if not torch.cuda.is_available():
        die(3, "no GPU in this process (torch.cuda.is_available() is false): the rows are kernel launches, nothing was run")
    import lip_amd  # noqa: F401
    from lip_amd import _native as nv
    try:
        lib = nv.load()
    except (OSError, ImportError) as e:
        die(4, f"the library could not be loaded ({e}): build it first (__graft_entry__.build())")
    import ab_switch_cases as ab
    import krylov_cases as kc
    import krylov_harness as kh
    import test_kernel_routes as T
    import test_krylov_ops as K
    known = set(ab.CONV_ROWS) | set(ab.DOT_ROWS)
    try:
        rows = parse_rows(argv[1], known)
    except KeyError as e:
        die(5, f"unknown row at {e} (names: ab_switch_cases.CONV_ROWS, the dot_nt_f64 rows of krylov_cases)")

    # ---- start-up defaults, before any setter
    prec0, wino0 = lib.lip_get_precision(), lib.lip_get_winograd()
    h = T.harness()
    case = ab.CONV_ROWS[ab.KS_ROW]
    op, L, host, outs = h.build(case.spec, 0)
    dev = h.upload(host)
    h.routes()
    h.run(op, dev, case.spec.P)
    emit({"startup": {"precision": prec0, "winograd": wino0, "first_launch": h.routes(), "seconds": time.time() - T0}})
    del dev

    # the census of a row's first run, kept when the check that follows it fails
    seen = []
    h_routes, kh_routes = h.routes, kh.routes

    def conv_routes():
        seen.append(h_routes())
        return seen[-1]

    def dot_routes(lib_):
        seen.append(kh_routes(lib_))
        return seen[-1]

    h.routes, kh.routes = conv_routes, dot_routes
    if any(s and not rows[i - 1][2] for i, (_, _, s) in enumerate(rows) if i):
        die(5, "the @startup rows must come first: the rows after them call the mode setters")
    set_modes, restore_modes = T.set_modes, T.restore_modes
    for name, tol, startup in rows:
        t0 = time.time()
        # a start-up row runs in the modes the process has had since it started: no setter before, none after
        T.set_modes, T.restore_modes = ((lambda lib_, case_: None), (lambda lib_, prev: None)) if startup else (set_modes, restore_modes)
        del seen[:]
        census, stats, err = None, {}, None
        try:
            if name in ab.CONV_ROWS:
                case = ab.CONV_ROWS[name]
                if tol:
                    case = dataclasses.replace(case, tol=tol)
                census, stats = T.run_case(case)
            else:
                for exact in (True, False):
                    c, s = K.run_case(kc.BY_NAME[name], exact)
                    census = c if census is None else census
                    assert c == census, f"{name}: the run with random inputs counted {c}, the run with exact inputs {census}"
                    for k, v in s.items():
                        stats[k] = tuple(max(a, b) for a, b in zip(stats.get(k, (0.0, 0.0)), v))
        except AssertionError as e:
            err = str(e) or repr(e)
            if census is None and len(seen) >= 2:
                census = seen[1]               # seen[0] is the read that clears the census
        except Exception as e:                 # a HIP error or anything else that is not a verdict: launch nothing more
            emit({"row": name, "census": census, "stats": {}, "error": f"{type(e).__name__}: {e}", "seconds": time.time() - t0})
            die(6, f"row {name} could not be run: {type(e).__name__}: {e}")
        emit({"row": name, "census": census, "stats": {k: list(v) for k, v in stats.items()}, "error": err, "seconds": time.time() - t0})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
