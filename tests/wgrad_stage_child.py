"""The runs of the switch-parity test of tests/test_wgrad_wino_stage.py, and its child process.

    python tests/wgrad_stage_child.py OUT.pt

outputs() runs the deterministic cases of tests/wgrad_stage_cases.py once each through lip_engine_run_op, in the
environment of THIS process (LIP_WGW_NOSTAGE is read once per process), and returns per case the route census of the
launch and every space that holds an output of the op, canaries around it included.  A plain script: not a test module,
not a conftest.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def outputs():
    import lip_amd  # noqa: F401
    import test_kernel_routes as T
    from wgrad_stage_cases import DET
    h = T.harness()
    res = {}
    for case in DET:
        op, L, host, outs = h.build(case.spec, 0)
        prev = T.set_modes(h.lib, case)
        try:
            dev = h.upload(host)
            h.routes()
            h.run(op, dev, case.spec.P)
            census = h.routes()
            got = h.download(dev)
        finally:
            T.restore_modes(h.lib, prev)
        res[case.name] = {"census": census, "spaces": {sp: got[sp].clone() for sp in sorted({o[1] for o in outs})}}
    return res


def main(argv):
    if len(argv) != 2:
        print("usage: wgrad_stage_child.py OUT.pt", file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        print("wgrad_stage_child: no GPU in this process", file=sys.stderr)
        return 3
    torch.save(outputs(), argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
