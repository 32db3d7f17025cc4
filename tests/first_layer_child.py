"""Child process of tests/test_first_layer.py: the tangent rows of first_layer_cases.py in THIS process's environment.

    python tests/first_layer_child.py OUT.pt

The parent starts it with LIP_NOFIRST=1 (read once per process), so the ops take the generic kernels.  Split-K is off
in both processes: every output element is then one sum over k in ascending order in both kernels.  Writes
{case name: (P, R N) float32 output} and {"census": {case name: routes}} with torch.save.  A plain script: not a test
module, not a conftest.  Exit status 0 when every row ran; nothing more is launched after a HIP error.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def run_tangents(h, cases):
    """{name: output}, {name: census} of the igemm rows, split-K off"""
    import torch
    from lip_amd import _native as nv
    from first_layer_cases import output
    outs_by, census = {}, {}
    nv.check(h.lib.lip_set_split_k(0), "lip_set_split_k")
    try:
        for case in cases:
            if case.spec.kind != nv.OP_IGEMM:
                continue
            op, L, host, outs = h.build(case.spec, 0)
            dev = h.upload(host)
            h.routes()
            h.run(op, dev, case.spec.P)
            census[case.name] = h.routes()
            outs_by[case.name] = output(h.download(dev), outs).clone()
            del dev
    finally:
        h.lib.lip_set_split_k(1)
    return outs_by, census


def main(argv):
    if len(argv) != 2:
        print("usage: first_layer_child.py OUT.pt", file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        print("first_layer_child: no GPU in this process", file=sys.stderr)
        return 3
    import lip_amd  # noqa: F401
    from op_harness import Harness
    from first_layer_cases import cases
    outs_by, census = run_tangents(Harness(max_chunk=16), cases())
    outs_by["census"] = census
    torch.save(outs_by, argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
