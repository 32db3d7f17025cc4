"""The call sequence of tests/test_bind_cache.py, and its child process.

    python tests/bind_cache_child.py OUT.pt

sequence() runs, on a two-stage toy ResNet (8 x 8 maps at 32 channels: the stage whose 3 x 3 layers take the Winograd
kernels; 4 x 4 at 64), the calls whose results must not depend on the engine's transform cache:

    y1, y2   the same GGN block product twice                       (the second finds every transform cached)
    z1       a product on a SECOND engine (other weights and inputs) bound on the same stream
    y3       the first engine again after the second
    y4       after theta changed IN PLACE and the primal pass was re-run (the cache must have dropped what it held)
    j1       a tangent sweep alone (lip_jvp) on the new weights

The test runs it in-process (cache on) and starts this script with LIP_NOBINDCACHE=1 and with LIP_BINDCACHE_MB=0 (both
read once per process).  A plain script: not a test module, not a conftest.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_IMG, P = 4, 4


def sequence(reference=None):
    """the outputs by name (CPU tensors).  reference(eng, state, Z, V): called after y1 and y4 with the first engine and after z1
    with the second; what it returns is kept as ref1 / ref4 / refz (the test's float64 emulation of the product just made)."""
    import torch
    import lip_amd  # noqa: F401
    from lip_amd import _native as nv
    from lip_amd.engine import LinearizedNet
    from lip_amd.scalemodels import ResNet1M
    from lip_amd.toymodels import create_state

    def bind(seed):
        net = ResNet1M(10, input_shape=(8, 8, 3), widths=(32, 64), blocks_per_stage=1)
        st = create_state(net, seed, dtype=torch.float64)
        Z = torch.rand(N_IMG, 8, 8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
        return LinearizedNet(st, Z, "classifier", workspace_bytes=1 << 28, max_chunk=P), st, Z

    def census(lib):
        import ctypes as C
        n = lib.lip_debug_route_count()
        counts, names = (C.c_int64 * n)(), (C.c_char_p * n)()
        nv.check(lib.lip_debug_routes(counts, n, names), "lip_debug_routes")
        return {names[i].decode(): counts[i] for i in range(n) if counts[i]}

    (eng, st, Z), (eng2, st2, Z2) = bind(3), bind(4)
    V = torch.randn(P, eng.D, generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    census(eng.lib)
    out["y1"] = eng.ggn_vp(V, 1.3, 0.25).clone()
    out["routes"] = census(eng.lib)
    if reference:
        out["ref1"] = reference(eng, st, Z, V)
    out["y2"] = eng.ggn_vp(V, 1.3, 0.25).clone()
    out["z1"] = eng2.ggn_vp(V, 1.3, 0.25).clone()
    if reference:
        out["refz"] = reference(eng2, st2, Z2, V)
    out["y3"] = eng.ggn_vp(V, 1.3, 0.25).clone()
    noise = torch.randn(eng.theta.numel(), generator=torch.Generator().manual_seed(6)).cuda()
    eng.theta.add_(0.05 * noise.reshape(eng.theta.shape))             # in place: the bound pointer stays
    nv.check(eng.lib.lip_engine_primal(eng.h, nv.stream_ptr()), "lip_engine_primal")
    out["y4"] = eng.ggn_vp(V, 1.3, 0.25).clone()
    if reference:
        out["ref4"] = reference(eng, st, Z, V)
    out["j1"] = eng.jvp(V, "lt", 1.0).clone()
    torch.cuda.synchronize()
    return {k: (v.cpu() if hasattr(v, "cpu") else v) for k, v in out.items()}


def main(argv):
    if len(argv) != 2:
        print("usage: bind_cache_child.py OUT.pt", file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        print("bind_cache_child: no GPU in this process", file=sys.stderr)
        return 3
    torch.save(sequence(), argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
