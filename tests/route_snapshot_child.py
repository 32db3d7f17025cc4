"""The child process of tests/test_route_snapshot.py, and the toy binding both share.

    LIP_NOBINDCACHE=1 python tests/route_snapshot_child.py OUT.pt

The library keeps float scratch for 16 (device, stream) pairs per process.  Without the engine's transform cache the
transformed activations of a Winograd weight gradient live in that scratch, so a product on a 17th stream has to take
the direct kernels, for the weight gradients that the first 16 streams run fused (overwrite) as well.  seventeen_streams()
makes the same GGN block product on 17 fresh streams, one after the other, and once more on the first stream with the
Winograd route switched off; it keeps the first and the last result, that one, and the route census of each.

A process of its own, so that the 16 records of the pytest process are not used up.  A plain script: not a test module,
not a conftest.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_IMG, P = 4, 4
N_STREAMS = 17          # one more than the library's per-stream tables hold


def bind(seed=3):
    """the toy net of tests/bind_cache_child.py: 8 x 8 maps at 32 channels, 4 x 4 at 64; 4 images, up to 4 probes per pass"""
    import torch
    import lip_amd  # noqa: F401
    from lip_amd.engine import LinearizedNet
    from lip_amd.scalemodels import ResNet1M
    from lip_amd.toymodels import create_state
    net = ResNet1M(10, input_shape=(8, 8, 3), widths=(32, 64), blocks_per_stage=1)
    st = create_state(net, seed, dtype=torch.float64)
    Z = torch.rand(N_IMG, 8, 8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    eng = LinearizedNet(st, Z, "classifier", workspace_bytes=1 << 28, max_chunk=P)
    V = torch.randn(P, eng.D, generator=torch.Generator().manual_seed(5)).cuda()
    return eng, V


def census(lib):
    """{route name: launches} since the last call (reading clears the counts)"""
    import ctypes as C
    from lip_amd import _native as nv
    n = lib.lip_debug_route_count()
    counts, names = (C.c_int64 * n)(), (C.c_char_p * n)()
    nv.check(lib.lip_debug_routes(counts, n, names), "lip_debug_routes")
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


def product(eng, V):
    """(GGN + 0.25 I) V at scale 1.3 on the current stream, with the census of exactly this call"""
    census(eng.lib)
    y = eng.ggn_vp(V, 1.3, 0.25).clone()
    return y, census(eng.lib)


def seventeen_streams():
    import torch
    from lip_amd import _native as nv
    eng, V = bind()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(N_STREAMS)]
    assert len({s.cuda_stream for s in streams}) == N_STREAMS
    out = {"routes": [], "error": None}
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            try:
                y, routes = product(eng, V)
            except nv.NativeError as e:         # kept for the test to report: the call must succeed
                out["error"] = f"stream {i}: {e}"
                break
            s.synchronize()
        out["routes"].append(routes)
        if i == 0:
            out["y_first"] = y.cpu()
        if i == N_STREAMS - 1:
            out["y_last"] = y.cpu()
    with torch.cuda.stream(streams[0]), nv.winograd_route(0):
        y, out["routes_direct"] = product(eng, V)
        streams[0].synchronize()
    out["y_direct"] = y.cpu()
    return out


def main(argv):
    if len(argv) != 2:
        print("usage: route_snapshot_child.py OUT.pt", file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        print("route_snapshot_child: no GPU in this process", file=sys.stderr)
        return 3
    torch.save(seventeen_streams(), argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
