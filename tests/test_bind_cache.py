"""GPU: the engine's per-binding cache of Winograd transforms (transformed shared kernels U, transformed primal
activations Vt) never changes a result.

tests/bind_cache_child.sequence() is run here with the cache on and, in child processes, with LIP_NOBINDCACHE=1 (today's
per-launch transforms) and with LIP_BINDCACHE_MB=0 (a cache that can hold nothing: every launch falls back).  A cached
transform is the output of the same kernel on the same input as the per-launch one, so whatever the engine computes
without float atomics must agree BITWISE across the three processes and between the repeated calls y1, y2, y3:

  * j1, the tangent sweep (lip_jvp): no kernel of it adds with atomics.  It reads every cached forward U.
  * in the products, the 3 x 3 kernels of the 32-channel stage (the only tensors of 3 * 3 * 32 * 32 floats): their
    gradients are the unsplit Winograd weight gradient, which reads the cached Vt and a cotangent that came through the
    cached flipped U of every layer above, all without atomics.

The other parameter cotangents (biases, BN parameters, the small and the split weight gradients) are summed with float
atomics and differ from run to run in the parent as well (measured: 1391 of 311464 elements of the same product twice,
by up to 2.4e-7).  They are compared per parameter tensor at 4e-5 of the float64 reference's largest entry: both sides
lie within 2e-5 of the float64 value (the tolerance of tests/test_kernel_routes.test_ggn_vp_fused_overwrite, asserted
here for y1, z1 and y4), so within 4e-5 of each other.  The product after an in-place change of theta and a new primal
pass (y4) is held to the same: a cache that kept a stale U or Vt is off by the size of the change.
"""
import os
import subprocess
import sys

import pytest
import torch

from bind_cache_child import sequence

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCTS = ("y1", "y2", "z1", "y3", "y4")
WINO_KERNEL_FLOATS = 3 * 3 * 32 * 32
_RUNS = {}


def _reference(eng, state, Z, V):
    """float64 (GGN + alpha I) V of the tape emulator on the weights the engine holds NOW, and the parameter slices"""
    from lip_amd.engine import build_consts
    from tape_emulator import TapeMachine
    from test_kernel_routes import _tensor_slices
    tm = TapeMachine(eng.cn, eng.theta.double().cpu(), build_consts(eng.cn, state.params, state.batch_stats, "cpu", torch.float64),
                     Z, chunk=eng.chunk)
    tm.primal()
    return tm.ggn_vp(V.double().cpu(), 1.3, 0.25), _tensor_slices(state.params)


def _child(tmp_path_factory, tag, env):
    out = tmp_path_factory.mktemp("bind_cache") / f"{tag}.pt"
    r = subprocess.run([sys.executable, os.path.join(HERE, "bind_cache_child.py"), str(out)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child {tag} failed ({r.returncode}): {r.stderr[-2000:]}"
    return torch.load(out)


def runs(tmp_path_factory):
    if not _RUNS:
        _RUNS["cached"] = sequence(_reference)
        _RUNS["nocache"] = _child(tmp_path_factory, "nocache", {"LIP_NOBINDCACHE": "1"})
        _RUNS["cap0"] = _child(tmp_path_factory, "cap0", {"LIP_BINDCACHE_MB": "0"})
    return _RUNS


def _same(a, b, what):
    ne = a.view(torch.int32) != b.view(torch.int32)
    d = (a.double() - b.double()).abs().max().item()
    print(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, max |diff| {d:.3g}")
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ (max |diff| {d:.3g})"


def _same_product(a, b, ref, slices, what):
    """bitwise on the Winograd layers' kernels, 4e-5 of the reference's largest entry on every other parameter tensor"""
    wino = [(n, lo, hi) for n, lo, hi in slices if hi - lo == WINO_KERNEL_FLOATS]
    assert len(wino) >= 2, [n for n, _, _ in slices]
    for name, lo, hi in slices:
        if hi - lo == WINO_KERNEL_FLOATS:
            _same(a[:, lo:hi].contiguous(), b[:, lo:hi].contiguous(), f"{what}: {name}")
        else:
            scale = ref[:, lo:hi].abs().max().item()
            d = (a[:, lo:hi].double() - b[:, lo:hi].double()).abs().max().item()
            assert d <= 4e-5 * scale + 1e-30, f"{what}: {name}: max |diff| {d:.3e} > 4e-5 x {scale:.3e}"


def _ref_of(r, call):
    """the float64 reference that scales the comparison of `call`"""
    return r["refz" if call == "z1" else "ref4" if call == "y4" else "ref1"]


def test_the_toy_net_takes_the_winograd_kernels(tmp_path_factory):
    rs = runs(tmp_path_factory)
    for tag, r in rs.items():
        routes = r["routes"]
        assert any(k.startswith("igemm_wino") for k in routes) and any(k.startswith("wgrad_wino") for k in routes), (tag, routes)
        assert routes == rs["nocache"]["routes"], f"{tag}: the cache changed a route: {routes} vs {rs['nocache']['routes']}"


@pytest.mark.parametrize("other", ["nocache", "cap0"])
def test_tangent_sweep_equals_the_per_launch_transforms(tmp_path_factory, other):
    r = runs(tmp_path_factory)
    _same(r["cached"]["j1"], r[other]["j1"], f"j1: cache on vs {other}")


@pytest.mark.parametrize("other", ["nocache", "cap0"])
@pytest.mark.parametrize("call", PRODUCTS)
def test_product_equals_the_per_launch_transforms(tmp_path_factory, call, other):
    r = runs(tmp_path_factory)
    ref, slices = _ref_of(r["cached"], call)
    _same_product(r["cached"][call], r[other][call], ref, slices, f"{call}: cache on vs {other}")


def test_repeated_products_agree(tmp_path_factory):
    r = runs(tmp_path_factory)["cached"]
    ref, slices = r["ref1"]
    _same_product(r["y1"], r["y2"], ref, slices, "first product vs the same product again")
    _same_product(r["y1"], r["y3"], ref, slices, "first product vs the same product after another engine's")
    assert not torch.equal(r["y1"], r["y4"]) and not torch.equal(r["y1"], r["z1"])
    # the weights did change: y4 is far from y1 where a stale cache would have left it
    name, lo, hi = next(s for s in slices if s[2] - s[1] == WINO_KERNEL_FLOATS)
    moved = (r["y4"][:, lo:hi] - r["y1"][:, lo:hi]).abs().max().item()
    assert moved > 1e-2 * ref[:, lo:hi].abs().max().item(), f"{name}: the new weights moved the product by {moved:.3e} only"


@pytest.mark.parametrize("call", ["y1", "z1", "y4"])
def test_products_against_float64(tmp_path_factory, call):
    from test_kernel_routes import _per_tensor
    r = runs(tmp_path_factory)["cached"]
    ref, slices = _ref_of(r, call)
    _per_tensor(r[call], ref, slices, 2e-5, f"ggn_vp {call}")
