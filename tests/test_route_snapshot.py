"""GPU: a call's route is decided once, and the overwrite plan made from it holds when the scratch table is full.

*The 17th stream* (tests/route_snapshot_child.py, a child process with LIP_NOBINDCACHE=1).  On the toy net every 3 x 3
weight gradient of the 32-channel stage is Winograd-eligible with one split at 4 probes, so lip_ggn_vp plans it as
overwrite: its range of Y is not initialised and the fused launch writes y = s acc + alpha v.  The library keeps
per-stream scratch for 16 (device, stream) pairs; on a 17th stream the Winograd launches cannot be made.  The product
there must succeed on the direct kernels and agree with the Winograd product of the first stream and with the direct
product (lip_set_winograd(0)) of the first stream, both to 2e-5 of max |y|, the Winograd-against-direct bound of
tests/test_winograd.py.  alpha = 0.25: a range left uninitialised, or initialised and not added to, shows at the size
of y itself.  Not bit equality: split-K has no scratch on the 17th stream either, which changes a summation order.
Before the launcher initialised such an op's block itself, the 17th call returned an error (hipErrorInvalidValue from
launch_wgrad: "wgrad launch: invalid argument"); it was never a GPU fault.

*Setters* (in this process).  A setter takes effect at the next entry-point call: after lip_set_winograd(0) a product
launches no Winograd kernel, after lip_set_winograd(2) it does; lip_set_split_k likewise for the split-K kernels; the
three getters return what was set.
"""
import os
import subprocess
import sys

import pytest
import torch

from route_snapshot_child import N_STREAMS, bind, product

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WINO_BOUND = 2e-5       # tests/test_winograd.py: Winograd against direct, relative to max |y|
_CACHE = {}


def child(tmp_path_factory):
    if "child" not in _CACHE:
        out = tmp_path_factory.mktemp("route_snapshot") / "streams.pt"
        r = subprocess.run([sys.executable, os.path.join(HERE, "route_snapshot_child.py"), str(out)],
                           env=dict(os.environ, LIP_NOBINDCACHE="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"child failed ({r.returncode}): {r.stderr[-2000:]}"
        _CACHE["child"] = torch.load(out)
    return _CACHE["child"]


def toy():
    if "toy" not in _CACHE:
        _CACHE["toy"] = bind()
    return _CACHE["toy"]


def _wino(routes):
    return sorted(k for k in routes if k.startswith(("wgrad_wino", "igemm_wino")))


def _direct_wgrads(routes):
    return sorted(k for k in routes if k.startswith(("wgrad_pb<", "wgrad_fast<", "wgrad<")))


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()


def test_first_stream_takes_the_winograd_routes(tmp_path_factory):
    r = child(tmp_path_factory)
    assert r["routes"], r["error"]
    first = r["routes"][0]
    print("first stream:", first)
    assert any(k.startswith("wgrad_wino") for k in first) and any(k.startswith("igemm_wino") for k in first), first
    assert not _wino(r["routes_direct"]), r["routes_direct"]


def test_seventeenth_stream_succeeds_on_the_direct_kernels(tmp_path_factory):
    r = child(tmp_path_factory)
    assert r["error"] is None, r["error"]
    assert len(r["routes"]) == N_STREAMS
    last = r["routes"][-1]
    print("17th stream:", last)
    assert not _wino(last), last
    assert _direct_wgrads(last), last
    # the weight gradients take the launches they take with the route switched off
    assert _direct_wgrads(last) == _direct_wgrads(r["routes_direct"]), (last, r["routes_direct"])
    # ... and the 16th stream still had a record
    assert _wino(r["routes"][-2]), r["routes"][-2]


def test_seventeenth_stream_agrees_with_winograd_and_direct(tmp_path_factory):
    r = child(tmp_path_factory)
    assert r["error"] is None, r["error"]
    y = r["y_last"]
    assert torch.isfinite(y).all()
    e_wino, e_direct = _rel(y, r["y_first"]), _rel(y, r["y_direct"])
    print(f"17th stream vs first stream (Winograd): {e_wino:.3g}; vs first stream (direct): {e_direct:.3g}; bound {WINO_BOUND:g}")
    assert e_wino <= WINO_BOUND, e_wino
    assert e_direct <= WINO_BOUND, e_direct


def test_winograd_setter_holds_from_the_next_call():
    eng, V = toy()
    lib = eng.lib
    before = lib.lip_get_winograd()
    try:
        assert lib.lip_set_winograd(0) == 0
        y_off, off = product(eng, V)
        assert lib.lip_set_winograd(2) == 0
        y_on, on = product(eng, V)
    finally:
        lib.lip_set_winograd(before)
    print("off:", off, "\non:", on)
    assert not _wino(off), off
    assert any(k.startswith("wgrad_wino") for k in on) and any(k.startswith("igemm_wino") for k in on), on
    assert _rel(y_on, y_off) <= WINO_BOUND
    assert lib.lip_get_winograd() == before


def test_split_k_setter_holds_from_the_next_call():
    eng, V = toy()
    lib = eng.lib
    try:
        assert lib.lip_set_split_k(0) == 0
        _, off = product(eng, V)
        assert lib.lip_set_split_k(1) == 0
        _, on = product(eng, V)
    finally:
        lib.lip_set_split_k(1)          # (the default; the mode has no getter)
    print("off:", off, "\non:", on)
    assert not [k for k in off if "/ks" in k], off
    assert [k for k in on if "/ks" in k], on


def test_getters_return_what_was_set():
    from lip_amd import _native as nv
    lib = nv.load()
    modes = (("winograd", lib.lip_set_winograd, lib.lip_get_winograd, (0, 1, 2)),
             ("precision", lib.lip_set_precision, lib.lip_get_precision, (1, 0)),
             ("wino_walk", lib.lip_set_wino_walk, lib.lip_get_wino_walk, (1, 2, 4, 0)))
    for name, setter, getter, values in modes:
        before = getter()
        try:
            for v in values:
                assert setter(v) == 0, (name, v)
                assert getter() == v, (name, v, getter())
            assert setter(7) != 0 and getter() == values[-1], name      # a refused value changes nothing
        finally:
            setter(before)
        assert getter() == before, name
