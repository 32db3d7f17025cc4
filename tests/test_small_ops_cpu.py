"""CPU: the float64 reference of tests/test_small_ops.py, checked independently of the GPU.

* For the geometries of the case table (probes cut to 2) the tape emulator's non-GEMM ops agree in float64 with
  torch.nn.functional / autograd: mean pool and its VJP, window average (padding counted) and max pool with their VJPs,
  the first-maximum argmax rule, softmax, the head modes against the dense c (diag p - p p^T), c L^T, c L, activations
  and their derivatives, the column sums.
* The float64 reference alone keeps ReLU's skipped elements within the cap the GPU test allows.
* The harness's checks bite: a flipped argmax, a dropped red1, an output one bound off, an unwritten tail element.
* The anisotropic window-pool rows ("an_...") can tell the two axes apart: the float64 result with IH / IW, KH / KW,
  pad_h / pad_w and OH / OW exchanged fails check() for every one of them, and every window-pool label has such a row.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as Fn

from lip_amd import _native as nv
import op_harness as oh
from small_op_cases import BY_NAME, CASES, first_argmax
from small_op_harness import build_small, region
from test_kernel_routes_cpu import cpu_harness  # noqa: F401  (fixture)

F64 = torch.float64
LIVE = [c for c in CASES if not c.refuse]


def _cut(case):
    """the case with at most 2 probes"""
    return dataclasses.replace(case, spec=dataclasses.replace(case.spec, P=min(case.spec.P, 2)))


def _io(h, case, seed=1):
    spec = case.spec
    op, L, host, outs = build_small(h, spec, seed)
    ref = h.emulate(op, host, spec.P, head_mode=spec.head_mode, head_c=spec.head_c)
    return op, L, host, outs, ref


def _in(host, L, spec, name):
    """float64 (probes, count) values of the input reference `name`"""
    sp = spec.refs[name].space
    i = [n for n, r in spec.refs.items() if r.role in ("in", "idle") and r.space == sp].index(name)
    return region(host[sp], L.regions[sp][i]).double()


def _o(outs, name):
    return next(t for t in outs if t[0] == name)


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)


def _reds(spec, host, L, outs, ref, v):
    """red0 / red1 of a (P, R, N) cotangent v: prefill + column sums"""
    N = spec.N
    for name in ("red0", "red1"):
        if name not in spec.refs:
            continue
        o = _o(outs, name)
        w = v if name == "red0" else v * _in(host, L, spec, "xhat2").reshape(1, -1, N)
        _close(region(ref[o[1]], o), region(host[o[1]], o).double() + w.sum(1))


def _small_enough(case):
    return sum(r.count for r in case.spec.refs.values()) * min(case.spec.P, 2) < 3_000_000


@pytest.mark.parametrize("case", [c for c in LIVE if _small_enough(c)], ids=lambda c: c.name)
def test_emulator_matches_torch(cpu_harness, case):  # noqa: F811
    h = cpu_harness
    case = _cut(case)
    spec = case.spec
    op, L, host, outs, ref = _io(h, case)
    P, n, N, kind = spec.P, spec.n_img, spec.N, spec.kind
    if kind == nv.OP_REDUCE:
        _reds(spec, host, L, outs, ref, _in(host, L, spec, "a").reshape(P, -1, N))
    elif kind == nv.OP_POOL_FWD:
        x = _in(host, L, spec, "a").reshape(P, n, spec.OH, N)
        o = _o(outs, "out")
        _close(region(ref[o[1]], o), x.mean(2).reshape(P, -1))
    elif kind == nv.OP_POOL_BWD:
        g = _in(host, L, spec, "a").reshape(P, n, N)
        x = torch.zeros(P, n, spec.OH, N, dtype=F64, requires_grad=True)
        v, = torch.autograd.grad(x.mean(2), x, g)
        if "dphi" in spec.refs:
            v = v * _in(host, L, spec, "dphi").reshape(1, n, spec.OH, N)
        o = _o(outs, "out")
        _close(region(ref[o[1]], o), v.reshape(P, -1))
        _reds(spec, host, L, outs, ref, v.reshape(P, -1, N))
    elif kind in (nv.OP_MAXPOOL_PRIMAL, nv.OP_MAXPOOL_FWD, nv.OP_MAXPOOL_BWD):
        _window_pool(spec, host, L, outs, ref)
    elif kind == nv.OP_PRIMAL_POST:
        _primal_post(spec, host, L, outs, ref)
    elif kind == nv.OP_SOFTMAX:
        f = _in(host, L, spec, "a").reshape(n, N)
        o, o2 = _o(outs, "out"), _o(outs, "out2")
        _close(region(ref[o[1]], o).reshape(n, N), Fn.softmax(f, -1))
        _close(region(ref[o2[1]], o2).reshape(n, N), Fn.softmax(f, -1).sqrt())
    elif kind == nv.OP_HEAD:
        _head(spec, host, L, outs, ref)
    else:
        raise AssertionError(kind)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _window_pool(spec, host, L, outs, ref):
    P, n, C, s = spec.P, spec.n_img, spec.N, spec.stride
    IH, IW, OH, OW, k, pad = spec.IH, spec.IW, spec.OH, spec.OW, (spec.KH, spec.KW), (spec.pad, spec.pad_w)
    avg = "aux0" not in spec.refs
    o = _o(outs, "out")
    got = region(ref[o[1]], o)

    def pool(x):                                     # (B, IH, IW, C) -> (B, OH, OW, C)
        x = _nchw(x)
        y = Fn.avg_pool2d(x, k, s, pad, count_include_pad=True) if avg else Fn.max_pool2d(x, k, s, pad)
        assert y.shape[2:] == (OH, OW)
        return y.permute(0, 2, 3, 1)

    if spec.kind == nv.OP_MAXPOOL_PRIMAL:
        x = _in(host, L, spec, "a").reshape(n, IH, IW, C)
        _close(got.reshape(n, OH, OW, C), pool(x))
        if avg:
            return
        oa = _o(outs, "aux0")
        am = region(ref[oa[1]], oa).reshape(n, OH, OW, C)
        best, arg = first_argmax(x, k, s, pad)
        assert torch.equal(am, arg), "argmax: not the first maximum in (kh, kw) order"
        # the cached pixel lies in the window and holds the maximum
        ih, iw = (am // IW).long(), (am % IW).long()
        oh_ = torch.arange(OH).reshape(1, OH, 1, 1)
        ow_ = torch.arange(OW).reshape(1, 1, OW, 1)
        assert ((ih >= oh_ * s - pad[0]) & (ih < oh_ * s - pad[0] + k[0]) & (iw >= ow_ * s - pad[1]) & (iw < ow_ * s - pad[1] + k[1])).all()
        val = torch.gather(x.reshape(n, IH * IW, C), 1, am.long().reshape(n, OH * OW, C)).reshape(n, OH, OW, C)
        assert torch.equal(val, got.reshape(n, OH, OW, C))
        return
    if avg:
        if spec.kind == nv.OP_MAXPOOL_FWD:
            x = _in(host, L, spec, "a").reshape(P * n, IH, IW, C)
            _close(got.reshape(P * n, OH, OW, C), pool(x))
            return
        g = _in(host, L, spec, "a").reshape(P * n, OH, OW, C)
        x = torch.zeros(P * n, IH, IW, C, dtype=F64, requires_grad=True)
        v, = torch.autograd.grad(pool(x), x, g)
    else:
        am = _in(host, L, spec, "aux0").reshape(n, OH * OW, C).long()
        if spec.kind == nv.OP_MAXPOOL_FWD:
            x = _in(host, L, spec, "a").reshape(P, n, IH * IW, C)
            _close(got.reshape(P, n, OH * OW, C), torch.gather(x, 2, am[None].expand(P, -1, -1, -1)))
            return
        # VJP of the gather y = x[argmax]: by autograd
        g = _in(host, L, spec, "a").reshape(P, n, OH * OW, C)
        x = torch.zeros(P, n, IH * IW, C, dtype=F64, requires_grad=True)
        v, = torch.autograd.grad(torch.gather(x, 2, am[None].expand(P, -1, -1, -1)), x, g)
    v = v.reshape(P, n * IH * IW, C)
    if "dphi" in spec.refs:
        v = v * _in(host, L, spec, "dphi").reshape(1, -1, C)
    _close(got, v.reshape(P, -1))
    _reds(spec, host, L, outs, ref, v)


def _primal_post(spec, host, L, outs, ref):
    R, N = spec.R, spec.N
    y = _in(host, L, spec, "a").reshape(R, N)
    if "e0" in spec.refs:
        y = y + _in(host, L, spec, "e0")
    if "e1" in spec.refs:
        xh = (y - _in(host, L, spec, "aux0")) * _in(host, L, spec, "aux1")
        o3 = _o(outs, "out3")
        _close(region(ref[o3[1]], o3).reshape(R, N), xh)
        y = xh * _in(host, L, spec, "e1") + _in(host, L, spec, "scale")
    if "res" in spec.refs:
        y = y + _in(host, L, spec, "res").reshape(R, N)
    y = y.clone().requires_grad_(True)
    a = (y, Fn.relu(y), torch.tanh(y), Fn.gelu(y, approximate="tanh"))[spec.act]
    d, = torch.autograd.grad(a.sum(), y) if spec.act else (torch.ones_like(y),)
    o = _o(outs, "out")
    _close(region(ref[o[1]], o).reshape(R, N), a.detach())
    if "out2" in spec.refs:
        o2 = _o(outs, "out2")
        _close(region(ref[o2[1]], o2).reshape(R, N), d)


def _head(spec, host, L, outs, ref):
    P, n, K, c = spec.P, spec.n_img, spec.N, spec.head_c
    mode = spec.head_mode
    rin = "a" if mode in (nv.HEAD_GGN, nv.HEAD_LT, nv.HEAD_OUT) else "out2"
    rout = "out" if mode in (nv.HEAD_GGN, nv.HEAD_L, nv.HEAD_IN) else "out2"
    u = _in(host, L, spec, rin).reshape(P, n, K)
    o = _o(outs, rout)
    got = region(ref[o[1]], o).reshape(P, n, K)
    if not spec.classifier or mode in (nv.HEAD_OUT, nv.HEAD_IN):
        _close(got, c * u)
        return
    p = _in(host, L, spec, "aux0").reshape(n, K)
    s = _in(host, L, spec, "aux1").reshape(n, K)
    for i in range(n):
        Lm = torch.diag(s[i]) - torch.outer(p[i], s[i])              # L = diag(s) - p s^T
        M = {nv.HEAD_GGN: c * (torch.diag(p[i]) - torch.outer(p[i], p[i])), nv.HEAD_LT: c * Lm.T, nv.HEAD_L: c * Lm}[mode]
        _close(got[:, i], u[:, i] @ M.T)


# ---------------------------------------------------------------------------------------------- ReLU skip cap
@pytest.mark.parametrize("case", [c for c in LIVE if c.relu_skip], ids=lambda c: c.name)
def test_relu_skip_cap_holds_for_the_reference(cpu_harness, case):  # noqa: F811
    """the seed of the GPU test (0): the float64 reference alone skips at most 1e-4 of the elements and at most 16"""
    import test_small_ops as T
    h = cpu_harness
    op, L, host, outs = build_small(h, case.spec, 0)
    mag = h.emulate(op, host, 1, absolute=True)
    skip = T.relu_skip_mask(h, case, op, host, outs, mag)["out2"]     # asserts the cap
    assert int(skip.sum()) <= min(T.RELU_SKIP_MAX, T.RELU_SKIP_SHARE * skip.numel())


# ---------------------------------------------------------------------------------------------- the checks bite
def _rounded(h, case, seed=2):
    spec = case.spec
    op, L, host, outs = build_small(h, spec, seed)
    ref = h.emulate(op, host, spec.P, head_mode=spec.head_mode, head_c=spec.head_c)
    mag = h.emulate(op, host, spec.P, absolute=True, head_mode=spec.head_mode, head_c=spec.head_c)
    got = {k: host[k].clone() for k in host}
    m = oh.output_mask(host, outs)
    for k in got:
        got[k][m[k]] = ref[k][m[k]].float()
    return op, L, host, outs, ref, mag, got


def _check(case, got, ref, mag, host, outs):
    import test_small_ops as T
    exact = {n for n, t in case.tol.items() if t == "exact"}
    return oh.check(got, ref, mag, host, outs, T.k_of_case(case), 1.0, case.name, exact=exact)


def test_rounded_reference_passes_every_case(cpu_harness):  # noqa: F811
    for case in LIVE:
        if not _small_enough(case) or case.relu_skip:
            continue
        op, L, host, outs, ref, mag, got = _rounded(cpu_harness, _cut(case))
        _check(case, got, ref, mag, host, outs)


def test_checks_catch_a_flipped_argmax(cpu_harness):  # noqa: F811
    case = BY_NAME["mpp_C64_I16_w321_const"]          # a constant map: every window is a tie
    op, L, host, outs, ref, mag, got = _rounded(cpu_harness, case)
    _check(case, got, ref, mag, host, outs)
    o = _o(outs, "aux0")
    spec = case.spec
    i = o[2] + ((1 * spec.OW + 1) * spec.N + 5)       # window (1, 1): interior, nine equal candidates
    first = got[o[1]][i].item()
    bad = {k: v.clone() for k, v in got.items()}
    bad[o[1]][i] = first + 1.0                        # the NEXT pixel of the window holds the same maximum
    with pytest.raises(AssertionError, match="differ bitwise"):
        _check(case, bad, ref, mag, host, outs)


def test_checks_catch_a_dropped_red1(cpu_harness):  # noqa: F811
    case = _cut(BY_NAME["pb_C12_HW49"])
    op, L, host, outs, ref, mag, got = _rounded(cpu_harness, case)
    _check(case, got, ref, mag, host, outs)
    o = _o(outs, "red1")
    bad = {k: v.clone() for k, v in got.items()}
    for p in range(o[5]):                             # red1 left at its prefill
        bad[o[1]][o[2] + p * o[4]: o[2] + p * o[4] + o[3]] = host[o[1]][o[2] + p * o[4]: o[2] + p * o[4] + o[3]]
    with pytest.raises(AssertionError, match="red1"):
        _check(case, bad, ref, mag, host, outs)


@pytest.mark.parametrize("name,out", [("red_N1028_R100", "red0"), ("pf_C512_HW49", "out"), ("pb_C512_HW49", "out"),
                                      ("mpb_C64_I16_const", "out"), ("head_ggn_cls_K1000", "out"), ("pp_none_bn_N64", "out3")])
def test_checks_catch_one_bound_off_and_an_unwritten_tail(cpu_harness, name, out):  # noqa: F811
    case = _cut(BY_NAME[name])
    op, L, host, outs, ref, mag, got = _rounded(cpu_harness, case)
    _check(case, got, ref, mag, host, outs)
    o = _o(outs, out)
    k = case.tol[out][0]
    last = o[2] + (o[5] - 1) * o[4] + o[3] - 1        # the last element of the last probe
    bad = {k_: v.clone() for k_, v in got.items()}
    first = last - o[3] + 1
    i = first + int(torch.argmax(mag[o[1]][first:last + 1]))          # (the tail itself may have Mag 0: a masked pixel)
    m = mag[o[1]][i].item()
    assert m > 0
    bad[o[1]][i] = float(ref[o[1]][i] + (k + 2) * oh.U24 * m)
    with pytest.raises(AssertionError, match="above"):
        _check(case, bad, ref, mag, host, outs)
    bad = {k_: v.clone() for k_, v in got.items()}
    bad[o[1]].view(torch.int32)[last] = oh.CANARY
    with pytest.raises(AssertionError, match="not written"):
        _check(case, bad, ref, mag, host, outs)


# ---------------------------------------------------------------------------------------------- the two axes
AN_CASES = [c for c in CASES if c.name.startswith("an_")]


@pytest.mark.parametrize("case", AN_CASES, ids=lambda c: c.name)
def test_axis_swap_fails_the_check(cpu_harness, case):  # noqa: F811
    """the op emulated with the two axes exchanged in its descriptor, on the same buffers, is not accepted as the device
    output.  A max pool's tangent and cotangent passes read the geometry only through the argmax that the primal pass
    cached, so for them the exchanged run reads the argmax an exchanged primal pass caches from the same map."""
    from test_kernel_routes_cpu import swap_axes
    h = cpu_harness
    spec = case.spec
    assert spec.n_img >= 2 and spec.IH != spec.IW
    op, L, host, outs, ref, mag, got = _rounded(h, case, seed=0)
    _check(case, got, ref, mag, host, outs)                                    # the rounded reference passes
    shost = host
    if spec.kind != nv.OP_MAXPOOL_PRIMAL and "aux0" in spec.refs:
        shost = {k: v.clone() for k, v in host.items()}
        i = [n for n, r in spec.refs.items() if r.role in ("in", "idle") and r.space == "V"].index("aux0")
        base, count, _, _ = L.regions["V"][i]
        am = spec.refs["aux0"].data.swapped().reshape(-1).float()
        assert not torch.equal(am, shost["V"][base:base + count])
        shost["V"][base:base + count] = am
    swapped = h.emulate(swap_axes(op), shost, spec.P)
    m = oh.output_mask(host, outs)
    bad = {k: host[k].clone() for k in host}
    for k in bad:
        bad[k][m[k]] = swapped[k][m[k]].float()
    with pytest.raises(AssertionError):
        _check(case, bad, ref, mag, host, outs)


def test_every_window_pool_label_has_an_anisotropic_row():
    labels = {c.route for c in CASES if c.route.startswith("maxpool_")}
    assert len(labels) == 8, sorted(labels)
    an = {c.route for c in AN_CASES}
    assert an == labels, sorted(labels - an)
    specs = [c.spec for c in AN_CASES]
    assert all(s.n_img >= 2 and s.IH != s.IW and s.KH != s.KW and s.pad != s.pad_w for s in specs)
    assert {(s.KH, s.KW, s.pad, s.pad_w) for s in specs} == {(3, 2, 1, 0), (2, 3, 0, 1)}
    assert any(s.stride == 2 and s.IH % 2 == 1 and s.IW % 2 == 0 for s in specs)
    assert any(c.name.endswith("const") for c in AN_CASES), "no tie map"
