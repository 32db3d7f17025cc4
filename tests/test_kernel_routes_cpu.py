"""CPU: the float64 reference of tests/test_kernel_routes.py, checked independently of the GPU.

* For every geometry of the case table, the tape emulator's IGEMM (mode 0: conv2d, mode 1: conv_transpose2d) and
  WGRAD (the weight-gradient formula) agree with torch.nn.functional in float64 — this pins the reference independently
  of the emulator's own index loops.
* The harness's checks catch what they are there to catch: a changed canary, an input overwritten, an output element
  off by more than the bound, an unwritten output, a WGRAD result that drops the accumulation prefill.
* The anisotropic rows ("an_...") can tell the two axes apart: the float64 result of the op with IH / IW, KH / KW,
  pad_h / pad_w and OH / OW exchanged, handed to check() as the device output, fails it for every one of them; and every
  route of the table has such a row.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as Fn

from lip_amd import _native as nv
import op_harness as oh
from kernel_route_cases import AN_CASES, CASES

F64 = torch.float64


class _Eng:
    pass


@pytest.fixture(scope="module")
def cpu_harness():
    """the harness's layout and emulator on CPU buffers of the same sizes as the GPU engine's"""
    from lip_amd.engine import build_consts, compile_net
    from lip_amd.netspec import NetSpec
    from lip_amd.toymodels import create_state
    net = NetSpec((8, 8, 16))
    x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, bn="BatchNorm_0", act="relu")
    x = net.conv(x, "Conv_1", 32, 3, 1, padding=1, bn="BatchNorm_1", act="relu")
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 10)
    net.model_type = "classifier"
    state = create_state(net, 0, dtype=F64)
    cn = compile_net(net, 4, state.params)
    h = oh.Harness.__new__(oh.Harness)
    h.chunk = 256
    h.eng = _Eng()
    h.eng.cn = cn
    h.eng.work = torch.zeros(cn.work_pp * h.chunk)
    h.eng.prim = torch.zeros(cn.prim_floats)
    h.eng.consts = torch.zeros(build_consts(cn, state.params, state.batch_stats, "cpu", F64).numel())
    return h


def _region(buf, base, count, ps, p):
    return buf[base + p * ps: base + p * ps + count]


def _small(spec):
    """the case's geometry without epilogue fields, at most 2 probes"""
    return dataclasses.replace(spec, P=min(spec.P, 2), epi={}, out_space="Y", out_shift=0,
                               segs=[dataclasses.replace(s, a_space="V", b_space="V") for s in spec.segs])


def _bases(L, space):
    return L.regions[space]


GEOMS = {}
for _c in CASES:
    GEOMS.setdefault(repr(_small(_c.spec)), _c)


@pytest.mark.parametrize("case", list(GEOMS.values()), ids=[c.name for c in GEOMS.values()])
def test_emulator_matches_torch(cpu_harness, case):
    h = cpu_harness
    spec = _small(case.spec)
    op, L, host, outs = h.build(spec, seed=1)
    P = spec.P
    got = oh.emulate(h.eng.cn, h.chunk, op, host, P)
    regs = _bases(L, "V")
    _, sp, obase, ocount, ops, Po, pre = outs[0]
    n, OH, OW, N = spec.n_img, spec.OH, spec.OW, spec.N
    if spec.kind == nv.OP_WGRAD:
        sg = spec.segs[0]
        abase, acount, _, _ = regs[0]
        gbase, gcount, gps, _ = regs[1]
        a = host["V"][abase:abase + acount].double().reshape(n, sg.IH, sg.IW, sg.C).permute(0, 3, 1, 2)
        for p in range(P):
            g = _region(host["V"], gbase, gcount, gps, p).double().reshape(n, OH, OW, N).permute(0, 3, 1, 2)
            dw = torch.nn.grad.conv2d_weight(a, (N, sg.C, sg.KH, sg.KW), g, stride=sg.stride, padding=(sg.pad, sg.pad_w))
            want = dw.permute(2, 3, 1, 0).reshape(-1) + _region(host["Y"], obase, ocount, ops, p).double()
            torch.testing.assert_close(_region(got["Y"], obase, ocount, ops, p), want, rtol=1e-12, atol=1e-12)
        return
    want = torch.zeros(P, n, N, OH, OW, dtype=F64)
    for s, sg in enumerate(spec.segs):
        abase, acount, aps, Pa = regs[2 * s]
        bbase, bcount, bps, Pb = regs[2 * s + 1]
        for p in range(P):
            a = _region(host["V"], abase, acount, aps, p if Pa > 1 else 0).double().reshape(n, sg.IH, sg.IW, sg.C)
            b = _region(host["V"], bbase, bcount, bps, p if Pb > 1 else 0).double()
            if sg.b_trans:            # B[(tap*C + c)][n] = b[(tap*N + n)*C + c]
                w = b.reshape(sg.KH, sg.KW, N, sg.C).permute(2, 3, 0, 1)
            else:                     # B[(tap*C + c)][n] = b[(tap*C + c)*N + n]
                w = b.reshape(sg.KH, sg.KW, sg.C, N).permute(3, 2, 0, 1)
            x = a.permute(0, 3, 1, 2)
            if sg.mode == 0:
                want[p] += Fn.conv2d(x, w, stride=sg.stride, padding=(sg.pad, sg.pad_w))
            else:
                oph = OH - ((sg.IH - 1) * sg.stride - 2 * sg.pad + sg.KH)
                opw = OW - ((sg.IW - 1) * sg.stride - 2 * sg.pad_w + sg.KW)
                assert 0 <= oph < max(sg.stride, 2) and 0 <= opw < max(sg.stride, 2), (oph, opw)
                want[p] += Fn.conv_transpose2d(x, w.transpose(0, 1), stride=sg.stride, padding=(sg.pad, sg.pad_w),
                                               output_padding=(oph, opw))
    for p in range(P):
        torch.testing.assert_close(_region(got["Y"], obase, ocount, ops, p),
                                   want[p].permute(0, 2, 3, 1).reshape(-1), rtol=1e-12, atol=1e-12)


def _rounded(h, spec, seed=2):
    """a 'kernel' that returns the float64 reference rounded to f32: it must pass every check"""
    op, L, host, outs = h.build(spec, seed)
    ref = oh.emulate(h.eng.cn, h.chunk, op, host, spec.P)
    mag = oh.emulate(h.eng.cn, h.chunk, op, host, spec.P, absolute=True)
    got = {k: host[k].clone() for k in host}
    m = oh.output_mask(host, outs)
    for k in got:
        got[k][m[k]] = ref[k][m[k]].float()
    return op, L, host, outs, ref, mag, got


def _k(kt):
    return lambda name: (kt + 16, kt)


def test_harness_checks_catch_faults(cpu_harness):
    from kernel_route_cases import BY_NAME
    h = cpu_harness
    spec = BY_NAME["fast_all_epi"].spec
    kt = spec.segs[0].Ktot
    op, L, host, outs, ref, mag, got = _rounded(h, spec)
    oh.check(got, ref, mag, host, outs, _k(kt), 1.0, "rounded reference")
    name, sp, base, count, ps, Pn, pre = outs[0]
    # an output element off by more than (Ktot + 16) 2^-24 Mag
    bad = {k: v.clone() for k, v in got.items()}
    i = base + ps + count // 2
    bad[sp][i] = float(bad[sp][i].double() + (kt + 20) * oh.U24 * mag[sp][i])
    with pytest.raises(AssertionError, match="above"):
        oh.check(bad, ref, mag, host, outs, _k(kt), 1.0, "off by one bound")
    # an output element never written (still the canary)
    bad = {k: v.clone() for k, v in got.items()}
    bad[sp].view(torch.int32)[base + 3] = oh.CANARY
    with pytest.raises(AssertionError, match="not written"):
        oh.check(bad, ref, mag, host, outs, _k(kt), 1.0, "unwritten")
    # a canary float in a guard zone just past the last output, and an input, overwritten
    for space, idx in ((sp, base + (Pn - 1) * ps + count), (sp, base + count), ("V", L.regions["V"][0][0])):
        bad = {k: v.clone() for k, v in got.items()}
        bad[space][idx] = 0.0
        with pytest.raises(AssertionError, match="outside the outputs changed"):
            oh.check(bad, ref, mag, host, outs, _k(kt), 1.0, "canary")
    # a small systematic error (every output scaled by 1 + 2^-12) passes no RMS bound of the exact routes
    bad = {k: v.clone() for k, v in got.items()}
    m = oh.output_mask(host, outs)[sp]
    bad[sp][m] = (bad[sp][m].double() * (1 + 2.0 ** -12)).float()
    with pytest.raises(AssertionError):
        oh.check(bad, ref, mag, host, outs, _k(kt), 1.0, "scaled")


def test_harness_wgrad_accumulates(cpu_harness):
    from kernel_route_cases import BY_NAME
    h = cpu_harness
    spec = BY_NAME["wg_4112_v4"].spec
    op, L, host, outs, ref, mag, got = _rounded(h, spec)
    R = spec.R
    oh.check(got, ref, mag, host, outs, _k(R), 1.0, "rounded reference")
    name, sp, base, count, ps, Pn, pre = outs[0]
    assert pre
    prefill = host[sp][base:base + count].double()
    assert prefill.abs().min() > 0
    # a kernel that overwrites instead of adding fails
    bad = {k: v.clone() for k, v in got.items()}
    bad[sp][base:base + count] = (ref[sp][base:base + count] - prefill).float()
    with pytest.raises(AssertionError, match="above"):
        oh.check(bad, ref, mag, host, outs, _k(R), 1.0, "overwrite")


# ---------------------------------------------------------------------------------------------- the two axes
# rows whose op has no axes to exchange: a skinny weight gradient needs KH = IH, KW = IW and ONE output pixel, so its
# im2col is the identity on the flattened map whichever way the map is cut into rows.  They are in the table for the
# dispatcher's KH == IH && KW == IW test on a non-square map; the swap test asserts that their result does NOT change.
AXIS_FREE = {c.name for c in AN_CASES if c.route.startswith("wgrad_skinny")}


def swap_axes(op):
    """the op descriptor with the two map axes exchanged; every element count stays"""
    import copy
    q = copy.copy(op)
    q.OH, q.OW = op.OW, op.OH
    for s in range(max(op.nseg, 1)):
        a, b = q.seg[s], op.seg[s]
        a.IH, a.IW, a.KH, a.KW, a.pad_h, a.pad_w = b.IW, b.IH, b.KW, b.KH, b.pad_w, b.pad_h
    return q


@pytest.mark.parametrize("case", AN_CASES, ids=[c.name for c in AN_CASES])
def test_axis_swap_fails_the_check(cpu_harness, case):
    """a kernel that mixes up the two axes everywhere cannot pass an anisotropic row (probes cut to 2: the bound does
    not depend on them)"""
    import test_kernel_routes as T
    h = cpu_harness
    sg = case.spec.segs[0]
    assert case.spec.n_img >= 2 and sg.IH != sg.IW, "an anisotropic row needs two images and IH != IW"
    case = dataclasses.replace(case, spec=dataclasses.replace(case.spec, P=min(case.spec.P, 2)))
    op, L, host, outs, ref, mag, got = _rounded(h, case.spec, seed=0)
    k_of, rms_c = T.tolerances(case)
    oh.check(got, ref, mag, host, outs, k_of, rms_c, case.name)                 # the rounded reference passes
    swapped = oh.emulate(h.eng.cn, h.chunk, swap_axes(op), host, case.spec.P)
    m = oh.output_mask(host, outs)
    bad = {k: host[k].clone() for k in host}
    for k in bad:
        bad[k][m[k]] = swapped[k][m[k]].float()
    if case.name in AXIS_FREE:
        for k in bad:
            assert torch.equal(swapped[k][m[k]], ref[k][m[k]]), f"{case.name} is listed as axis-free but the swap changes it"
        return
    with pytest.raises(AssertionError):
        oh.check(bad, ref, mag, host, outs, k_of, rms_c, case.name + " (axes exchanged)")


def _map_geometry(route):
    return route.startswith(("igemm", "wgrad"))


def test_every_map_route_has_an_anisotropic_row():
    """over the committed table: every route that takes a map geometry has a row with IH != IW (the A/B-only routes have
    no row at all: test_kernel_routes.AB_ONLY), and the table holds the shapes where the axes differ in kind"""
    routes = {c.route for c in CASES if _map_geometry(c.route)}
    assert len(routes) >= 80
    an = {c.route for c in CASES if c.spec.segs[0].IH != c.spec.segs[0].IW and c.spec.n_img >= 2}
    assert not (routes - an), f"routes without an anisotropic row: {sorted(routes - an)}"
    segs = [(c, c.spec.segs[0]) for c in AN_CASES]
    assert any(g.KH != g.KW for _, g in segs)
    assert any(g.pad != g.pad_w for _, g in segs)
    assert any(g.KH == 3 and g.KW == 3 and (g.pad, g.pad_w) == (0, 1) for _, g in segs)
    assert any(g.KH == 3 and g.KW == 3 and (g.pad, g.pad_w) == (1, 0) for _, g in segs)
    t2 = [c.spec for c, g in segs if g.mode == 1 and g.stride == 2]
    assert any(s.OH % 2 == 0 and s.OW % 2 == 1 for s in t2), "no (even, odd) output of a stride-2 transposed conv"
    assert any(s.OH % 2 == 1 and s.OW % 2 == 0 for s in t2), "no (odd, even) output of a stride-2 transposed conv"
    assert any(s.OH % 2 == 0 and s.OW % 2 == 0 and s.OH != s.OW for s in t2)
    assert any(g.mode == 0 and g.stride == 2 and g.IH % 2 == 0 and g.IW % 2 == 1 for _, g in segs)
    assert not any(g.KH == 1 and g.KW == 1 for c, g in segs if c.name not in AXIS_FREE)
