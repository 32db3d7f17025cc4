"""CPU: the float64 reference of tests/test_kernel_routes.py, checked independently of the GPU.

* For every geometry of the case table, the tape emulator's IGEMM (mode 0: conv2d, mode 1: conv_transpose2d) and
  WGRAD (the weight-gradient formula) agree with torch.nn.functional in float64 — this pins the reference independently
  of the emulator's own index loops.
* The harness's checks catch what they are there to catch: a changed canary, an input overwritten, an output element
  off by more than the bound, an unwritten output, a WGRAD result that drops the accumulation prefill.
"""
import dataclasses

import pytest
import torch
import torch.nn.functional as Fn

from lip_amd import _native as nv
import op_harness as oh
from kernel_route_cases import CASES

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
            dw = torch.nn.grad.conv2d_weight(a, (N, sg.C, sg.KH, sg.KW), g, stride=sg.stride, padding=sg.pad)
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
                want[p] += Fn.conv2d(x, w, stride=sg.stride, padding=sg.pad)
            else:
                oph = OH - ((sg.IH - 1) * sg.stride - 2 * sg.pad + sg.KH)
                opw = OW - ((sg.IW - 1) * sg.stride - 2 * sg.pad + sg.KW)
                want[p] += Fn.conv_transpose2d(x, w.transpose(0, 1), stride=sg.stride, padding=sg.pad,
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
