"""Specs, layout and Mag of the non-GEMM engine ops for tests/op_harness.py — TEST INFRASTRUCTURE (a plain helper module).

A ``SmallSpec`` names the operand references one op of ``include/lip.h`` uses (``"a"`` is ``seg[0].a``, the rest are the
field names of ``lip_op_t``) and, per reference, where it lives, how it is aligned and what it holds.  ``build_small``
lays it out with ``op_harness.Layout`` and returns the same tuple as ``Harness.build``, so running, emulating and
checking are the harness's own.

``MagMachine`` gives the magnitude ``Mag`` for the ops where the emulator on absolute values is not one: differences
are taken as sums (HEAD, BatchNorm), and the non-linear outputs get the magnitude of the terms they are formed from.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Union

import torch

from lip_amd import _native as nv
from op_harness import F64, Layout, _ref
from tape_emulator import TapeMachine

FLT_MIN = 2.0 ** -126


@dataclass
class RefSpec:
    count: int
    pp: bool = False                  # one region per probe (else shared: probe stride 0)
    space: str = "V"
    shift: int = 0                    # floats added to the offset (0: 16-byte aligned)
    odd: bool = False                 # odd probe stride: the alignment changes from probe to probe
    role: str = "in"                  # "in" | "out" (written) | "acc" (random prefill, the op adds) | "idle" (a reference
                                      # the op must neither read nor write: it stays canary)
    data: Union[None, float, torch.Tensor, Callable] = None   # None: randn; float: randn * it; tensor (probes, count);
                                                              # callable(generator) -> such a tensor


@dataclass
class SmallSpec:
    kind: int
    P: int
    n_img: int
    OH: int
    OW: int
    N: int
    refs: Dict[str, RefSpec] = field(default_factory=dict)
    IH: int = 0
    IW: int = 0
    KH: int = 0
    KW: int = 0
    stride: int = 0
    pad: int = 0
    pad_w: int = None                 # padding of the W axis (None: pad)
    act: int = 0
    classifier: int = 0
    fscale: float = 0.0
    head_mode: int = 0
    head_c: float = 1.0

    def __post_init__(self):
        if self.pad_w is None:
            self.pad_w = self.pad

    @property
    def R(self):
        return self.n_img * self.OH * self.OW


def build_small(h, spec: SmallSpec, seed=0):
    """lay the op out; returns (op, layout, host buffers, outputs) as op_harness.Harness.build does."""
    g = torch.Generator().manual_seed(seed)
    L = Layout(h.chunk)
    op = nv.Op()
    op.kind, op.nseg = spec.kind, 1
    op.n_img, op.OH, op.OW, op.N = spec.n_img, spec.OH, spec.OW, spec.N
    op.act, op.classifier, op.fscale = spec.act, spec.classifier, spec.fscale
    for f in nv.REF_FIELDS:
        setattr(op, f, _ref(None))
    seg = op.seg[0]
    seg.a = _ref(None)
    seg.b = _ref(None)
    seg.IH, seg.IW, seg.C, seg.KH, seg.KW = spec.IH, spec.IW, spec.N, spec.KH, spec.KW
    seg.stride, seg.pad_h, seg.pad_w = spec.stride, spec.pad, spec.pad_w
    fills, outs = [], []
    for name, r in spec.refs.items():
        Pn = spec.P if r.pp else 1
        ps = None
        if r.odd:
            ps = r.count + 1 if (r.count + 1) % 2 else r.count + 2
        off, ps, base = L.alloc(r.space, r.count, Pn, ps, shift=r.shift, output=r.role in ("out", "acc"))
        if not r.pp:
            ps = 0
        ref = _ref(r.space, off, ps)
        if name == "a":
            seg.a = ref
        else:
            setattr(op, name, ref)
        if r.role == "in":
            fills.append((r, r.space, base, r.count, ps, Pn))
        elif r.role != "idle":
            outs.append((name, r.space, base, r.count, ps, Pn, r.role == "acc"))
    host = h.buffers(L)
    for r, sp, base, count, ps, Pn in fills:
        if callable(r.data):
            v = r.data(g)
        elif isinstance(r.data, torch.Tensor):
            v = r.data
        else:
            v = torch.randn(Pn, count, generator=g, dtype=F64) * (1.0 if r.data is None else r.data)
        v = v.reshape(Pn, count).float()
        for p in range(Pn):
            host[sp][base + p * ps: base + p * ps + count] = v[p]
    for name, sp, base, count, ps, Pn, pre in outs:
        if pre:
            for p in range(Pn):
                host[sp][base + p * ps: base + p * ps + count] = torch.randn(count, generator=g, dtype=F64).float()
    return op, L, host, outs


def region(buf, out, p=None):
    """the (probes, count) values of an output tuple / (base, count, ps, P) region in a host buffer"""
    if len(out) == 7:
        _, _, base, count, ps, Pn, _ = out
    else:
        base, count, ps, Pn = out
    rows = [buf[base + q * ps: base + q * ps + count] for q in range(Pn)]
    return torch.stack(rows) if p is None else rows[p]


class MagMachine(TapeMachine):
    """Mag of HEAD, PRIMAL_POST and SOFTMAX.  Its buffers hold |operand|; ``signed`` is a TapeMachine on the operands."""

    signed: Optional[TapeMachine] = None

    def head(self, op, P, mode, c):
        # every difference of the head actions as a sum: c w (|u| + sum_k p |u|), c (s |u| + (sum_k s |u|) p)
        n, K = op.n_img, op.N
        if mode == nv.HEAD_GGN:
            rin, rout = op.seg[0].a, op.out
        elif mode in (nv.HEAD_LT, nv.HEAD_OUT):
            rin, rout = op.seg[0].a, op.out2
        else:
            rin, rout = op.out2, op.out
        u = self.view(rin, P, n * K).reshape(P, n, K)
        if (not op.classifier) or mode in (nv.HEAD_OUT, nv.HEAD_IN):
            v = c * u
        else:
            p = self.view(op.aux0, 1, n * K).reshape(1, n, K)
            s = self.view(op.aux1, 1, n * K).reshape(1, n, K)
            if mode == nv.HEAD_GGN:
                v = c * p * (u + (p * u).sum(-1, keepdim=True))
            elif mode == nv.HEAD_LT:
                v = c * s * (u + (p * u).sum(-1, keepdim=True))
            else:
                v = c * (s * u + (s * u).sum(-1, keepdim=True) * p)
        self.view(rout, P, n * K).copy_(v.reshape(P, n * K))

    def primal_post(self, op):
        # Y = Mag of the pre-activation (BatchNorm's y - mean as |y| + |mean|).  none / relu: Mag_a = Y.
        # tanh, GELU: the magnitude of the terms of a and of act' at Y, with the cancelling 1 - t^2 taken as 1 + t^2,
        # plus Y itself where y was formed by arithmetic (bias, BatchNorm, residual): its roundings (<= 6 units of Y)
        # pass through act and act', whose slopes are at most 1.13.
        R, N = op.n_img * op.OH * op.OW, op.N
        y = self.view(op.seg[0].a, 1, R * N).reshape(R, N).clone()
        arith = False
        if op.e0.space != nv.SP_NONE:
            y = y + self.view(op.e0, 1, N)
            arith = True
        if op.e1.space != nv.SP_NONE:
            xh = (y + self.view(op.aux0, 1, N)) * self.view(op.aux1, 1, N)
            self.view(op.out3, 1, R * N).copy_(xh.reshape(1, -1))
            y = xh * self.view(op.e1, 1, N) + self.view(op.scale, 1, N)
            arith = True
        if op.res.space != nv.SP_NONE:
            y = y + self.view(op.res, 1, R * N).reshape(R, N)
            arith = True
        if op.act in (0, 1):
            a, d = y, torch.ones_like(y)
        elif op.act == 2:
            t = torch.tanh(y)
            a, d = t, 1 + t * t
        else:
            k0, k1 = 0.7978845608028654, 0.044715
            t = torch.tanh(k0 * (y + k1 * y ** 3))
            a = 0.5 * y * (1 + t)
            d = 0.5 * (1 + t) + 0.5 * y * (1 + t * t) * k0 * (1 + 3 * k1 * y * y)
        if arith and op.act in (2, 3):
            a, d = a + y, d + y
        self.view(op.out, 1, R * N).copy_(a.reshape(1, -1))
        if op.out2.space != nv.SP_NONE:
            self.view(op.out2, 1, R * N).copy_(d.reshape(1, -1))

    def softmax(self, op):
        # p = exp(f - max f) / sum: the rounding of f - max f (half a unit of |f - max f|) is a RELATIVE error of p, so
        # Mag_p = p (1 + |f - max f|), and half of that relative error reaches sqrt(p)
        n, K = op.n_img, op.N
        f = self.signed.view(op.seg[0].a, 1, n * K).reshape(n, K)
        p = torch.softmax(f, -1)
        w = 1 + (f - f.max(-1, keepdim=True).values).abs()
        self.view(op.out, 1, n * K).copy_((p * w).reshape(1, -1))
        self.view(op.out2, 1, n * K).copy_((p.sqrt() * w).reshape(1, -1))
