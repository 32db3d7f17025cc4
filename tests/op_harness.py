"""Op-level harness for the kernel routes — TEST INFRASTRUCTURE (a plain helper module; the specs and Mag of the
non-GEMM ops are in its sibling small_op_harness.py).

One synthetic IGEMM / WGRAD op is laid out in the caller-owned V, Y and H blocks (plus, for a few cases, the engine's
WORK, PRIM and CONST buffers), run once through ``lip_engine_run_op`` and compared element by element with
``tape_emulator.TapeMachine.run_op`` in float64 on float64 copies of the same buffers.

* Bound: ``|y - ref| <= k * 2^-24 * Mag + tiny`` where ``Mag`` is the emulator's result on the absolute values of every
  operand (epilogue fields and the accumulation prefill included).  For exact-f32 routes ``k = Ktot + 16`` (red0 / red1:
  ``+ R``) bounds any summation order; Winograd and bf16x3 get measured constants on ``Mag``.
* RMS: the error normalised by ``2^-24 * Mag`` has an RMS that grows like ``sqrt(Ktot)``; a dropped K-tile or a bad
  transform coefficient shows there long before the worst-case bound.
* Canaries: every float of V, Y, H and of the engine buffers that the op must not write holds a NaN payload before
  the run and must be bitwise unchanged after it; so must every input.  Outputs sit between guard zones.
* Accumulation: WGRAD outputs, red0 and red1 are prefilled with random values; the result is prefill + product.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

from lip_amd import _native as nv

F64 = torch.float64
U24 = 2.0 ** -24
CANARY = 0x7FC0DEAD                  # quiet-NaN payload: no kernel result or input value has these bits
GUARD = 16384                        # floats around every region of V / Y / H (>= one 128 x 128 tile)
GUARD_SMALL = 1024                   # ... of the engine's WORK / PRIM / CONST buffers
TINY = 1e-30

SPACES = {"V": nv.SP_VIN, "Y": nv.SP_YOUT, "H": nv.SP_HEAD, "W": nv.SP_WORK, "P": nv.SP_PRIM, "C": nv.SP_CONST}


@dataclass
class SegSpec:
    IH: int
    IW: int
    C: int
    KH: int = 3
    KW: int = 3
    stride: int = 1
    pad: int = 1
    mode: int = 0
    a_pp: bool = False                # A per probe (else shared)
    b_pp: bool = False                # B per probe
    b_trans: bool = False
    a_space: str = "V"
    b_space: str = "V"
    a_odd: bool = False               # per-probe A with an odd probe stride (C % 4 != 0 only)
    pad_w: int = None                 # padding of the W axis (None: pad, which is then the padding of both axes)

    def __post_init__(self):
        if self.pad_w is None:
            self.pad_w = self.pad

    @property
    def Ktot(self):
        return self.KH * self.KW * self.C


@dataclass
class OpSpec:
    kind: int                         # nv.OP_IGEMM or nv.OP_WGRAD
    segs: List[SegSpec]
    n_img: int
    OH: int
    OW: int
    N: int
    P: int
    out_space: str = "Y"
    out_shift: int = 0                # floats added to the output offset (0: 16-byte aligned)
    epi: Dict[str, str] = field(default_factory=dict)    # field -> "shared" | "probe" | space letter suffix ":C" etc.
    ksplit: int = 0

    @property
    def R(self):
        return self.n_img * self.OH * self.OW

    @property
    def M(self):
        return self.segs[0].Ktot


class Layout:
    """Bump allocator of operand regions per space; offsets in floats, regions 16-byte aligned, guard zones between."""

    def __init__(self, chunk):
        self.chunk = chunk
        self.cur = {k: (GUARD if k in "VYH" else GUARD_SMALL) for k in SPACES}
        self.regions: Dict[str, List[Tuple[int, int, int, int]]] = {k: [] for k in SPACES}   # (base, count, ps, P)
        self.outputs: Dict[str, List[Tuple[int, int, int, int]]] = {k: [] for k in SPACES}

    def alloc(self, space, count, P=1, ps=None, shift=0, output=False):
        """a (P, count) region with probe stride ps; returns (ref off, ps, first float).  WORK offsets count chunk floats."""
        if ps is None:
            ps = 0 if P == 1 else ((count + 3) // 4) * 4 + 4           # a gap between probes (checked as canary)
        span = (P - 1) * ps + count + shift
        g = GUARD if space in "VYH" else GUARD_SMALL
        base = ((self.cur[space] + 3) // 4) * 4
        if space == "W":
            off = (base + self.chunk - 1) // self.chunk
            base = off * self.chunk
        else:
            off = base
        base += shift
        self.cur[space] = base + span + g
        (self.outputs if output else self.regions)[space].append((base, count, ps, P))
        return (off + shift if space != "W" else off), ps, base

    def size(self, space):
        return self.cur[space]


def _ref(space, off=0, ps=0):
    return nv.Ref(SPACES[space] if space else nv.SP_NONE, 0, off, ps)


class Harness:
    """One engine bound to a small net with max_chunk >= the largest P; synthetic ops run against its buffers."""

    def __init__(self, max_chunk=256):
        from lip_amd.engine import LinearizedNet
        from lip_amd.netspec import NetSpec
        from lip_amd.toymodels import create_state
        net = NetSpec((8, 8, 16))
        x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, bn="BatchNorm_0", act="relu")
        x = net.conv(x, "Conv_1", 32, 3, 1, padding=1, bn="BatchNorm_1", act="relu")
        x = net.meanpool(x)
        net.dense(x, "Dense_0", 10)
        net.model_type = "classifier"
        state = create_state(net, 0, dtype=F64)
        Z = torch.rand(4, 8, 8, 16, dtype=F64, generator=torch.Generator().manual_seed(0))
        self.eng = LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 30, max_chunk=max_chunk)
        assert self.eng.chunk == max_chunk
        torch.cuda.synchronize()
        self.chunk = max_chunk
        self.lib = self.eng.lib

    # ------------------------------------------------------------------ census
    def routes(self) -> Dict[str, int]:
        n = self.lib.lip_debug_route_count()
        import ctypes as C
        counts = (C.c_int64 * n)()
        names = (C.c_char_p * n)()
        nv.check(self.lib.lip_debug_routes(counts, n, names), "lip_debug_routes")
        return {names[i].decode(): counts[i] for i in range(n) if counts[i]}

    # ------------------------------------------------------------------ one op
    def build(self, spec: OpSpec, seed=0):
        """lay the op out; returns (op, layout, host buffers {space: float32 tensor}, output index sets)."""
        g = torch.Generator().manual_seed(seed)
        L = Layout(self.chunk)
        op = nv.Op()
        op.kind = spec.kind
        op.nseg = len(spec.segs)
        op.n_img, op.OH, op.OW, op.N, op.ksplit = spec.n_img, spec.OH, spec.OW, spec.N, spec.ksplit
        op.M = spec.M
        for f in nv.REF_FIELDS:
            setattr(op, f, _ref(None))
        fills = []                                     # inputs: (space, first float, count, probe stride, probes)
        R, N, P = spec.R, spec.N, spec.P
        for s, sg in enumerate(spec.segs):
            seg = op.seg[s]
            seg.IH, seg.IW, seg.C, seg.KH, seg.KW = sg.IH, sg.IW, sg.C, sg.KH, sg.KW
            seg.stride, seg.pad_h, seg.pad_w, seg.mode = sg.stride, sg.pad, sg.pad_w, sg.mode
            seg.flags = nv.SEG_B_TRANS if sg.b_trans else 0
            acount = spec.n_img * sg.IH * sg.IW * sg.C
            if spec.kind == nv.OP_WGRAD:               # a: shared activations, b: per-probe cotangent [P][R][N]
                off, ps, base = L.alloc(sg.a_space, acount)
                seg.a = _ref(sg.a_space, off, 0)
                fills.append((sg.a_space, base, acount, 0, 1))
                off, ps, base = L.alloc(sg.b_space, R * N, P)
                seg.b = _ref(sg.b_space, off, ps)
                fills.append((sg.b_space, base, R * N, ps, P))
                continue
            Pa = P if sg.a_pp else 1
            aps = (acount + 1 if (acount + 1) % 2 else acount + 2) if sg.a_odd else None
            off, ps, base = L.alloc(sg.a_space, acount, Pa, aps)
            seg.a = _ref(sg.a_space, off, ps)
            fills.append((sg.a_space, base, acount, ps, Pa))
            Pb = P if sg.b_pp else 1
            off, ps, base = L.alloc(sg.b_space, sg.Ktot * N, Pb)
            seg.b = _ref(sg.b_space, off, ps)
            fills.append((sg.b_space, base, sg.Ktot * N, ps, Pb))
        outs = []
        if spec.kind == nv.OP_WGRAD:
            off, ps, base = L.alloc(spec.out_space, spec.M * N, P, shift=spec.out_shift, output=True)
            op.out = _ref(spec.out_space, off, ps)
            outs.append(("out", spec.out_space, base, spec.M * N, ps, P, True))
        else:
            Po = 1 if spec.out_space == "P" else P
            off, ps, base = L.alloc(spec.out_space, R * N, Po, shift=spec.out_shift, output=True)
            op.out = _ref(spec.out_space, off, ps)
            outs.append(("out", spec.out_space, base, R * N, ps, Po, False))
        for name, how in spec.epi.items():
            how, _, sp = how.partition(":")
            sp = sp or "V"
            if name in ("red0", "red1"):
                off, ps, base = L.alloc("Y", N, P, output=True)
                setattr(op, name, _ref("Y", off, ps))
                outs.append((name, "Y", base, N, ps, P, True))
                continue
            per = how == "probe"
            count = N if name in ("scale", "e0", "e1") else R * N
            Pf = P if per else 1
            off, ps, base = L.alloc(sp, count, Pf)
            setattr(op, name, _ref(sp, off, ps))
            fills.append((sp, base, count, ps, Pf))
        host = self.buffers(L)
        for sp, base, count, ps, Pn in fills:
            for p in range(Pn):
                v = torch.randn(count, generator=g, dtype=F64).float()
                host[sp][base + p * ps: base + p * ps + count] = v
        for name, sp, base, count, ps, Pn, pre in outs:
            if pre:
                for p in range(Pn):
                    host[sp][base + p * ps: base + p * ps + count] = torch.randn(count, generator=g, dtype=F64).float()
        return op, L, host, outs

    def buffers(self, L):
        """host copies of every space, sized by the layout, every float a canary"""
        eng = self.eng
        sizes = {k: L.size(k) for k in "VYH"}
        host = {k: torch.full((sizes[k],), 0, dtype=torch.int32).view(torch.float32) for k in "VYH"}
        for k in "VYH":
            host[k].view(torch.int32).fill_(CANARY)
        for k, t in (("W", eng.work), ("P", eng.prim), ("C", eng.consts)):
            need = L.size(k) - GUARD_SMALL
            used = any(L.regions[k]) or any(L.outputs[k])
            assert not used or need <= t.numel(), f"space {k}: {need} floats needed, {t.numel()} bound"
            host[k] = torch.full((t.numel(),), 0, dtype=torch.int32)
            host[k].fill_(CANARY)
            host[k] = host[k].view(torch.float32)
        return host

    def upload(self, host):
        eng = self.eng
        dev = {k: host[k].cuda() for k in "VYH"}
        eng.work.copy_(host["W"])
        eng.prim.copy_(host["P"])
        eng.consts.copy_(host["C"])
        return dev

    def run(self, op, dev, P, head_mode=0, head_c=1.0):
        nv.check(self.run_rc(op, dev, P, head_mode, head_c), "lip_engine_run_op")
        torch.cuda.synchronize()

    def run_rc(self, op, dev, P, head_mode=0, head_c=1.0):
        """the return code of lip_engine_run_op (for ops the engine must refuse)"""
        return self.lib.lip_engine_run_op(self.eng.h, op, nv.ptr(dev["V"]), nv.ptr(dev["Y"]), nv.ptr(dev["H"]), P, head_mode,
                                          head_c, nv.stream_ptr())

    def download(self, dev):
        eng = self.eng
        out = {k: dev[k].cpu() for k in "VYH"}
        out["W"], out["P"], out["C"] = eng.work.cpu(), eng.prim.cpu(), eng.consts.cpu()
        return out

    def emulate(self, op, host, P, absolute=False, head_mode=0, head_c=1.0):
        return emulate(self.eng.cn, self.chunk, op, host, P, absolute, head_mode, head_c)


def _machine(cls, cn, chunk, b):
    tm = cls.__new__(cls)
    tm.cn, tm.chunk = cn, chunk
    tm.V, tm.Y, tm.H = b["V"], b["Y"], b["H"]
    tm.work, tm.prim, tm.consts = b["W"], b["P"], b["C"]
    tm.theta = torch.zeros(1, dtype=F64)
    return tm


def emulate(cn, chunk, op, host, P, absolute=False, head_mode=0, head_c=1.0):
    """float64 result of the op on copies of the host buffers (absolute: on |every operand|, giving Mag; the ops that
    subtract or are not linear take their Mag from small_op_harness.MagMachine)."""
    from tape_emulator import TapeMachine
    b = {k: (host[k].double().abs() if absolute else host[k].double()) for k in host}
    if absolute and op.kind in (nv.OP_HEAD, nv.OP_PRIMAL_POST, nv.OP_SOFTMAX):
        from small_op_harness import MagMachine
        tm = _machine(MagMachine, cn, chunk, b)
        tm.signed = _machine(TapeMachine, cn, chunk, {k: host[k].double() for k in host})
    else:
        tm = _machine(TapeMachine, cn, chunk, b)
    tm.run_op(op, P, head_mode, abs(head_c) if absolute else head_c)
    return b


def output_mask(host, outs):
    """{space: bool mask of the output elements}"""
    m = {k: torch.zeros(host[k].numel(), dtype=torch.bool) for k in host}
    for name, sp, base, count, ps, Pn, pre in outs:
        for p in range(Pn):
            m[sp][base + p * ps: base + p * ps + count] = True
    return m


def check(got, ref, mag, host, outs, k_of, rms_c, what="", exact=(), skip=None, floor=None):
    """element-wise + RMS bound on every output, canaries and inputs bitwise unchanged.  k_of(name) -> (k, kref) where
    kref scales the RMS bound (sqrt(kref) * rms_c), or (k, kref, rms_c) with a constant of its own for that output.
    Returns {output name: (max normalised err, rms normalised err)}.

    exact: output names that must equal the float32 value of the reference bitwise (gathers: no Mag).
    skip: {output name: bool mask over the output's (probe, element) order} of elements left out of the comparison
    (they must still be written and finite).  floor: {output name: absolute error allowed on top of the bound}."""
    mask = output_mask(host, outs)
    for k in host:
        keep = ~mask[k]
        a, b = got[k].view(torch.int32)[keep], host[k].view(torch.int32)[keep]
        if not torch.equal(a, b):
            idx = torch.nonzero(a != b)[:5].flatten().tolist()
            pos = torch.nonzero(keep).flatten()[idx].tolist()
            raise AssertionError(f"{what}: space {k}: {int((a != b).sum())} floats outside the outputs changed "
                                 f"(first at {pos})")
    stats = {}
    for name, sp, base, count, ps, Pn, pre in outs:
        idx = torch.cat([torch.arange(base + p * ps, base + p * ps + count) for p in range(Pn)])
        y = got[sp][idx].double()
        r = ref[sp][idx]
        M = mag[sp][idx]
        assert torch.isfinite(y).all(), f"{what}: {name}: {int((~torch.isfinite(y)).sum())} elements not written or not finite"
        if name in exact:
            a, b = got[sp][idx].view(torch.int32), r.float().view(torch.int32)
            if skip is not None and name in skip:
                a, b = a[~skip[name]], b[~skip[name]]
            ne = a != b
            if ne.any():
                i = int(torch.nonzero(ne)[0])
                raise AssertionError(f"{what}: {name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise from the float32 "
                                     f"reference (first at {i}: got bits {int(a[i]):#x}, ref bits {int(b[i]):#x})")
            stats[name] = (0.0, 0.0)
            continue
        kk = k_of(name)
        k, kref = kk[0], kk[1]
        c_rms = kk[2] if len(kk) > 2 else rms_c
        e = ((y - r).abs() - (floor or {}).get(name, 0.0)).clamp_min(0) / (U24 * M + TINY)
        if skip is not None and name in skip:
            e = e[~skip[name]]
        bad = e > k
        if bad.any():
            i = int(torch.argmax(e))
            raise AssertionError(f"{what}: {name}: {int(bad.sum())} of {e.numel()} elements above {k:.3g} * 2^-24 * Mag "
                                 f"(worst {e[i].item():.3g} at {i}: got {y[i].item():.9g}, ref {r[i].item():.9g}, Mag {M[i].item():.3g})")
        rms = e.pow(2).mean().sqrt().item()
        bound = c_rms * math.sqrt(kref)
        assert rms <= bound, f"{what}: {name}: RMS of the normalised error {rms:.4g} above {bound:.4g} (= {c_rms} sqrt({kref}))"
        stats[name] = (e.max().item(), rms / math.sqrt(kref))
    return stats


def all_routes(lib) -> List[str]:
    import ctypes as C
    n = lib.lip_debug_route_count()
    names = (C.c_char_p * n)()
    counts = (C.c_int64 * n)()
    nv.check(lib.lip_debug_routes(counts, n, names), "lip_debug_routes")
    return [names[i].decode() for i in range(n)]
