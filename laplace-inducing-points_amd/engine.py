"""NetSpec -> op tapes for the HIP engine, and the handle wrapper around the C ABI.

``compile_net`` is pure Python (no GPU): it lays out the cached primal tensors, the
per-binding constants and the probe workspace, and emits the three op tapes of
``include/lip.h``:

  primal   : per unit  IGEMM(z = conv(a, W))  ->  PRIMAL_POST(xhat, a = act(y), act'(y));  SOFTMAX
  tangent  : per unit  IGEMM(conv(da, W) + conv(a, dW_p), epilogue: BN/bias tangent, residual, act');
             HEAD
  backward : HEAD; per tensor (reverse)  IGEMM(act' * (sum_consumers convT(g, W^T s) + res),
             reductions into the bias / BN cotangents);  WGRAD(dW_p)

The linearisation point never changes across Krylov iterations, so everything primal is
cached once per binding — the reference re-evaluates the forward pass three times per example
per matvec (``src/ggn.py:139,140,142``).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _native as nv
from .netspec import ACT_IDS, NetSpec, Unit, _get
from .utils import param_layout


def _r4(x: int) -> int:
    return (x + 3) // 4 * 4


class VT:
    """A virtual workspace tensor (per-probe size in floats), placed by the allocator."""
    __slots__ = ("size", "off", "name")

    def __init__(self, size: int, name: str = ""):
        self.size, self.off, self.name = _r4(size), None, name


NONE = (nv.SP_NONE, 0, 0)


@dataclasses.dataclass
class SymOp:
    kind: int
    f: Dict[str, Any]                 # scalar fields
    refs: Dict[str, Any]              # ref fields: (space, off, pstride) or ('work', VT, pstride)
    segs: List[Dict[str, Any]] = dataclasses.field(default_factory=list)

    def work_tensors(self):
        for r in list(self.refs.values()) + [s[k] for s in self.segs for k in ("a", "b")]:
            if r[0] == "work":
                yield r[1]


@dataclasses.dataclass
class CompiledNet:
    net: NetSpec
    n: int
    D: int
    K: int
    classifier: bool
    offsets: Dict[Tuple, Tuple[int, Tuple[int, ...]]]
    prim_floats: int
    const_floats: int
    work_pp: int
    tapes: List[List[nv.Op]]
    a_off: Dict[int, int]
    const_plan: List[Tuple]           # how to fill the constants buffer
    prob_off: int
    input_off: int
    meta: Dict[str, Any] = dataclasses.field(default_factory=dict)   # per-tensor offsets the second-order pass needs
    train_tapes: List[List[nv.Op]] = dataclasses.field(default_factory=list)   # compile_net(train=True): [primal, backward]
    train_work_pp: int = 0            # workspace floats of the train backward tape (one probe: the minibatch)

    def last_unit(self) -> Unit:
        """the final unit, a plain Dense (:func:`last_dense_unit`)"""
        return last_dense_unit(self.net)

    def last_layer(self) -> Tuple[int, int, int]:
        """``(offset, F, K)`` of the final Dense layer (:func:`last_layer_of`)"""
        return last_layer_of(self.net, self.offsets)


def last_dense_unit(net: NetSpec) -> Unit:
    """The final unit, which must be a plain Dense: a conv unit with a bias, no BN, no residual, no activation, whose
    window covers its whole source (a 1 x 1 source, or the flattened feature map of ``flat_kernel``) so that the
    output is 1 x 1.  Anything else raises ``ValueError``: the last-layer posterior needs a head linear in theta_L."""
    u = net.units[-1] if net.units else None
    if u is None or u.kind != "conv" or u.dst != net.out:
        raise ValueError("last-layer Laplace needs a final Dense unit; the network ends in "
                         f"{'nothing' if u is None else repr(u.kind)}")
    ih, iw, _ = net.tensors[u.src]
    plain = (u.bias is not None and u.bn_scale is None and u.res is None and u.act == "none" and
             tuple(net.tensors[u.dst][:2]) == (1, 1) and (u.kh, u.kw) == (ih, iw) and u.pad_h == 0 and u.pad_w == 0)
    if not plain:
        raise ValueError("last-layer Laplace needs a plain final Dense (bias, no BN, no residual, act='none', 1x1 "
                         f"output); got act={u.act!r}, bias={u.bias is not None}, bn={u.bn_scale is not None}, "
                         f"res={u.res is not None}, window {u.kh}x{u.kw} on a {ih}x{iw} source")
    return u


def last_layer_of(net: NetSpec, layout: Dict[Tuple, Tuple[int, Tuple[int, ...]]]) -> Tuple[int, int, int]:
    """``(offset, F, K)`` of the final Dense: theta_L = theta[offset : offset + (F + 1) K] = [bias (K), kernel (F, K)
    row-major], F the flattened width of its source; ``layout`` maps a parameter path to (flat offset, shape) as
    ``param_layout`` gives them.  Raises ``ValueError`` when the last unit is not a plain Dense
    (:func:`last_dense_unit`) or when bias and kernel are not adjacent in the flat layout in that order."""
    u = last_dense_unit(net)
    F, K = u.kh * u.kw * u.cin, u.cout
    boff, koff = layout[u.bias][0], layout[u.kernel][0]
    if koff != boff + K:
        raise ValueError(f"last-layer Laplace needs the final bias (offset {boff}, {K} entries) directly before its "
                         f"kernel (offset {koff}) in the flat parameter order")
    return boff, F, K


@dataclasses.dataclass
class KfacBlock:
    """One layer block of the Kronecker-factored posterior: the flat slice theta[off : off + Mt N] = [bias (N)] + kernel
    (M x N row-major) of a conv unit read as an (Mt, N) matrix, the bias row 0 when the unit has one; T = OH OW output
    positions; ``bn`` the (offset, N) slice of the frozen BN scale s in the constants buffer, or None; ``src`` the
    offset of the unit's input tensor in ``prim``; ``final``: the plain final Dense, whose classifier factor is centred."""
    unit: Unit
    off: int
    Mt: int
    N: int
    T: int
    bias: bool
    kernel_off: int
    final: bool = False
    bn: Optional[Tuple[int, int]] = None
    src: Optional[int] = None


def kfac_block_table(net: NetSpec, layout: Dict[Tuple, Tuple[int, Tuple[int, ...]]]) -> List[KfacBlock]:
    """The layer blocks of ``net``, one per conv unit in unit order, from the layer program and the flat layout
    (``param_layout``) alone: pure Python.  Raises ``ValueError`` when a unit's bias is not directly before its kernel
    in the flat parameter order."""
    try:
        last = last_dense_unit(net)
    except ValueError:
        last = None
    blocks = []
    for u in net.units:
        if u.kind != "conv":
            continue
        M, N = u.kh * u.kw * u.cin, u.cout
        oh, ow, _ = net.tensors[u.dst]
        koff = layout[u.kernel][0]
        off = koff
        if u.bias is not None:
            off = layout[u.bias][0]
            if koff != off + N:
                raise ValueError(f"the Kronecker-factored posterior needs the bias of {'/'.join(map(str, u.kernel[:-1]))} "
                                 f"(offset {off}, {N} entries) directly before its kernel (offset {koff}) in the flat "
                                 f"parameter order")
        blocks.append(KfacBlock(u, off, M + (u.bias is not None), N, oh * ow, u.bias is not None, koff, final=u is last))
    return blocks


def _seg(a, b, IH, IW, Cc, KH, KW, stride, pad_h, pad_w, mode):
    return dict(a=a, b=b, IH=IH, IW=IW, C=Cc, KH=KH, KW=KW, stride=stride, pad_h=pad_h, pad_w=pad_w, mode=mode)


BN_MOMENTUM = 0.99       # flax.linen.BatchNorm's default: running = momentum * running + (1 - momentum) * batch


def compile_net(net: NetSpec, n: int, params: Dict[str, Any], train: bool = False) -> CompiledNet:
    """The three tapes of a binding of ``n`` examples.  ``train=True`` adds the two train tapes of MAP training
    (``CompiledNet.train_tapes``: primal with batch statistics, backward through them), slots for the running statistics
    at the END of the constants (the offsets of everything else, and the three tapes, are those of ``train=False``) and
    the workspace the train backward tape needs (``train_work_pp``)."""
    layout = {path: (off, shape) for path, off, shape in param_layout(params)}
    D = sum(int(torch.Size(s).numel()) for _, s in layout.values())
    K = net.num_outputs
    classifier = getattr(net, "model_type", "classifier") == "classifier"
    tens = net.tensors

    def poff(path) -> int:
        if path not in layout:
            raise KeyError(f"parameter {path} is not in state.params")
        return layout[path][0]

    # ------------------------------------------------------------------ primal / const layout
    prim = 0

    def palloc(sz):
        nonlocal prim
        o = prim
        prim += _r4(sz)
        return o

    a_off: Dict[int, int] = {0: palloc(n * tens[0][0] * tens[0][1] * tens[0][2])}
    dphi_off: Dict[int, int] = {}
    xhat_off: Dict[int, int] = {}
    amax_off: Dict[int, int] = {}
    producer: Dict[int, Unit] = {}
    zmax = 0
    for u in net.units:
        producer[u.dst] = u
        h, w, c = tens[u.dst]
        if u.kind == "view":
            a_off[u.dst] = a_off[u.src]
            continue
        a_off[u.dst] = palloc(n * h * w * c)
        if u.kind == "maxpool":
            amax_off[u.dst] = palloc(n * h * w * c)
        if u.kind == "avgpool":
            amax_off[u.dst] = None             # a NONE argmax ref selects the window average (include/lip.h)
        if u.kind == "conv":
            zmax = max(zmax, n * h * w * c)
            if u.act != "none":
                dphi_off[u.dst] = palloc(n * h * w * c)
            if u.bn_scale is not None:
                xhat_off[u.dst] = palloc(n * h * w * c)
    z_off = palloc(zmax)
    prob_off = palloc(n * K)
    sqrtp_off = palloc(n * K)

    cst = 0
    const_plan: List[Tuple] = []
    s_off: Dict[int, int] = {}
    mean_off: Dict[int, int] = {}
    rstd_off: Dict[int, int] = {}
    wt_off: Dict[int, int] = {}

    def calloc(sz):
        nonlocal cst
        o = cst
        cst += _r4(sz)
        return o

    for u in net.units:
        if u.kind != "conv":
            continue
        if u.bn_scale is not None:
            s_off[u.dst] = calloc(u.cout)
            mean_off[u.dst] = calloc(u.cout)
            rstd_off[u.dst] = calloc(u.cout)
            const_plan.append(("bn", u, s_off[u.dst], mean_off[u.dst], rstd_off[u.dst]))
        if u.src != 0 and producer.get(u.src, None) is not None and _has_grad(net, u.src):
            wt_off[u.dst] = calloc(u.kh * u.kw * u.cout * u.cin)
            const_plan.append(("wt", u, wt_off[u.dst], s_off.get(u.dst)))
    cst = max(cst, 4)
    run_off: Dict[int, Tuple[int, int]] = {}
    if train:
        for u in net.units:
            if u.kind == "conv" and u.bn_scale is not None:
                run_off[u.dst] = (calloc(u.cout), calloc(u.cout))
                const_plan.append(("run", u, run_off[u.dst][0], run_off[u.dst][1]))

    P = lambda off: (nv.SP_PRIM, off, 0)
    TH = lambda off: (nv.SP_THETA, off, 0)
    CS = lambda off: (nv.SP_CONST, off, 0)
    VIN = lambda off: (nv.SP_VIN, off, D)
    YO = lambda off: (nv.SP_YOUT, off, D)

    def geom(u: Unit):
        ih, iw, _ = tens[u.src]
        return dict(IH=ih, IW=iw, Cc=u.cin, KH=u.kh, KW=u.kw, stride=u.stride, pad_h=u.pad_h, pad_w=u.pad_w)

    def AMAX(t):
        return NONE if amax_off[t] is None else P(amax_off[t])

    def pool_seg(u: Unit, a_ref):
        ih, iw, cc = tens[u.src]
        return _seg(a_ref, NONE, ih, iw, cc, u.kh, u.kw, u.stride, u.pad_h, u.pad_w, 0)

    # ------------------------------------------------------------------ primal tape
    primal: List[SymOp] = []
    for u in net.units:
        if u.kind == "view":
            continue
        oh, ow, c = tens[u.dst]
        if u.kind == "meanpool":
            ih, iw, _ = tens[u.src]
            primal.append(SymOp(nv.OP_POOL_FWD, dict(n_img=n, OH=ih, OW=iw, N=c, fscale=1.0 / (ih * iw)),
                                dict(out=P(a_off[u.dst])), [dict(a=P(a_off[u.src]), b=NONE)]))
            continue
        if u.kind in ("maxpool", "avgpool"):
            primal.append(SymOp(nv.OP_MAXPOOL_PRIMAL, dict(n_img=n, OH=oh, OW=ow, N=c),
                                dict(out=P(a_off[u.dst]), aux0=AMAX(u.dst)), [pool_seg(u, P(a_off[u.src]))]))
            continue
        g = geom(u)
        primal.append(SymOp(nv.OP_IGEMM, dict(n_img=n, OH=oh, OW=ow, N=c), dict(out=P(z_off)),
                            [_seg(P(a_off[u.src]), TH(poff(u.kernel)), g["IH"], g["IW"], g["Cc"], g["KH"], g["KW"],
                                  g["stride"], g["pad_h"], g["pad_w"], 0)]))
        refs = dict(out=P(a_off[u.dst]))
        if u.dst in dphi_off:
            refs["out2"] = P(dphi_off[u.dst])
        if u.bias is not None:
            refs["e0"] = TH(poff(u.bias))
        if u.bn_scale is not None:
            refs["out3"] = P(xhat_off[u.dst])
            refs["e1"] = TH(poff(u.bn_scale))
            refs["scale"] = TH(poff(u.bn_bias))
            refs["aux0"] = CS(mean_off[u.dst])
            refs["aux1"] = CS(rstd_off[u.dst])
        if u.res is not None:
            refs["res"] = P(a_off[u.res])
        primal.append(SymOp(nv.OP_PRIMAL_POST, dict(n_img=n, OH=oh, OW=ow, N=c, act=ACT_IDS[u.act]), refs,
                            [dict(a=P(z_off), b=NONE)]))
    if classifier:
        primal.append(SymOp(nv.OP_SOFTMAX, dict(n_img=n, OH=1, OW=1, N=K),
                            dict(out=P(prob_off), out2=P(sqrtp_off)), [dict(a=P(a_off[net.out]), b=NONE)]))

    # the train primal tape: the same ops without the SOFTMAX (the loss head takes the logits), and BN_STATS between a
    # BN unit's IGEMM and its PRIMAL_POST, which then normalises with the batch statistics BN_STATS left in CONST
    train_primal: List[SymOp] = []
    if train:
        conv_at = {a_off[u.dst]: u for u in net.units if u.kind == "conv"}
        for op in primal:
            if op.kind == nv.OP_SOFTMAX:
                continue
            if op.kind == nv.OP_PRIMAL_POST and "e1" in op.refs:
                u = conv_at[op.refs["out"][1]]
                refs = dict(e1=op.refs["e1"], aux0=op.refs["aux0"], aux1=op.refs["aux1"], scale=CS(s_off[u.dst]),
                            out=CS(run_off[u.dst][0]), out2=CS(run_off[u.dst][1]))
                if "e0" in op.refs:
                    refs["e0"] = op.refs["e0"]
                train_primal.append(SymOp(nv.OP_BN_STATS, dict(n_img=n, OH=op.f["OH"], OW=op.f["OW"], N=op.f["N"],
                                                               bn_eps=float(u.bn_eps), fscale=BN_MOMENTUM), refs,
                                          [dict(a=P(z_off), b=NONE)]))
            train_primal.append(op)

    # ------------------------------------------------------------------ tangent tape
    def tsize(t):
        h, w, c = tens[t]
        return n * h * w * c

    W = lambda vt: ("work", vt, vt.size)
    g_head = VT(n * K, "g_head")           # reserved: head output / backward input, offset 0 in both tapes
    tangent: List[SymOp] = []
    da: Dict[int, Optional[VT]] = {0: None}
    for u in net.units:
        if u.kind == "view":
            da[u.dst] = da[u.src]
            continue
        oh, ow, c = tens[u.dst]
        out = VT(tsize(u.dst), f"da{u.dst}")
        if u.kind == "meanpool":
            ih, iw, _ = tens[u.src]
            tangent.append(SymOp(nv.OP_POOL_FWD, dict(n_img=n, OH=ih, OW=iw, N=c, fscale=1.0 / (ih * iw)),
                                 dict(out=W(out)), [dict(a=W(da[u.src]), b=NONE)]))
            da[u.dst] = out
            continue
        if u.kind in ("maxpool", "avgpool"):
            tangent.append(SymOp(nv.OP_MAXPOOL_FWD, dict(n_img=n, OH=oh, OW=ow, N=c),
                                 dict(out=W(out), aux0=AMAX(u.dst)), [pool_seg(u, W(da[u.src]))]))
            da[u.dst] = out
            continue
        g = geom(u)
        segs = []
        if da[u.src] is not None:
            segs.append(_seg(W(da[u.src]), TH(poff(u.kernel)), g["IH"], g["IW"], g["Cc"], g["KH"], g["KW"],
                             g["stride"], g["pad_h"], g["pad_w"], 0))
        segs.append(_seg(P(a_off[u.src]), VIN(poff(u.kernel)), g["IH"], g["IW"], g["Cc"], g["KH"], g["KW"],
                         g["stride"], g["pad_h"], g["pad_w"], 0))
        refs = dict(out=W(out))
        if u.bias is not None:
            refs["e0"] = VIN(poff(u.bias))
        if u.bn_scale is not None:
            refs["scale"] = CS(s_off[u.dst])
            refs["e0"] = VIN(poff(u.bn_bias))
            refs["e1"] = VIN(poff(u.bn_scale))
            refs["xhat"] = P(xhat_off[u.dst])
        if u.res is not None and da[u.res] is not None:
            refs["res"] = W(da[u.res])
        if u.dst in dphi_off:
            refs["dphi"] = P(dphi_off[u.dst])
        tangent.append(SymOp(nv.OP_IGEMM, dict(n_img=n, OH=oh, OW=ow, N=c), refs, segs))
        da[u.dst] = out
    head_refs = dict(out=W(g_head), out2=(nv.SP_HEAD, 0, n * K))
    if classifier:
        head_refs["aux0"] = P(prob_off)
        head_refs["aux1"] = P(sqrtp_off)
    tangent.append(SymOp(nv.OP_HEAD, dict(n_img=n, OH=1, OW=1, N=K, classifier=int(classifier)),
                         dict(head_refs), [dict(a=W(da[net.out]), b=NONE)]))

    # ------------------------------------------------------------------ backward tape
    consumers: Dict[int, List[Tuple[Unit, str]]] = {}
    for u in net.units:
        consumers.setdefault(u.src, []).append((u, "src"))
        if u.res is not None:
            consumers.setdefault(u.res, []).append((u, "res"))

    def build_backward(train: bool) -> List[SymOp]:
        """the backward tape; ``train``: every BN unit's cotangent g is followed by BN_TRAIN_BWD, whose corrected copy g'
        feeds the unit's WGRAD and the data-gradient segments through its kernel, while a residual consumer upstream
        keeps reading g (for y = BN(z) + res, d/d res is g, not g')"""
        backward: List[SymOp] = []
        # head input lives in HEAD space (vjp calls); its seg a is unused in modes L / IN
        backward.append(SymOp(nv.OP_HEAD, dict(n_img=n, OH=1, OW=1, N=K, classifier=int(classifier)),
                              dict(head_refs), [dict(a=W(g_head), b=NONE)]))
        gp: Dict[int, VT] = {net.out: g_head}
        gq: Dict[int, VT] = {}            # train: the corrected cotangent g' of a BN unit's output

        def through_kernel(t: int) -> VT:
            """the cotangent that goes through the kernel of the unit producing t (its WGRAD, its data gradient)"""
            return gq.get(t, gp[t])

        def bn_correction(u: Unit, t: int) -> None:
            if not (train and u.kind == "conv" and u.bn_scale is not None):
                return
            h, w, c = tens[t]
            gq[t] = VT(tsize(t), f"gq{t}")
            backward.append(SymOp(nv.OP_BN_TRAIN_BWD, dict(n_img=n, OH=h, OW=w, N=c),
                                  dict(out=W(gq[t]), e0=YO(poff(u.bn_bias)), e1=YO(poff(u.bn_scale)), xhat=P(xhat_off[t])),
                                  [dict(a=W(gp[t]), b=NONE)]))

        def param_reds(u: Unit) -> Dict[str, Any]:
            """reductions into the bias / BN cotangents of the unit that produced the tensor"""
            r: Dict[str, Any] = {}
            if u.kind != "conv":
                return r
            if u.bn_scale is not None:
                r["red0"] = YO(poff(u.bn_bias))
                r["red1"] = YO(poff(u.bn_scale))
                r["xhat2"] = P(xhat_off[u.dst])
            elif u.bias is not None:
                r["red0"] = YO(poff(u.bias))
            return r

        order = [u.dst for u in net.units if u.kind != "view"]
        for t in reversed(order):
            u = producer[t]
            if not _has_grad(net, t):
                continue
            h, w, c = tens[t]
            if t != net.out:
                cons = consumers.get(t, [])
                conv_c = [cu for cu, role in cons if role == "src" and cu.kind == "conv"]
                res_c = [cu for cu, role in cons if role == "res"]
                pool_c = [cu for cu, role in cons if role == "src" and cu.kind == "meanpool"]
                mpool_c = [cu for cu, role in cons if role == "src" and cu.kind in ("maxpool", "avgpool")]
                view_c = [cu for cu, role in cons if cu.kind == "view"]
                if view_c:
                    raise NotImplementedError("flatten of a non-input tensor is not supported by the HIP engine yet")
                if len(res_c) > 1 or len(conv_c) > 3 or ((pool_c or mpool_c) and (conv_c or res_c)) or len(mpool_c) > 1:
                    raise NotImplementedError(f"unsupported fan-out at tensor {t}")
                reds = param_reds(u)
                if mpool_c:
                    mu = mpool_c[0]
                    moh, mow, _ = tens[mu.dst]
                    out = VT(tsize(t), f"g{t}")
                    refs = dict(out=W(out), aux0=AMAX(mu.dst), **reds)
                    if t in dphi_off:
                        refs["dphi"] = P(dphi_off[t])
                    backward.append(SymOp(nv.OP_MAXPOOL_BWD, dict(n_img=n, OH=moh, OW=mow, N=c), refs,
                                          [pool_seg(mu, W(gp[mu.dst]))]))
                    gp[t] = out
                elif pool_c:
                    pu = pool_c[0]
                    out = VT(tsize(t), f"g{t}")
                    refs = dict(out=W(out), **reds)
                    if t in dphi_off:
                        refs["dphi"] = P(dphi_off[t])
                    backward.append(SymOp(nv.OP_POOL_BWD, dict(n_img=n, OH=h, OW=w, N=c, fscale=1.0 / (h * w)), refs,
                                          [dict(a=W(gp[pu.dst]), b=NONE)]))
                    gp[t] = out
                elif not conv_c:
                    # only a residual consumer and no activation of its own: the cotangent is an alias
                    if t in dphi_off:
                        raise NotImplementedError("activated tensor consumed only as a residual")
                    gp[t] = gp[res_c[0].dst]
                    if reds:
                        backward.append(SymOp(nv.OP_REDUCE, dict(n_img=n, OH=h, OW=w, N=c), dict(reds),
                                              [dict(a=W(gp[t]), b=NONE)]))
                else:
                    out = VT(tsize(t), f"g{t}")
                    segs = []
                    for cu in conv_c:
                        coh, cow, cc = tens[cu.dst]
                        segs.append(_seg(W(through_kernel(cu.dst)), CS(wt_off[cu.dst]), coh, cow, cu.cout, cu.kh, cu.kw, cu.stride,
                                         cu.pad_h, cu.pad_w, 1))
                    refs = dict(out=W(out), **reds)
                    if res_c:
                        refs["res"] = W(gp[res_c[0].dst])
                    if t in dphi_off:
                        refs["dphi"] = P(dphi_off[t])
                    backward.append(SymOp(nv.OP_IGEMM, dict(n_img=n, OH=h, OW=w, N=c), refs, segs))
                    gp[t] = out
            else:
                reds = param_reds(u)
                if reds:
                    backward.append(SymOp(nv.OP_REDUCE, dict(n_img=n, OH=h, OW=w, N=c), dict(reds),
                                          [dict(a=W(gp[t]), b=NONE)]))
            bn_correction(u, t)
            if u.kind == "conv":
                g = geom(u)
                refs = dict(out=YO(poff(u.kernel)))
                if u.bn_scale is not None:
                    refs["scale"] = CS(s_off[u.dst])
                backward.append(SymOp(nv.OP_WGRAD, dict(n_img=n, OH=h, OW=w, N=c, ksplit=0, M=u.kh * u.kw * u.cin), refs,
                                      [_seg(P(a_off[u.src]), W(through_kernel(t)), g["IH"], g["IW"], g["Cc"], g["KH"], g["KW"],
                                            g["stride"], g["pad_h"], g["pad_w"], 0)]))
        return backward

    backward = build_backward(False)

    # ------------------------------------------------------------------ workspace placement
    work_pp = 0
    for tape in (tangent, backward):
        work_pp = max(work_pp, _place(tape, g_head))

    tapes = [[_lower(op) for op in tape] for tape in (primal, tangent, backward)]
    train_tapes: List[List[nv.Op]] = []
    train_work_pp = 0
    if train:
        train_backward = build_backward(True)
        train_work_pp = _place(train_backward, g_head)
        train_tapes = [[_lower(op) for op in tape] for tape in (train_primal, train_backward)]
    return CompiledNet(net=net, n=n, D=D, K=K, classifier=classifier, offsets=layout, prim_floats=max(prim, 4),
                       const_floats=cst, work_pp=work_pp, tapes=tapes, a_off=a_off, const_plan=const_plan,
                       prob_off=prob_off, input_off=a_off[0],
                       meta=dict(dphi_off=dphi_off, xhat_off=xhat_off, s_off=s_off, rstd_off=rstd_off, wt_off=wt_off, amax_off=amax_off,
                                 sqrtp_off=sqrtp_off, layout=layout, mean_off=mean_off, run_off=run_off),
                       train_tapes=train_tapes, train_work_pp=train_work_pp)


def _has_grad(net: NetSpec, t: int) -> bool:
    """Does tensor t depend on theta (i.e. is it downstream of a parameterised unit)?"""
    if t == 0:
        return False
    for u in net.units:
        if u.dst == t:
            if u.kind == "conv":
                return True
            return _has_grad(net, u.src)
    return False


def _place(tape: List[SymOp], reserved: VT) -> int:
    """Liveness-based placement of the virtual workspace tensors of one tape; returns floats/probe."""
    for op in tape:
        for vt in op.work_tensors():
            if vt is not reserved:
                vt.off = None
    last: Dict[int, int] = {}
    for i, op in enumerate(tape):
        for vt in op.work_tensors():
            last[id(vt)] = i
    reserved.off = 0
    top = reserved.size
    free: Dict[int, List[int]] = {}
    for i, op in enumerate(tape):
        touched = list(op.work_tensors())
        for vt in touched:
            if vt.off is None:
                lst = free.get(vt.size)
                if lst:
                    vt.off = lst.pop()
                else:
                    vt.off = top
                    top += vt.size
        # lowering happens later; remember placement per op now (offsets may be reused afterwards)
        op._placed = {id(vt): vt.off for vt in touched}            # type: ignore[attr-defined]
        seen = set()
        for vt in touched:
            if vt is reserved or id(vt) in seen:
                continue
            seen.add(id(vt))
            if last[id(vt)] == i:
                free.setdefault(vt.size, []).append(vt.off)
    return top


def _mkref(op: SymOp, r) -> nv.Ref:
    if r[0] == "work":
        return nv.Ref(nv.SP_WORK, 0, op._placed[id(r[1])], r[2])       # type: ignore[attr-defined]
    return nv.Ref(int(r[0]), 0, int(r[1]), int(r[2]))


def _lower(op: SymOp) -> nv.Op:
    o = nv.Op()
    o.kind = op.kind
    o.nseg = len(op.segs)
    for name in nv.REF_FIELDS:
        setattr(o, name, _mkref(op, op.refs.get(name, NONE)))
    for i in range(3):
        if i < len(op.segs):
            s = op.segs[i]
            o.seg[i].a = _mkref(op, s["a"])
            o.seg[i].b = _mkref(op, s.get("b", NONE))
            for k, fld in (("IH", "IH"), ("IW", "IW"), ("C", "C"), ("KH", "KH"), ("KW", "KW"), ("stride", "stride"),
                           ("pad_h", "pad_h"), ("pad_w", "pad_w"), ("mode", "mode"), ("flags", "flags")):
                setattr(o.seg[i], fld, int(s.get(k, 0)))
        else:
            o.seg[i].a = _mkref(op, NONE)
            o.seg[i].b = _mkref(op, NONE)
    for k, v in op.f.items():
        setattr(o, k, v)
    return o


def build_consts(cn: CompiledNet, params: Dict[str, Any], batch_stats: Dict[str, Any], device, dtype=torch.float32):
    """Per-binding constants: BN factors s = gamma * rsqrt(var + eps), mean, rsqrt; and the transposed,
    BN-scaled kernels  Wt[kh][kw][co][ci] = W[kh][kw][ci][co] * s[co]  the data-gradient layers read."""
    out = torch.zeros(cn.const_floats, device=device, dtype=dtype)
    svals: Dict[int, torch.Tensor] = {}
    for item in cn.const_plan:
        if item[0] == "bn":
            _, u, so, mo, ro = item
            var = _get(batch_stats, u.bn_var).to(device=device, dtype=dtype)
            mean = _get(batch_stats, u.bn_mean).to(device=device, dtype=dtype)
            gamma = _get(params, u.bn_scale).to(device=device, dtype=dtype)
            rstd = torch.rsqrt(var + u.bn_eps)
            s = gamma * rstd
            svals[u.dst] = s
            out[so:so + u.cout] = s
            out[mo:mo + u.cout] = mean
            out[ro:ro + u.cout] = rstd
        elif item[0] == "run":
            _, u, mo, vo = item
            out[mo:mo + u.cout] = _get(batch_stats, u.bn_mean).to(device=device, dtype=dtype)
            out[vo:vo + u.cout] = _get(batch_stats, u.bn_var).to(device=device, dtype=dtype)
    for item in cn.const_plan:
        if item[0] == "wt":
            _, u, wo, so = item
            Wk = _get(params, u.kernel).to(device=device, dtype=dtype).reshape(u.kh, u.kw, u.cin, u.cout)
            if so is not None:
                Wk = Wk * svals[u.dst]
            out[wo:wo + Wk.numel()] = Wk.permute(0, 1, 3, 2).reshape(-1)
    return out


def set_precision(mode: str = "f32") -> None:
    """Process-wide arithmetic of the MFMA kernels: ``"f32"`` — exact f32 MFMA (default; bit-for-bit an fmaf
    chain) — or ``"bf16x3"`` — split-precision operands (x = hi + lo in bf16, three bf16 MFMAs per product, f32
    accumulation; ~1e-5 relative error per product, measured 6e-6 on a GGN-vp) at ~5x fewer matrix-pipe cycles."""
    modes = {"f32": 0, "bf16x3": 1}
    if mode not in modes:
        raise ValueError(f"precision must be one of {sorted(modes)}")
    nv.check(nv.load().lip_set_precision(modes[mode]), "lip_set_precision")


def get_precision() -> str:
    return {0: "f32", 1: "bf16x3"}[nv.load().lip_get_precision()]


def tape_flops_per_probe(cn: CompiledNet):
    """ALGORITHMIC FLOPs of one probe's tangent-forward + backward sweep, per op kind, from the tapes:
    conv segment 2 R N Ktot; transposed (data-gradient) segment 2 x the MACs of the conv it differentiates
    (the gather also visits stride-masked taps — those are not counted); WGRAD 2 R N M.
    Totals 8 MACs_fwd per example minus the input layer's two absent terms."""
    out = {}
    for which in (1, 2):
        for op in cn.tapes[which]:
            R = op.n_img * op.OH * op.OW
            if op.kind == nv.OP_IGEMM:
                fl = 0
                for i in range(op.nseg):
                    sg = op.seg[i]
                    if sg.mode == 0:
                        fl += 2 * R * op.N * sg.KH * sg.KW * sg.C
                    else:
                        fl += 2 * op.n_img * sg.IH * sg.IW * sg.C * sg.KH * sg.KW * op.N
                out[nv.OP_IGEMM] = out.get(nv.OP_IGEMM, 0) + fl
            elif op.kind == nv.OP_WGRAD:
                out[nv.OP_WGRAD] = out.get(nv.OP_WGRAD, 0) + 2 * R * op.N * op.M
    return out


def tape_executed_flops_per_probe(cn: CompiledNet):
    """Matrix-pipe FLOPs the kernels EXECUTE for one probe's sweep when the Winograd route is on: the ops that
    csrc/lip_mfma.hip sends to igemm_wino_kernel / wgrad_wino_kernel (3x3, stride 1, pad 1, channel counts multiples
    of 32, even maps) multiply 16 times per 2x2 output patch and (c, n)
    instead of 36 — 4/9 of the algorithmic count (padded tile blocks not counted); every other op executes its
    algorithmic FLOPs.  The utilisation of the f32 MFMA pipe follows from THIS count; `tape_flops_per_probe` stays the
    algorithmic figure the throughput is quoted in."""
    out = {}
    for which in (1, 2):
        for op in cn.tapes[which]:
            R = op.n_img * op.OH * op.OW
            even = op.OH % 2 == 0 and op.OW % 2 == 0
            if op.kind == nv.OP_IGEMM:
                segs = [op.seg[i] for i in range(op.nseg)]
                wino = (even and op.N % 32 == 0 and op.N >= 32 and
                        all(sg.KH == 3 and sg.KW == 3 and sg.stride == 1 and sg.pad_h == 1 and sg.pad_w == 1 and
                            sg.C % 32 == 0 and sg.IH == op.OH and sg.IW == op.OW for sg in segs))
                fl = 0
                for sg in segs:
                    if sg.mode == 0:
                        fl += 2 * R * op.N * sg.KH * sg.KW * sg.C
                    else:
                        fl += 2 * op.n_img * sg.IH * sg.IW * sg.C * sg.KH * sg.KW * op.N
                out[nv.OP_IGEMM] = out.get(nv.OP_IGEMM, 0) + (fl * 4 // 9 if wino else fl)
            elif op.kind == nv.OP_WGRAD:
                sg = op.seg[0]
                wino = (even and op.N % 32 == 0 and sg.C % 32 == 0 and sg.KH == 3 and sg.KW == 3 and
                        sg.stride == 1 and sg.pad_h == 1 and sg.pad_w == 1 and sg.IH == op.OH and sg.IW == op.OW)
                fl = 2 * R * op.N * op.M
                out[nv.OP_WGRAD] = out.get(nv.OP_WGRAD, 0) + (fl * 4 // 9 if wino else fl)
    return out


class LinearizedNet:
    """The linearised-network operator bound to (network, theta_MAP, data slice Z) on one GPU.

    Block operators on (P, D) row-major float32 device tensors:
      ``ggn_vp(V, scale, alpha)`` -> (P, D)      Y = scale * sum_i J_i^T H_i J_i V + alpha V
      ``ggn_vp_diag(V, scale, a)`` -> (P, D)     the same with a (D,) prior-precision vector: ... + a (.) V
      ``jvp(V, mode, c)``         -> (P, n, K)   c * L^T J V   ('lt')   or   J V   ('raw')
      ``vjp(U, mode, c)``         -> (P, D)      J^T (c * L U) ('l')    or   J^T U ('raw')
    """

    def __init__(self, state, Z: torch.Tensor, model_type: Optional[str] = None, device=None,
                 workspace_bytes: int = 8 << 30, max_chunk: int = 1024, work: Optional[torch.Tensor] = None):
        net = getattr(state, "net", None)
        if net is None:
            raise TypeError("the HIP engine needs state.net (a NetSpec layer program); an opaque apply_fn cannot "
                            "be differentiated by hand-written kernels, and there is no CPU fallback")
        if Z.shape[0] == 0:
            raise ValueError("empty data block: the engine needs at least one example (an empty sum is the zero operator)")
        self.lib = nv.load()
        if not torch.cuda.is_available():
            raise nv.NativeError("no GPU: the product path has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda")
        if model_type is not None:
            net.model_type = model_type
        self.n = int(Z.shape[0])
        self.cn = compile_net(net, self.n, state.params)
        cn = self.cn
        self.D, self.K = cn.D, cn.K
        f32 = dict(device=self.device, dtype=torch.float32)
        from .utils import flatten_nn_params
        flat, _ = flatten_nn_params(state.params)
        self.theta = flat.detach().to(**f32).contiguous()
        self.consts = build_consts(cn, state.params, state.batch_stats, self.device)
        self.prim = torch.zeros(cn.prim_floats, **f32)
        nin = self.n * net.tensors[0][0] * net.tensors[0][1] * net.tensors[0][2]
        self.prim[cn.input_off:cn.input_off + nin] = net.prepare_input(Z.detach().to(**f32)).reshape(-1)
        if work is not None:
            # a probe workspace shared with other engines on the same stream (ExampleChunkedGGN: the chunks of a large
            # data set run one after the other, so one workspace serves them all)
            if not (work.is_cuda and work.dtype == torch.float32 and work.is_contiguous()) or work.numel() < cn.work_pp:
                raise ValueError("shared workspace must be a contiguous float32 device tensor of >= work_pp floats")
            chunk = int(min(max_chunk, work.numel() // cn.work_pp))
            self.work = work
        else:
            chunk = int(max(1, min(max_chunk, workspace_bytes // (4 * cn.work_pp))))
            self.work = torch.empty(cn.work_pp * chunk, **f32)
        self.chunk = chunk
        h = C.c_void_p()
        nv.check(self.lib.lip_engine_create(C.byref(h), cn.D, self.n, cn.K), "lip_engine_create")
        self.h = h
        self._scratches = {}
        self._tapes = []
        for which, tape in enumerate(cn.tapes):
            arr = (nv.Op * len(tape))(*tape)
            self._tapes.append(arr)
            nv.check(self.lib.lip_engine_set_tape(h, which, arr, len(tape)), "lip_engine_set_tape")
        nv.check(self.lib.lip_engine_bind(h, nv.ptr(self.theta), nv.ptr(self.consts), nv.ptr(self.prim),
                                          nv.ptr(self.work), cn.work_pp, chunk), "lip_engine_bind")
        nv.check(self.lib.lip_engine_primal(h, nv.stream_ptr()), "lip_engine_primal")

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.lib.lip_engine_destroy(h)
            except Exception:
                pass
            self.h = None

    # -------------------------------------------------------------------------------- helpers
    def _block(self, V: torch.Tensor, width: int) -> torch.Tensor:
        if V.dim() == 1:
            V = V[None]
        if V.shape[-1] != width:
            raise ValueError(f"expected trailing dimension {width}, got {tuple(V.shape)}")
        return V.reshape(-1, width).to(device=self.device, dtype=torch.float32).contiguous()

    def _cotangents(self, U: torch.Tensor, mode: str, strict: bool = False):
        """(P, n K) device block of the head cotangents U, and the head constant of ``mode`` (``strict``: 'l' or 'raw')"""
        if strict and mode not in ("l", "raw"):
            raise ValueError("mode must be 'l' or 'raw'")
        Ub = U.reshape(-1, self.n * self.K).to(device=self.device, dtype=torch.float32).contiguous()
        return Ub, (nv.HEAD_L if mode == "l" else nv.HEAD_IN)

    def _scratch(self, query: str) -> torch.Tensor:
        """scratch of a square-accumulating sweep: allocated once, sized for the probe chunk by its ``*_scratch`` query"""
        scratch = self._scratches.get(query)
        if scratch is None:
            floats = C.c_int64(0)
            nv.check(getattr(self.lib, query)(self.h, int(self.chunk), C.byref(floats)), query)
            scratch = self._scratches[query] = torch.empty(max(1, floats.value), device=self.device, dtype=torch.float32)
        return scratch

    def outputs(self) -> torch.Tensor:
        """primal network outputs f(z_i; theta) (n, K)"""
        o = self.cn.a_off[self.cn.net.out]
        return self.prim[o:o + self.n * self.K].reshape(self.n, self.K).clone()

    def probs(self) -> torch.Tensor:
        o = self.cn.prob_off
        return self.prim[o:o + self.n * self.K].reshape(self.n, self.K).clone()

    def last_layer(self) -> Tuple[int, int, int]:
        """``(offset, F, K)`` of the final Dense layer (:meth:`CompiledNet.last_layer`)"""
        return self.cn.last_layer()

    def features(self) -> torch.Tensor:
        """(n, F) penultimate activations phi_i, the input of the final Dense, read from the cached primal pass; for a
        Dense on a feature map (``flat_kernel``) the flattened (h w c) source tensor, contiguous in ``prim`` already"""
        _, F, _ = self.cn.last_layer()
        o = self.cn.a_off[self.cn.last_unit().src]
        return self.prim[o:o + self.n * F].reshape(self.n, F).clone()

    def last_layer_ggn(self, out: torch.Tensor) -> torch.Tensor:
        """ADD sum_i phit_i phit_i^T (x) H_i of this binding's examples into ``out`` (DL, DL) float64, DL = (F + 1) K:
        the GGN block of theta_L = [bias, kernel] of the final Dense (``lip_ll_ggn``), H_i = diag(p_i) - p_i p_i^T for
        the classifier and I for the regressor, from the cached features and probabilities: no backward sweep, no
        per-example rows, bitwise reproducible and exactly symmetric."""
        _, F, K = self.cn.last_layer()
        DL = (F + 1) * K
        if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (DL, DL)):
            raise ValueError(f"out must be a contiguous float64 device matrix of {DL} x {DL}")
        scratch = self._scratches.get("lip_ll_ggn_scratch")
        if scratch is None:
            doubles = C.c_int64(0)
            nv.check(self.lib.lip_ll_ggn_scratch(self.n, F, K, C.byref(doubles)), "lip_ll_ggn_scratch")
            scratch = self._scratches["lip_ll_ggn_scratch"] = torch.empty(max(1, doubles.value), device=self.device,
                                                                          dtype=torch.float64)
        cn = self.cn
        phi = self.prim[cn.a_off[cn.last_unit().src]:]
        pr = self.prim[cn.prob_off:] if cn.classifier else None
        nv.check(self.lib.lip_ll_ggn(phi.data_ptr(), F, 0 if pr is None else pr.data_ptr(), self.n, F, K, out.data_ptr(),
                                     scratch.data_ptr(), scratch.numel(), nv.stream_ptr()), "lip_ll_ggn")
        return out

    def last_layer_kron_factors(self, A: torch.Tensor, Bf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """ADD this binding's examples into the two Kronecker factors of the last-layer curvature
        (``lip_ll_kron_factors``): A (F + 1, F + 1) += sum_i phit_i phit_i^T and Bf (K, K) += sum_i diag(p_i) - p_i p_i^T
        for the classifier, n I for the regressor; both float64, from the cached features and probabilities, bitwise
        reproducible and exactly symmetric."""
        _, F, K = self.cn.last_layer()
        for name, t, d in (("A", A, F + 1), ("Bf", Bf, K)):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (d, d)):
                raise ValueError(f"{name} must be a contiguous float64 device matrix of {d} x {d}")
        scratch = self._scratches.get("lip_ll_kron_factors_scratch")
        if scratch is None:
            doubles = C.c_int64(0)
            nv.check(self.lib.lip_ll_kron_factors_scratch(self.n, F, K, C.byref(doubles)), "lip_ll_kron_factors_scratch")
            scratch = self._scratches["lip_ll_kron_factors_scratch"] = torch.empty(max(1, doubles.value), device=self.device,
                                                                                   dtype=torch.float64)
        cn = self.cn
        phi = self.prim[cn.a_off[cn.last_unit().src]:]
        pr = self.prim[cn.prob_off:] if cn.classifier else None
        nv.check(self.lib.lip_ll_kron_factors(phi.data_ptr(), F, 0 if pr is None else pr.data_ptr(), self.n, F, K,
                                              A.data_ptr(), Bf.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                              nv.stream_ptr()), "lip_ll_kron_factors")
        return A, Bf

    # ------------------------------------------------------------------------------ subnetwork
    ROW_BLOCK_BYTES = 2 << 30          # cap of a (P, n, D) float32 row block: the rule of ggn.materialize_factor

    def _sub_index(self, idx: torch.Tensor) -> torch.Tensor:
        """(S,) contiguous device int64 copy of ``idx``, checked against [0, D) before any launch"""
        idx = torch.as_tensor(idx).reshape(-1)
        if idx.numel() == 0 or idx.dtype not in (torch.int64, torch.int32):
            raise ValueError("idx must be a non-empty integer index tensor")
        if int(idx.min()) < 0 or int(idx.max()) >= self.D:
            raise ValueError(f"idx must lie in [0, {self.D})")
        return idx.to(device=self.device, dtype=torch.int64).contiguous()

    def _sub_scratch(self, query: str, *shape: int) -> torch.Tensor:
        """float64 scratch of ``lip_sub_gram`` / ``lip_sub_predict``: one buffer per query, kept and grown on demand"""
        doubles = C.c_int64(0)
        nv.check(getattr(self.lib, query)(*[int(s) for s in shape], C.byref(doubles)), query)
        scratch = self._scratches.get(query)
        if scratch is None or scratch.numel() < doubles.value:
            scratch = self._scratches[query] = torch.empty(max(1, doubles.value), device=self.device, dtype=torch.float64)
        return scratch

    def _class_blocks(self, class_chunk: Optional[int]):
        """(k0, k1) class blocks whose (k1 - k0, n, D) float32 rows stay under ``ROW_BLOCK_BYTES``"""
        pc = max(1, min(self.K, (self.ROW_BLOCK_BYTES // (4 * self.D)) // self.n))
        if class_chunk is not None:
            if class_chunk < 1:
                raise ValueError("class_chunk must be positive")
            pc = min(pc, int(class_chunk))
        return [(k0, min(self.K, k0 + pc)) for k0 in range(0, self.K, pc)]

    def _one_hot_rows(self, k0: int, k1: int, mode: str) -> torch.Tensor:
        """(k1 - k0, n, D) rows of :meth:`vjp_rows` for the probes e_k, k0 <= k < k1, on every example"""
        E = torch.eye(self.K, device=self.device, dtype=torch.float32)[k0:k1, None, :].expand(k1 - k0, self.n, self.K)
        return self.vjp_rows(E.contiguous(), mode)

    def subnetwork_gram(self, idx: torch.Tensor, out: torch.Tensor, class_chunk: Optional[int] = None) -> torch.Tensor:
        """ADD sum_i (J_i^T H_i J_i)[idx][:, idx] of this binding's examples into ``out`` (S, S) float64: the GGN block
        over the flat-parameter indices ``idx``.  One-hot probes e_k on every example go through :meth:`vjp_rows` ('l') in
        class blocks whose (Pc, n, D) float32 rows stay under 2 GiB (``class_chunk`` caps Pc further); each block's
        rows are gathered to a compact (Pc n, S) panel and Gram-multiplied in float64 (``lip_sub_gram``): bitwise
        reproducible and exactly symmetric."""
        idx = self._sub_index(idx)
        S = idx.numel()
        if not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (S, S)):
            raise ValueError(f"out must be a contiguous float64 device matrix of {S} x {S}")
        for k0, k1 in self._class_blocks(class_chunk):
            rows = self._one_hot_rows(k0, k1, "l")
            R = (k1 - k0) * self.n
            scratch = self._sub_scratch("lip_sub_gram_scratch", R, S)
            nv.check(self.lib.lip_sub_gram(rows.data_ptr(), self.D, self.D, R, idx.data_ptr(), S, out.data_ptr(),
                                           scratch.data_ptr(), scratch.numel(), nv.stream_ptr()), "lip_sub_gram")
        return out

    def subnetwork_predict(self, idx: torch.Tensor, Sigma: torch.Tensor, diag: bool = False,
                           class_chunk: Optional[int] = None) -> torch.Tensor:
        """J_S(x) Sigma J_S(x)^T for every point of this binding, J_S the Jacobian columns ``idx``: (n, K, K) float64, or
        (n, K) for ``diag`` (``lip_sub_predict`` on the 'raw' rows of :meth:`vjp_rows`).  The diag form runs in class
        blocks like :meth:`subnetwork_gram`.  The full form needs all K rows of a point at once: when the (K, n, D)
        float32 rows exceed 2 GiB it runs in chunks of points, and when the K rows of ONE point exceed it, it raises
        ``ValueError`` before allocating."""
        idx = self._sub_index(idx)
        S, K, n = idx.numel(), self.K, self.n
        if not (Sigma.is_cuda and Sigma.dtype == torch.float64 and Sigma.is_contiguous() and tuple(Sigma.shape) == (S, S)):
            raise ValueError(f"Sigma must be a contiguous float64 device matrix of {S} x {S}")
        if diag:
            blocks = self._class_blocks(class_chunk)
        else:
            fit = (self.ROW_BLOCK_BYTES // (4 * self.D)) // K
            if fit < 1:
                raise ValueError(f"the full predictive needs the K = {K} Jacobian rows of a point at once: {K} x {self.D} "
                                 f"floats exceed the row-block cap (use diag)")
            blocks = [(0, K)]
        out = torch.empty((n, K) if diag else (n, K, K), device=self.device, dtype=torch.float64)
        if not diag and fit < n:
            # the rows of all n points do not fit: chunks of `fit` points, each assembled from class-block sweeps (a sweep
            # always covers every bound example, so the sweeps repeat per point chunk: bind fewer points to avoid it)
            for b0 in range(0, n, fit):
                b1 = min(n, b0 + fit)
                Jr = torch.empty(K, b1 - b0, self.D, device=self.device, dtype=torch.float32)
                for k0, k1 in self._class_blocks(class_chunk):
                    Jr[k0:k1] = self._one_hot_rows(k0, k1, "raw")[:, b0:b1]
                scratch = self._sub_scratch("lip_sub_predict_scratch", b1 - b0, K, S)
                nv.check(self.lib.lip_sub_predict(Jr.data_ptr(), self.D, self.D, b1 - b0, K, idx.data_ptr(), S,
                                                  Sigma.data_ptr(), out[b0:b1].data_ptr(), 0, scratch.data_ptr(),
                                                  scratch.numel(), nv.stream_ptr()), "lip_sub_predict")
            return out
        for k0, k1 in blocks:
            rows = self._one_hot_rows(k0, k1, "raw")
            Kc = k1 - k0
            scratch = self._sub_scratch("lip_sub_predict_scratch", n, Kc, S)
            part = out if Kc == K else torch.empty(n, Kc, device=self.device, dtype=torch.float64)
            nv.check(self.lib.lip_sub_predict(rows.data_ptr(), self.D, self.D, n, Kc, idx.data_ptr(), S, Sigma.data_ptr(),
                                              part.data_ptr(), int(diag), scratch.data_ptr(), scratch.numel(),
                                              nv.stream_ptr()), "lip_sub_predict")
            if part is not out:
                out[:, k0:k1] = part
        return out

    # ------------------------------------------------------------------------------ Kronecker factors of every layer
    KFAC_SCRATCH_BYTES = 1 << 30       # cap of the float64 scratch of one lip_kfac_predict call (it chunks the points)

    def kfac_blocks(self) -> List[KfacBlock]:
        """The layer blocks of this binding (:func:`kfac_block_table`) with the BN scale slice in ``consts`` and the
        offset of every block's input tensor in ``prim`` filled in."""
        blocks = getattr(self, "_kfac_blocks", None)
        if blocks is None:
            cn = self.cn
            blocks = kfac_block_table(cn.net, cn.offsets)
            for b in blocks:
                b.src = cn.a_off[b.unit.src]
                if b.unit.bn_scale is not None:
                    b.bn = (cn.meta["s_off"][b.unit.dst], b.N)
            self._kfac_blocks = blocks
        return blocks

    def _f64_scratch(self, name: str, doubles: int) -> torch.Tensor:
        scratch = self._scratches.get(name)
        if scratch is None or scratch.numel() < doubles:
            scratch = self._scratches[name] = torch.empty(max(1, int(doubles)), device=self.device, dtype=torch.float64)
        return scratch

    def kfac_input_grams(self, As: List[torch.Tensor]) -> List[torch.Tensor]:
        """ADD A_l += sum_i sum_t at_{i,t} at_{i,t}^T of this binding's examples into every (Mt, Mt) float64 matrix of
        ``As``: one ``lip_kfac_input_gram`` per block on the cached primal activations."""
        tens = self.cn.net.tensors
        for b, A in zip(self.kfac_blocks(), As):
            u = b.unit
            ih, iw, _ = tens[u.src]
            oh, ow, _ = tens[u.dst]
            geom = (self.n, ih, iw, u.cin, u.kh, u.kw, u.stride, u.pad_h, u.pad_w, oh, ow, int(b.bias))
            doubles = C.c_int64(0)
            nv.check(self.lib.lip_kfac_input_gram_scratch(*geom, C.byref(doubles)), "lip_kfac_input_gram_scratch")
            scratch = self._f64_scratch("lip_kfac_input_gram", doubles.value)
            nv.check(self.lib.lip_kfac_input_gram(self.prim[b.src:].data_ptr(), *geom, A.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), nv.stream_ptr()), "lip_kfac_input_gram")
        return As

    def kfac_output_grams(self, Ss: List[torch.Tensor], class_chunk: Optional[int] = None,
                          probes: Optional[torch.Tensor] = None, divisor: float = 1.0) -> List[torch.Tensor]:
        """ADD S_l += sum_i sum_t sum_k g_{i,t,k} g_{i,t,k}^T into every (N, N) float64 matrix of ``Ss``: one
        ``lip_vjp_kron`` sweep ('l') over the one-hot probes, in the class blocks of :meth:`_class_blocks`; the frozen BN
        scale s s^T o S_l is applied here, in float64, to this binding's sums before they are added.  ``probes``: a raw
        (P, n, K) block of head cotangents swept instead ('raw'), in probe chunks under the same byte cap, its sums divided by
        ``divisor`` before they are added (``fisher.py``)."""
        blocks = self.kfac_blocks()
        cap = len(blocks)
        koff, ooff, Ns = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
        count, total = C.c_int32(0), C.c_int64(0)
        nv.check(self.lib.lip_vjp_kron_layout(self.h, cap, koff, ooff, Ns, C.byref(count), C.byref(total)), "lip_vjp_kron_layout")
        where = {int(koff[i]): (int(ooff[i]), int(Ns[i])) for i in range(min(cap, count.value))}
        if count.value != cap or any(b.kernel_off not in where or where[b.kernel_off][1] != b.N for b in blocks):
            raise nv.NativeError("lip_vjp_kron_layout: the backward tape's weight gradients do not match the layer blocks")
        buf = torch.zeros(total.value, device=self.device, dtype=torch.float64)
        if probes is None:
            eye = torch.eye(self.K, device=self.device, dtype=torch.float32)
            sweeps = ((eye[k0:k1, None, :].expand(k1 - k0, self.n, self.K).contiguous(), nv.HEAD_L)
                      for k0, k1 in self._class_blocks(class_chunk))
        else:
            Ub, head = self._cotangents(probes, "raw")
            pc = max(1, (self.ROW_BLOCK_BYTES // (4 * self.D)) // self.n)        # the cap of _class_blocks, not cut at K
            pc = pc if class_chunk is None else max(1, min(pc, int(class_chunk)))
            sweeps = ((Ub[p0:p0 + pc], head) for p0 in range(0, Ub.shape[0], pc))
        for E, head in sweeps:
            doubles = C.c_int64(0)                     # for the probes this call passes: the need is not monotone in them
            nv.check(self.lib.lip_vjp_kron_scratch(self.h, E.shape[0], C.byref(doubles)), "lip_vjp_kron_scratch")
            scratch = self._f64_scratch("lip_vjp_kron", doubles.value)
            nv.check(self.lib.lip_vjp_kron(self.h, nv.ptr(E), buf.data_ptr(), E.shape[0], head, 1.0, scratch.data_ptr(),
                                           scratch.numel(), nv.stream_ptr()), "lip_vjp_kron")
        for b, S in zip(blocks, Ss):
            o, N = where[b.kernel_off]
            part = buf[o:o + N * N].reshape(N, N)
            if b.bn is not None:
                s = self.consts[b.bn[0]:b.bn[0] + N].double()
                part = part * (s[:, None] * s[None, :])            # the outer product first: exactly symmetric
            if probes is not None and divisor != 1.0:
                part = part / float(divisor)
            S += part
        return Ss

    def kfac_factors(self, As: List[torch.Tensor], Ss: List[torch.Tensor], class_chunk: Optional[int] = None,
                     probes: Optional[torch.Tensor] = None, divisor: float = 1.0):
        """ADD this binding's examples into the Kronecker factors of every layer block (:meth:`kfac_blocks` order):
        ``As[l]`` (Mt, Mt) and ``Ss[l]`` (N, N), contiguous float64 device matrices; unscaled.  ``probes`` / ``divisor``
        go to :meth:`kfac_output_grams`; the input factors do not depend on them."""
        blocks = self.kfac_blocks()
        if len(As) != len(blocks) or len(Ss) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} matrices in As and in Ss")
        for b, A, S in zip(blocks, As, Ss):
            for name, t, d in (("A", A, b.Mt), ("S", S, b.N)):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (d, d)):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{d} x {d}")
        self.kfac_input_grams(As)
        self.kfac_output_grams(Ss, class_chunk=class_chunk, probes=probes, divisor=divisor)
        return As, Ss

    def _kfac_predict_rows(self, rows: torch.Tensor, B: int, Kc: int, fits, rem, out: torch.Tensor, diag: bool) -> None:
        """add every block's and the remainder's term of the (Kc, B, D) float32 rows into ``out``"""
        for b, (V, R, Ub) in zip(self.kfac_blocks(), fits):
            doubles = C.c_int64(0)
            nv.check(self.lib.lip_kfac_predict_scratch(B, Kc, b.Mt, b.N, C.byref(doubles)), "lip_kfac_predict_scratch")
            one = 2 * Kc * b.Mt * b.N
            scratch = self._f64_scratch("lip_kfac_predict", min(doubles.value, max(one, self.KFAC_SCRATCH_BYTES // 8)))
            nv.check(self.lib.lip_kfac_predict(rows.data_ptr(), self.D, B, Kc, b.off, b.Mt, b.N, V.data_ptr(), Ub.data_ptr(),
                                               R.data_ptr(), out.data_ptr(), int(diag), scratch.data_ptr(), scratch.numel(),
                                               nv.stream_ptr()), "lip_kfac_predict")
        idx, var = rem
        if idx.numel():
            Jd = rows[:, :, idx].double()                                                  # (Kc, B, r)
            dg = (Jd * Jd * var).sum(-1).T                                                  # (B, Kc)
            if diag:
                out += dg
            else:
                # symmetrised, and its diagonal the expression of the diag form: the two forms agree bitwise there
                full = torch.einsum("kbd,d,mbd->bkm", Jd, var, Jd)
                full = 0.5 * (full + full.transpose(1, 2))
                k = torch.arange(Kc, device=full.device)
                full[:, k, k] = dg
                out += full

    def kfac_predict(self, fits, rem, diag: bool = False, class_chunk: Optional[int] = None) -> torch.Tensor:
        """J(x) Sigma J(x)^T for every point of this binding under the Kronecker-factored posterior: (n, K, K) float64,
        or (n, K) for ``diag``.  ``fits`` holds (V, R, Ub) of every layer block in :meth:`kfac_blocks` order (contiguous
        float64 device matrices), ``rem`` = (indices, variances) of the parameters outside every block, whose term
        sum_d J_d^2 var_d is formed in float64 torch.  The blocks go through ``lip_kfac_predict`` on the 'raw' rows of
        :meth:`vjp_rows`, with the row-block cap and the refusals of :meth:`subnetwork_predict`."""
        blocks = self.kfac_blocks()
        if len(fits) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} fitted factor triples")
        for b, (V, R, Ub) in zip(blocks, fits):
            for name, t, shape in (("V", V, (b.Mt, b.Mt)), ("R", R, (b.Mt, b.N)), ("Ub", Ub, (b.N, b.N))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{shape[0]} x {shape[1]}")
        rem = (rem[0].to(self.device), rem[1].to(device=self.device, dtype=torch.float64))
        K, n = self.K, self.n
        if diag:
            out = torch.zeros(n, K, device=self.device, dtype=torch.float64)
            for k0, k1 in self._class_blocks(class_chunk):
                Kc = k1 - k0
                part = out if Kc == K else torch.zeros(n, Kc, device=self.device, dtype=torch.float64)
                self._kfac_predict_rows(self._one_hot_rows(k0, k1, "raw"), n, Kc, fits, rem, part, True)
                if part is not out:
                    out[:, k0:k1] = part
            return out
        fit = (self.ROW_BLOCK_BYTES // (4 * self.D)) // K
        if fit < 1:
            raise ValueError(f"the full predictive needs the K = {K} Jacobian rows of a point at once: {K} x {self.D} "
                             f"floats exceed the row-block cap (use diag)")
        out = torch.zeros(n, K, K, device=self.device, dtype=torch.float64)
        if fit >= n:
            self._kfac_predict_rows(self._one_hot_rows(0, K, "raw"), n, K, fits, rem, out, False)
            return out
        # the rows of all n points do not fit: chunks of `fit` points, as in subnetwork_predict
        for b0 in range(0, n, fit):
            b1 = min(n, b0 + fit)
            Jr = torch.empty(K, b1 - b0, self.D, device=self.device, dtype=torch.float32)
            for k0, k1 in self._class_blocks(class_chunk):
                Jr[k0:k1] = self._one_hot_rows(k0, k1, "raw")[:, b0:b1]
            self._kfac_predict_rows(Jr, b1 - b0, K, fits, rem, out[b0:b1], False)
        return out

    KFAC_GRID_MAX = 32                 # LIP_GRID_MAX: the scales of one lip_kfac_predict_grid call

    def kfac_predict_grid(self, bases, Evs: List[torch.Tensor], rem, scales, class_chunk: Optional[int] = None) -> torch.Tensor:
        """The marginal variances of :meth:`kfac_predict` (``diag``) at the priors s_g a for every s_g of ``scales``, a
        the prior of the fit: (G, n, K) float64 from ONE pass over the Jacobian rows.  ``bases[l] = (V, Ub)`` and
        ``Evs[l]`` (Mt, N) are the fitted eigenbasis and the eigenvalues in the whitened basis of every layer block
        (:meth:`kfac_blocks` order; contiguous float64 device matrices; R = 1 / (Ev + 1) at the fit), so that slice g is
        sum_{j,l} T[j][l]^2 / (Ev[j][l] + s_g) per block (``lip_kfac_predict_grid``, at most 32 scales per call; more
        go through it in groups of 32).  ``rem`` = (indices, a_rem, h_rem): the parameters outside every block, their
        prior precisions at the fit and their curvature; their term (J_d^2) @ (1 / (s_g a + h))^T is float64 torch.  The
        class blocks, the row-block cap and the ``KFAC_SCRATCH_BYTES`` cap are those of :meth:`kfac_predict`."""
        blocks = self.kfac_blocks()
        if len(bases) != len(blocks) or len(Evs) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} (V, Ub) pairs and {len(blocks)} matrices in Evs")
        for b, (V, Ub), Ev in zip(blocks, bases, Evs):
            for name, t, shape in (("V", V, (b.Mt, b.Mt)), ("Ub", Ub, (b.N, b.N)), ("Ev", Ev, (b.Mt, b.N))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{shape[0]} x {shape[1]}")
        s = torch.as_tensor(scales, dtype=torch.float64).reshape(-1).cpu()
        if s.numel() < 1 or not bool((torch.isfinite(s) & (s > 0)).all()):
            raise ValueError("scales must be one or more finite positive numbers")
        idx = rem[0].to(self.device)
        a_rem, h_rem = (t.to(device=self.device, dtype=torch.float64) for t in rem[1:])
        G, K, n = s.numel(), self.K, self.n
        w_rem = 1.0 / (s.to(self.device)[:, None] * a_rem[None, :] + h_rem[None, :]) if idx.numel() else None   # (G, r)
        out = torch.zeros(G, n, K, device=self.device, dtype=torch.float64)
        for k0, k1 in self._class_blocks(class_chunk):
            Kc = k1 - k0
            rows = self._one_hot_rows(k0, k1, "raw")
            part = out if Kc == K else torch.zeros(G, n, Kc, device=self.device, dtype=torch.float64)
            for g0 in range(0, G, self.KFAC_GRID_MAX):
                Gc = min(self.KFAC_GRID_MAX, G - g0)
                sc = (C.c_double * Gc)(*s[g0:g0 + Gc].tolist())
                dst = part[g0:g0 + Gc]                                                       # contiguous (Gc, n, Kc)
                for b, (V, Ub), Ev in zip(blocks, bases, Evs):
                    doubles = C.c_int64(0)
                    nv.check(self.lib.lip_kfac_predict_grid_scratch(n, Kc, b.Mt, b.N, Gc, C.byref(doubles)),
                             "lip_kfac_predict_grid_scratch")
                    tiles = ((b.Mt + 31) // 32) * ((b.N + 31) // 32)
                    one = Gc * b.Mt * b.N + Kc * (b.Mt * b.N + tiles * Gc)
                    scratch = self._f64_scratch("lip_kfac_predict_grid",
                                                min(doubles.value, max(one, self.KFAC_SCRATCH_BYTES // 8)))
                    nv.check(self.lib.lip_kfac_predict_grid(rows.data_ptr(), self.D, n, Kc, b.off, b.Mt, b.N, V.data_ptr(),
                                                            Ub.data_ptr(), Ev.data_ptr(), sc, Gc, dst.data_ptr(),
                                                            scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
                             "lip_kfac_predict_grid")
            if w_rem is not None:
                Jd = rows[:, :, idx].double()                                               # (Kc, n, r)
                part += ((Jd * Jd) @ w_rem.T).permute(2, 1, 0)                              # (Kc, n, G) -> (G, n, Kc)
            del rows                                                                        # before the next block's rows
            if part is not out:
                out[:, :, k0:k1] = part
        return out

    def kfac_eigen_sqsums(self, bases, Lams: List[torch.Tensor], class_chunk: Optional[int] = None) -> List[torch.Tensor]:
        """ADD Lam_l[j][m] += sum_i sum_k ((V_l^T mat_l(J_i^T L_i e_k) Ub_l)[j][m])^2 of this binding's examples into every
        (Mt, N) float64 matrix of ``Lams``: the second moments of the per-example factor rows in the eigenbasis
        ``bases[l] = (V, Ub)`` of every layer block (:meth:`kfac_blocks` order; contiguous float64 device matrices), what
        EKFAC puts in place of KFAC's eigenvalue products.  One-hot probes on every example go through :meth:`vjp_rows`
        ('l') in the class blocks of :meth:`_class_blocks`, each block's rows once for all layer blocks
        (``lip_kfac_eigen_sqsum``; its scratch is capped by ``KFAC_SCRATCH_BYTES``, under which it chunks the rows)."""
        blocks = self.kfac_blocks()
        if len(bases) != len(blocks) or len(Lams) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} (V, Ub) pairs in bases and {len(blocks)} matrices in Lams")
        for b, (V, Ub), Lam in zip(blocks, bases, Lams):
            for name, t, shape in (("V", V, (b.Mt, b.Mt)), ("Ub", Ub, (b.N, b.N)), ("Lam", Lam, (b.Mt, b.N))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{shape[0]} x {shape[1]}")
        for k0, k1 in self._class_blocks(class_chunk):
            rows = self._one_hot_rows(k0, k1, "l")
            R = (k1 - k0) * self.n
            for b, (V, Ub), Lam in zip(blocks, bases, Lams):
                doubles = C.c_int64(0)
                nv.check(self.lib.lip_kfac_eigen_sqsum_scratch(R, b.Mt, b.N, C.byref(doubles)), "lip_kfac_eigen_sqsum_scratch")
                # the doubles asked for, not the buffer's (it may have grown): the row chunks, and with them the order of
                # the sums, depend on the binding alone
                need = min(doubles.value, max(2 * b.Mt * b.N, self.KFAC_SCRATCH_BYTES // 8))
                scratch = self._f64_scratch("lip_kfac_eigen_sqsum", need)
                nv.check(self.lib.lip_kfac_eigen_sqsum(rows.data_ptr(), self.D, R, b.off, b.Mt, b.N, V.data_ptr(), Ub.data_ptr(),
                                                       Lam.data_ptr(), scratch.data_ptr(), need, nv.stream_ptr()),
                         "lip_kfac_eigen_sqsum")
        return Lams

    def kfac_eigen_sqsums_sweep(self, bases, Lams: List[torch.Tensor], class_chunk: Optional[int] = None,
                                probes: Optional[torch.Tensor] = None, divisor: float = 1.0) -> List[torch.Tensor]:
        """:meth:`kfac_eigen_sqsums` from backward sweeps instead of factor rows (``lip_vjp_eigen``): the block's slice of
        a row is the per-example weight gradient At_i^T G_i diag(s), so V^T mat_l(.) Ub = (At_i V)^T (G_i diag(s) Ub) and
        every WGRAD op of the sweep projects its patches and its cotangent rows and square-sums the per-(probe, example)
        products of the pair; no D-wide row exists.  Same operand checks and the same ADD into ``Lams``; the frozen BN
        scale of a block is folded into its Ub here, in float64.  The probes are chunked as in
        :meth:`kfac_output_grams`: one-hot 'l' probes in class blocks, or a raw (P, n, K) block ``probes`` whose sums
        are divided by ``divisor`` before they are added (``fisher.py``).  The sums of a sweep are float32 (those of
        ``lip_vjp_sqsum``), added to ``Lams`` in float64 pass by pass."""
        blocks = self.kfac_blocks()
        if len(bases) != len(blocks) or len(Lams) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} (V, Ub) pairs in bases and {len(blocks)} matrices in Lams")
        for b, (V, Ub), Lam in zip(blocks, bases, Lams):
            for name, t, shape in (("V", V, (b.Mt, b.Mt)), ("Ub", Ub, (b.N, b.N)), ("Lam", Lam, (b.Mt, b.N))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{shape[0]} x {shape[1]}")
        cap = len(blocks)
        koff, ooff, Ns = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
        count, total = C.c_int32(0), C.c_int64(0)
        nv.check(self.lib.lip_vjp_kron_layout(self.h, cap, koff, ooff, Ns, C.byref(count), C.byref(total)), "lip_vjp_kron_layout")
        order = {int(koff[i]): i for i in range(min(cap, count.value))}
        if count.value != cap or any(b.kernel_off not in order or int(Ns[order[b.kernel_off]]) != b.N for b in blocks):
            raise nv.NativeError("lip_vjp_kron_layout: the backward tape's weight gradients do not match the layer blocks")
        divided = probes is not None and divisor != 1.0
        Ubs, outs = [], []
        for b, (V, Ub), Lam in zip(blocks, bases, Lams):
            if b.bn is not None:
                Ub = (self.consts[b.bn[0]:b.bn[0] + b.N].double()[:, None] * Ub).contiguous()
            Ubs.append(Ub)
            outs.append(torch.zeros_like(Lam) if divided else Lam)
        Vp, Up, Lp, Mts = (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_int32 * cap)()
        for b, (V, _), Ub, out in zip(blocks, bases, Ubs, outs):
            k = order[b.kernel_off]
            Vp[k], Up[k], Lp[k], Mts[k] = V.data_ptr(), Ub.data_ptr(), out.data_ptr(), b.Mt
        if probes is None:
            eye = torch.eye(self.K, device=self.device, dtype=torch.float32)
            sweeps = ((eye[k0:k1, None, :].expand(k1 - k0, self.n, self.K).contiguous(), nv.HEAD_L)
                      for k0, k1 in self._class_blocks(class_chunk))
        else:
            U, head = self._cotangents(probes, "raw")
            pc = max(1, (self.ROW_BLOCK_BYTES // (4 * self.D)) // self.n)        # the cap of _class_blocks, not cut at K
            pc = pc if class_chunk is None else max(1, min(pc, int(class_chunk)))
            sweeps = ((U[p0:p0 + pc], head) for p0 in range(0, U.shape[0], pc))
        for E, head in sweeps:
            floats = C.c_int64(0)
            nv.check(self.lib.lip_vjp_eigen_scratch(self.h, E.shape[0], C.byref(floats)), "lip_vjp_eigen_scratch")
            scratch = self._scratches.get("lip_vjp_eigen")
            if scratch is None or scratch.numel() < floats.value:
                scratch = self._scratches["lip_vjp_eigen"] = torch.empty(max(4, floats.value), device=self.device,
                                                                         dtype=torch.float32)
            nv.check(self.lib.lip_vjp_eigen(self.h, nv.ptr(E), Vp, Up, Lp, Mts, cap, E.shape[0], head, 1.0,
                                            scratch.data_ptr(), scratch.numel(), nv.stream_ptr()), "lip_vjp_eigen")
        if divided:
            for Lam, out in zip(Lams, outs):
                Lam += out / float(divisor)
        return Lams

    def kfac_predict_sweep(self, fits, rem, diag: bool = True, class_chunk: Optional[int] = None,
                           probes: Optional[torch.Tensor] = None) -> torch.Tensor:
        """:meth:`kfac_predict` from backward sweeps instead of Jacobian rows (``lip_vjp_eigen_wnorm``): with
        T = V^T mat_l(J_i^T u) Ub = (At_i V)^T (G_i diag(s) Ub) of :meth:`kfac_eigen_sqsums_sweep`,

            u^T J_i Sigma J_i^T u = sum_l sum_{j,m} R_l[j][m] T_l[j][m]^2 + sum_{d in remainder} var_d (J_i^T u)_d^2,

        so every WGRAD op of the sweep projects its patches and its cotangent rows and the weighted-norm kernel of
        :meth:`vjp_wnorm` reduces the per-(probe, example) products of the pair against the block's R; the remainder's
        term is that kernel's own reduction.  No D-wide row and no float64 Mt x N stage exists, so there is no row-block
        cap: the probes go in blocks of ``class_chunk`` (None: all at once; the engine splits them into its passes).
        The working set is the call's scratch instead, kept on the engine: per op the projected patches (n OH OW Mt
        floats) and the projected rows of one pass's probes (P' n OH OW N floats), the largest op counting (609 MiB at
        the CIFAR config with 256 points, 6 GiB at ResNet-50 with K = 1000 probes in one pass; ``class_chunk`` cuts
        the second part).
        Same operands and operand checks as :meth:`kfac_predict`; the BN scale of a block is folded into its Ub in
        float64, R and the remainder's variances are cast to float32 once.  The remainder's variances are scattered into
        a zero (D,) vector, so a bias that a block carries as its row 0 has weight 0 in its own reduction and is counted
        once; a net without a remainder launches no reduction.  ``diag=True``: one-hot 'raw' probes, (n, K) float64.
        ``diag=False``: the K (K + 1) / 2 probes of ``lla.polarisation_probes`` combined in float64, (n, K, K), exactly
        symmetric; K > 32 raises ``ValueError`` before anything runs.  ``probes``: a raw (P, n, K) block of head
        cotangents swept instead; the (P, n) float32 weighted norms come back as they are.  The sums are float32 (those
        of ``lip_vjp_wnorm``), bitwise reproducible for a given chunking."""
        from .lla import POLARISATION_MAX_K, covariance_from_polarisation, polarisation_probes
        blocks = self.kfac_blocks()
        if len(fits) != len(blocks):
            raise ValueError(f"{len(blocks)} layer blocks need {len(blocks)} fitted factor triples")
        for b, (V, R, Ub) in zip(blocks, fits):
            for name, t, shape in (("V", V, (b.Mt, b.Mt)), ("R", R, (b.Mt, b.N)), ("Ub", Ub, (b.N, b.N))):
                if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
                    raise ValueError(f"{name} of the block at offset {b.off} must be a contiguous float64 device matrix of "
                                     f"{shape[0]} x {shape[1]}")
        K, n = self.K, self.n
        if class_chunk is not None and class_chunk < 1:
            raise ValueError("class_chunk must be positive")
        if probes is None and not diag and K > POLARISATION_MAX_K:
            raise ValueError(f"the full predictive takes K (K + 1) / 2 probes per binding: refused for K = {K} > "
                             f"{POLARISATION_MAX_K} outputs (use diag)")
        if probes is not None and (probes.dim() != 3 or tuple(probes.shape[1:]) != (n, K)):
            raise ValueError(f"probes must be a (P, {n}, {K}) block of head cotangents, got {tuple(probes.shape)}")
        idx, var = rem[0].to(self.device), rem[1].to(device=self.device, dtype=torch.float64)
        if idx.numel() != var.numel():
            raise ValueError("the remainder needs one variance per index")
        cap = len(blocks)
        koff, ooff, Ns = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int32 * cap)()
        count, total = C.c_int32(0), C.c_int64(0)
        nv.check(self.lib.lip_vjp_kron_layout(self.h, cap, koff, ooff, Ns, C.byref(count), C.byref(total)), "lip_vjp_kron_layout")
        order = {int(koff[i]): i for i in range(min(cap, count.value))}
        if count.value != cap or any(b.kernel_off not in order or int(Ns[order[b.kernel_off]]) != b.N for b in blocks):
            raise nv.NativeError("lip_vjp_kron_layout: the backward tape's weight gradients do not match the layer blocks")
        keep = []                                                       # the operands the pointer arrays refer to
        Vp, Up, Rp, Mts = (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_void_p * cap)(), (C.c_int32 * cap)()
        for b, (V, R, Ub) in zip(blocks, fits):
            if b.bn is not None:
                Ub = (self.consts[b.bn[0]:b.bn[0] + b.N].double()[:, None] * Ub).contiguous()
            Rw = R.float().contiguous()
            keep.append((V, Ub, Rw))
            k = order[b.kernel_off]
            Vp[k], Up[k], Rp[k], Mts[k] = V.data_ptr(), Ub.data_ptr(), Rw.data_ptr(), b.Mt
        w_rem = None
        if idx.numel():
            w_rem = torch.zeros(self.D, device=self.device, dtype=torch.float32)
            w_rem[idx] = var.float()

        def sweep(E: torch.Tensor, head: int) -> torch.Tensor:
            """(P, n) float32 weighted norms of the (P, n K) cotangents E"""
            P = E.shape[0]
            out = torch.zeros(P, n, device=self.device, dtype=torch.float32)
            floats = C.c_int64(0)
            nv.check(self.lib.lip_vjp_eigen_wnorm_scratch(self.h, P, C.byref(floats)), "lip_vjp_eigen_wnorm_scratch")
            scratch = self._scratches.get("lip_vjp_eigen_wnorm")
            if scratch is None or scratch.numel() < floats.value:
                scratch = self._scratches["lip_vjp_eigen_wnorm"] = torch.empty(max(4, floats.value), device=self.device,
                                                                               dtype=torch.float32)
            nv.check(self.lib.lip_vjp_eigen_wnorm(self.h, nv.ptr(E), Vp, Up, Rp, Mts, cap, nv.ptr(w_rem), nv.ptr(out), P, head,
                                                  1.0, scratch.data_ptr(), scratch.numel(), nv.stream_ptr()),
                     "lip_vjp_eigen_wnorm")
            return out

        def chunked(U: torch.Tensor, head: int) -> torch.Tensor:
            pc = U.shape[0] if class_chunk is None else int(class_chunk)
            return torch.cat([sweep(U[p0:p0 + pc], head) for p0 in range(0, U.shape[0], pc)])

        if probes is not None:
            return chunked(*self._cotangents(probes, "raw"))
        if diag:
            E = torch.eye(K, device=self.device, dtype=torch.float32)
        else:
            E, ks, kps = polarisation_probes(K)
            E = E.to(self.device)
        U, head = self._cotangents(E[:, None, :].expand(E.shape[0], n, K), "raw")
        q = chunked(U, head).T.double()                                                     # (n, P)
        return q if diag else covariance_from_polarisation(q, ks.to(self.device), kps.to(self.device), K)

    # ------------------------------------------------------------------------------ measurement
    def profile(self, enable: bool):
        nv.check(self.lib.lip_engine_profile(self.h, int(enable)), "lip_engine_profile")

    def profile_read(self):
        """{op kind: (ms, launches)} accumulated since the last read (HIP events on the launch stream)."""
        nk = 16
        ms = (C.c_double * nk)()
        cnt = (C.c_int64 * nk)()
        nv.check(self.lib.lip_engine_profile_read(self.h, ms, cnt, nk), "lip_engine_profile_read")
        return {k: (ms[k], cnt[k]) for k in range(nk) if cnt[k]}

    def flops_per_probe(self):
        return tape_flops_per_probe(self.cn)

    def executed_flops_per_probe(self):
        """matrix-pipe FLOPs actually issued per probe (Winograd ops at 4/9 of their algorithmic count) when the route
        is on (``lip_get_winograd() != 0``), else the algorithmic count"""
        if self.lib.lip_get_winograd() == 0 or self.lib.lip_get_precision() != 0:
            return tape_flops_per_probe(self.cn)
        return tape_executed_flops_per_probe(self.cn)

    # ------------------------------------------------------------------------------ operators
    def ggn_vp(self, V: torch.Tensor, scale: float = 1.0, alpha: float = 0.0, out: Optional[torch.Tensor] = None):
        Vb = self._block(V, self.D)
        Y = out if out is not None else torch.empty_like(Vb)
        nv.check(self.lib.lip_ggn_vp(self.h, nv.ptr(Vb), nv.ptr(Y), Vb.shape[0], float(scale), float(alpha),
                                     nv.stream_ptr()), "lip_ggn_vp")
        return Y

    def ggn_vp_diag(self, V: torch.Tensor, scale: float, a: torch.Tensor, out: Optional[torch.Tensor] = None):
        """:meth:`ggn_vp` with a vector prior precision: Y = scale * sum_i J_i^T H_i J_i V + a (.) V, ``a`` a (D,) vector
        in flat-parameter order (``lip_ggn_vp_diag``).  V is not written."""
        Vb = self._block(V, self.D)
        a = a.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if a.numel() != self.D:
            raise ValueError(f"a must hold {self.D} precisions, got {tuple(a.shape)}")
        Y = out if out is not None else torch.empty_like(Vb)
        nv.check(self.lib.lip_ggn_vp_diag(self.h, nv.ptr(Vb), nv.ptr(Y), Vb.shape[0], float(scale), nv.ptr(a),
                                          nv.stream_ptr()), "lip_ggn_vp_diag")
        return Y

    def run_op(self, op: "nv.Op", P: int, V: Optional[torch.Tensor] = None, Y: Optional[torch.Tensor] = None,
               H: Optional[torch.Tensor] = None, head_mode: int = 0, head_c: float = 1.0) -> None:
        """Launch ONE host-built op against this binding (``lip_engine_run_op``): operands in the THETA / CONST / PRIM /
        WORK spaces resolve to the engine's buffers, VIN / YOUT / HEAD to the blocks passed here."""
        nv.check(self.lib.lip_engine_run_op(self.h, C.byref(op), nv.ptr(V), nv.ptr(Y), nv.ptr(H), int(P), int(head_mode),
                                            float(head_c), nv.stream_ptr()), "lip_engine_run_op")

    def jvp(self, V: torch.Tensor, mode: str = "raw", c: float = 1.0) -> torch.Tensor:
        Vb = self._block(V, self.D)
        U = torch.empty(Vb.shape[0], self.n, self.K, device=self.device, dtype=torch.float32)
        m = nv.HEAD_LT if mode == "lt" else nv.HEAD_OUT
        nv.check(self.lib.lip_jvp(self.h, nv.ptr(Vb), nv.ptr(U), Vb.shape[0], m, float(c), nv.stream_ptr()), "lip_jvp")
        return U

    def vjp(self, U: torch.Tensor, mode: str = "raw", c: float = 1.0) -> torch.Tensor:
        Ub, m = self._cotangents(U, mode)
        Y = torch.empty(Ub.shape[0], self.D, device=self.device, dtype=torch.float32)
        nv.check(self.lib.lip_vjp(self.h, nv.ptr(Ub), nv.ptr(Y), Ub.shape[0], m, float(c), nv.stream_ptr()), "lip_vjp")
        return Y

    def vjp_rows(self, U: torch.Tensor, mode: str = "raw", c: float = 1.0) -> torch.Tensor:
        """Per-example rows of :meth:`vjp`: ``out[p, i] = J_i^T (c L_i U[p, i])`` -> (P, n, D).  Nothing is summed
        over examples, so the cost is that of ONE backward sweep per probe for all n rows."""
        Ub, m = self._cotangents(U, mode)
        Y = torch.empty(Ub.shape[0], self.n, self.D, device=self.device, dtype=torch.float32)
        nv.check(self.lib.lip_vjp_rows(self.h, nv.ptr(Ub), nv.ptr(Y), Ub.shape[0], m, float(c), nv.stream_ptr()),
                 "lip_vjp_rows")
        return Y

    def vjp_sqsum(self, U: torch.Tensor, mode: str = "raw", c: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Square sum of the rows of :meth:`vjp_rows` -> (D,):  ``sum_p sum_i (J_i^T (c L_i U[p, i]))**2`` ('l') or
        ``sum_p sum_i (J_i^T U[p, i])**2`` ('raw'), ADDED into ``out`` when it is given (a zero vector otherwise).
        Every per-(probe, example) parameter cotangent is squared where the backward sweep forms it (``lip_vjp_sqsum``),
        so no (P, n, D) rows exist; the result is bitwise reproducible.  One-hot probes e_k on every example give the
        GGN diagonal (:func:`ggn.compute_ggn_diag`); per-example loss gradients ('raw') the empirical-Fisher diagonal.
        The kernels' scratch is a device buffer allocated once per engine, sized for the engine's probe chunk."""
        Ub, m = self._cotangents(U, mode, strict=True)
        if out is None:
            out = torch.zeros(self.D, device=self.device, dtype=torch.float32)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.D):
            raise ValueError(f"out must be a contiguous float32 device vector of {self.D} floats")
        scratch = self._scratch("lip_vjp_sqsum_scratch")
        nv.check(self.lib.lip_vjp_sqsum(self.h, nv.ptr(Ub), nv.ptr(out), Ub.shape[0], m, float(c), nv.ptr(scratch),
                                        scratch.numel(), nv.stream_ptr()), "lip_vjp_sqsum")
        return out

    def vjp_wnorm(self, U: torch.Tensor, w: Optional[torch.Tensor] = None, mode: str = "raw", c: float = 1.0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Weighted square norm of the rows of :meth:`vjp_rows` -> (P, n):  ``out[p, i] = sum_d w[d] r_pi[d]**2`` with
        ``r_pi = J_i^T (c L_i U[p, i])`` ('l') or ``J_i^T U[p, i]`` ('raw'), ADDED into ``out`` when it is given.
        ``w`` is a (D,) vector in flat-parameter order (None: all ones, the squared row norms).  The squares are
        weighted and summed where the backward sweep forms each per-(probe, example) cotangent (``lip_vjp_wnorm``): no
        (P, n, D) rows exist and the result is bitwise reproducible.  One-hot probes e_k with the variances of a diagonal
        posterior give the linearised predictive variances (:func:`lla.predict_lla_diag`).  The kernels' scratch is a
        device buffer allocated once per engine, sized for the engine's probe chunk."""
        Ub, m = self._cotangents(U, mode, strict=True)
        P = Ub.shape[0]
        if w is not None:
            w = w.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if w.numel() != self.D:
                raise ValueError(f"w must hold {self.D} weights, got {tuple(w.shape)}")
        if out is None:
            out = torch.zeros(P, self.n, device=self.device, dtype=torch.float32)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == P * self.n):
            raise ValueError(f"out must be a contiguous float32 device block of {P} x {self.n} floats")
        scratch = self._scratch("lip_vjp_wnorm_scratch")
        nv.check(self.lib.lip_vjp_wnorm(self.h, nv.ptr(Ub), nv.ptr(w), nv.ptr(out), P, m, float(c), nv.ptr(scratch),
                                        scratch.numel(), nv.stream_ptr()), "lip_vjp_wnorm")
        return out
