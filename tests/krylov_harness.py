"""Call-level harness for the Krylov / trace primitives (csrc/lip_krylov.hip and the two tall-skinny GEMMs of
csrc/lip_mfma.hip) — TEST INFRASTRUCTURE (a plain helper module).

One call of one ``lip_*`` entry point is laid out in a single arena of 32-bit words, every word the NaN canary of
``op_harness.CANARY``: each operand sits at a chosen float offset 0..3 from a 16-byte aligned address between guard
zones; row padding, unused basis rows and the rows of inactive probes stay canaries.  ``compare`` then checks, on the
host alone (so the CPU suite can show that it bites):

* every word outside the elements the call must write is bitwise unchanged (canaries and inputs alike);
* every element the call must write is finite (no canary left) and within its bound of the float64 reference:
  ``k * unit * Mag`` with ``Mag`` the reference on the absolute values of every operand and ``unit`` 2^-24 (2^-53 for
  the float64 output of ``dot_nt_f64``); sums of length L additionally ``RMS(err / (unit Mag)) <= sqrt(L)``
  (``RMS_EXACT`` of tests/test_kernel_routes.py) when the call has at least 64 such outputs;
* exact inputs (small integers; the harness asserts that the sum of the absolute terms of every output stays below
  2^24, resp. 2^53, so that any summation order is exact): the result EQUALS the reference;
* a second run on restored buffers: bitwise equal for the outputs no float atomics feed, within the bound otherwise.

The module also holds a numpy Philox4x32-10 and the two layouts the fill kernels document.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from op_harness import CANARY, TINY

F64 = torch.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
GUARD = 1024                         # canary words around every operand
RMS_EXACT = 1.0                      # as tests/test_kernel_routes.py
LIP_OK, LIP_ERR_ARG = 0, 1


# ------------------------------------------------------------------------------------------------ arena
@dataclass
class Region:
    base: int                        # first word in the arena
    rows: int
    n: int
    ld: int                          # elements between rows
    dtype: str = "f32"               # "f32" | "f64" (two words per element, base even) | "i32"
    rowsel: Optional[List[int]] = None   # the rows the call writes (outputs only; None: all)

    @property
    def w(self):
        return 2 if self.dtype == "f64" else 1

    def span(self):
        return ((self.rows - 1) * self.ld + self.n) * self.w

    def sub(self, row0, rows, ld, n=None):
        """rows row0, row0 + ld/self.ld, ... as a region of their own"""
        return Region(self.base + row0 * self.ld * self.w, rows, self.n if n is None else n, ld, self.dtype)

    def view(self, words):
        t = words[self.base: self.base + self.span()]
        t = t.view({"f32": torch.float32, "f64": torch.float64, "i32": torch.int32}[self.dtype])
        return t.as_strided((self.rows, self.n), (self.ld, 1))

    def read(self, words):
        v = self.view(words)
        return (v[self.rowsel] if self.rowsel is not None else v).clone()

    def write(self, words, values):
        v = self.view(words)
        if self.rowsel is not None:
            v[self.rowsel] = values.to(v.dtype)
        else:
            v.copy_(values)

    def mark(self, mask):
        """set the words of the (selected) elements in an int32 mask"""
        m = Region(self.base, self.rows, self.n * self.w, self.ld * self.w, "i32").view(mask)
        if self.rowsel is not None:
            m[self.rowsel] = 1
        else:
            m.fill_(1)


class Arena:
    """bump allocator: word offsets, operands 16-byte aligned + ``off`` floats, GUARD canaries between"""

    def __init__(self):
        self.cur = GUARD
        self.regs: Dict[str, Region] = {}

    def alloc(self, name, rows, n, ld=None, off=0, dtype="f32"):
        ld = n if ld is None else ld
        assert ld >= n and (dtype != "f64" or off % 2 == 0)
        r = Region((self.cur + 3) // 4 * 4 + off, rows, n, ld, dtype)
        self.cur = r.base + r.span() + GUARD
        self.regs[name] = r
        return r

    def words(self):
        return torch.full((self.cur,), CANARY, dtype=torch.int32)


@dataclass
class Out:
    region: Region
    k: float                         # bound in units of unit * Mag (ignored for exact inputs)
    L: int = 0                       # reduction length for the RMS criterion (0: none)
    det: Optional[bool] = True       # bitwise equal in a second run (None: decided by the census label)
    unit: float = U24


@dataclass
class Call:
    """one laid-out call: ``args(devbase)`` are the ctypes arguments (stream excluded); ``ref(get, ab, got)`` returns
    {output: float64 tensor} from ``get(name)`` (float64 operand values; absolute values and differences taken as sums
    when ``ab``) and ``got(name)`` (what the kernel wrote, for the outputs defined on another output)."""
    prim: str
    arena: Arena
    words: torch.Tensor
    args: Callable[[int], list]
    outs: Dict[str, Out]
    ref: Callable
    exact: bool = False
    exact_unit: float = 1.0          # every output of an exact case is a multiple of this
    dep: bool = False                # an output is defined on another output (nrm2 on w, rr_new on r)
    info: dict = field(default_factory=dict)

    def get(self, words, ab=False):
        def g(name):
            v = self.arena.regs[name].view(words).double()
            return v.abs() if ab else v
        return g

    def got(self, words):
        return lambda name: self.outs[name].region.read(words).double()

    def reference(self, got_words):
        """(ref, mag): {output: float64 (rows, n)}"""
        return (self.ref(self.get(self.words), False, self.got(got_words)),
                self.ref(self.get(self.words, True), True, self.got(got_words)))

    def ptr(self, devbase, name):
        return devbase + 4 * self.arena.regs[name].base if name in self.arena.regs else 0


def simulate(call: Call):
    """the arena after a perfect kernel: every output holds the reference rounded to its type (CPU tests)"""
    words = call.words.clone()
    for _ in range(2 if call.dep else 1):          # twice: outputs defined on other outputs (nrm2, rr_new)
        ref, _ = call.reference(words)
        for name, o in call.outs.items():
            o.region.write(words, ref[name].to(o.region.view(words).dtype))
    return words


def assert_exact_inputs(call: Call, got_words=None):
    """the condition that makes an exact case independent of the summation order: every output's reference and the
    sum of the absolute values of its terms are multiples of exact_unit below 2^24 (2^53) of them"""
    words = simulate(call) if got_words is None else got_words
    ref, mag = call.reference(words)
    for name, o in call.outs.items():
        lim = (2.0 ** 53 if o.unit == U53 else 2.0 ** 24) * call.exact_unit
        if ref[name].numel() == 0:
            continue
        assert mag[name].max().item() < lim, f"{call.prim}: {name}: sum of absolute terms {mag[name].max().item():.4g} >= {lim:.4g}"
        q = ref[name] / call.exact_unit
        assert torch.equal(q, q.round()), f"{call.prim}: {name}: the reference is not a multiple of {call.exact_unit}"


def compare(call: Call, got_words, again_words=None, what="", det_override=None, measure=False):
    """all checks of one run (and of a second run); returns {output: (worst normalised error, rms / sqrt(L))}"""
    mask = torch.zeros(call.words.numel(), dtype=torch.int32)
    for o in call.outs.values():
        o.region.mark(mask)
    keep = mask == 0
    for tag, w in (("", got_words), (" (second run)", again_words)):
        if w is None:
            continue
        a, b = w[keep], call.words[keep]
        if not torch.equal(a, b):
            pos = torch.nonzero(keep).flatten()[torch.nonzero(a != b).flatten()[:5]].tolist()
            where = [n for n, r in call.arena.regs.items() if any(r.base - GUARD <= p < r.base + r.span() + GUARD for p in pos)]
            raise AssertionError(f"{what}{tag}: {int((a != b).sum())} words outside the outputs changed "
                                 f"(first at {pos}, near {where})")
    stats = {}
    for tag, w in (("", got_words), (" (second run)", again_words)):
        if w is None:
            continue
        if tag == "" or call.dep:
            ref, mag = call.reference(w)
        for name, o in call.outs.items():
            y = o.region.read(w).double()
            if y.numel() == 0:                      # no active probe: nothing to write
                continue
            r, M = ref[name], mag[name]
            assert y.shape == r.shape, (name, y.shape, r.shape)
            bad = ~torch.isfinite(y)
            assert not bad.any(), f"{what}{tag}: {name}: {int(bad.sum())} of {y.numel()} elements not written or not finite"
            if call.exact and o.k == 0:
                ne = y != r
                if ne.any():
                    i = torch.nonzero(ne)[0].tolist()
                    raise AssertionError(f"{what}{tag}: {name}: {int(ne.sum())} of {ne.numel()} elements differ from the exact "
                                         f"reference (first at {i}: got {y[tuple(i)].item()!r}, ref {r[tuple(i)].item()!r})")
                stats.setdefault(name, (0.0, 0.0))
                continue
            e = (y - r).abs() / (o.unit * M + TINY)
            worst = e.max().item()
            if not measure and worst > o.k:
                i = torch.nonzero(e == e.max())[0].tolist()
                raise AssertionError(f"{what}{tag}: {name}: {int((e > o.k).sum())} of {e.numel()} elements above {o.k:.4g} units of Mag "
                                     f"(worst {worst:.4g} at {i}: got {y[tuple(i)].item()!r}, ref {r[tuple(i)].item()!r}, "
                                     f"Mag {M[tuple(i)].item():.4g})")
            rms = 0.0
            if o.L and e.numel() >= 64:
                rms = e.pow(2).mean().sqrt().item() / math.sqrt(o.L)
                assert measure or rms <= RMS_EXACT, f"{what}{tag}: {name}: RMS of the normalised error {rms:.4g} sqrt({o.L}) above {RMS_EXACT}"
            old = stats.get(name, (0.0, 0.0))
            stats[name] = (max(old[0], worst), max(old[1], rms))
    if again_words is not None:
        for name, o in call.outs.items():
            det = o.det if o.det is not None else det_override
            assert det is not None, f"{what}: {name}: determinism undecided"
            if det:
                a, b = o.region.read(got_words), o.region.read(again_words)
                same = torch.equal(a.view(torch.int32) if a.dtype != F64 else a.view(torch.int64),
                                   b.view(torch.int32) if b.dtype != F64 else b.view(torch.int64))
                assert same, f"{what}: {name} differs bitwise in a second run"
    return stats


# ------------------------------------------------------------------------------------------------ GPU side
def routes(lib) -> Dict[str, int]:
    """the census since the last read (reading clears it)"""
    n = lib.lip_debug_route_count()
    counts = (C.c_int64 * n)()
    names = (C.c_char_p * n)()
    rc = lib.lip_debug_routes(counts, n, names)
    assert rc >= 0
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


def launch(lib, call: Call, dev):
    from lip_amd import _native as nv
    rc = getattr(lib, "lip_" + call.prim)(*call.args(dev.data_ptr()), nv.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run(lib, call: Call, what="", measure=False, det_of_label=None):
    """two runs on the GPU and every check; returns (census of the first run, stats)"""
    from lip_amd import _native as nv
    if call.exact:
        assert_exact_inputs(call)
    dev = call.words.cuda()
    assert dev.data_ptr() % 16 == 0
    routes(lib)
    nv.check(launch(lib, call, dev), what)
    census = routes(lib)
    got = dev.cpu()
    dev.copy_(call.words)
    nv.check(launch(lib, call, dev), what)
    again = dev.cpu()
    del dev
    det = det_of_label(census) if det_of_label else None
    return census, compare(call, got, again, what, det_override=det, measure=measure)


def run_refused(lib, call: Call, what=""):
    """the call must return LIP_ERR_ARG with a message, launch nothing and leave every word as it was"""
    dev = call.words.cuda()
    routes(lib)
    rc = launch(lib, call, dev)
    assert rc == LIP_ERR_ARG, f"{what}: returned {rc}, expected LIP_ERR_ARG"
    msg = lib.lip_last_error()
    assert msg and call.prim.encode() in msg, f"{what}: no message naming the primitive: {msg!r}"
    assert routes(lib) == {}, f"{what}: a refused call reached a launch site"
    assert torch.equal(dev.cpu(), call.words), f"{what}: a refused call wrote to memory"


# ------------------------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(ctr, key, rounds=10):
    """Philox4x32: ctr = 4 arrays (or ints) of 32-bit words, key = 2; returns 4 uint64 arrays holding 32-bit words"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in ctr]
    k = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in key]
    for _ in range(rounds):
        m0, m1 = _M0 * c[0], _M1 * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(m1 >> _S32) ^ c[1] ^ k[0], m1 & _MASK, (m0 >> _S32) ^ c[3] ^ k[1], m0 & _MASK]
        k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return c


def _lib_words(counter, seed):
    """the library's call: counter in words 0, 1, the two constants in words 2, 3, key = the seed's two words"""
    counter = np.asarray(counter, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32([counter & _MASK, counter >> _S32, 0x9E3779B9, 0xBB67AE85], [seed & 0xFFFFFFFF, seed >> 32])


def ref_rademacher(total, seed):
    """fill_rademacher_kernel: thread t of chunk ch draws once (counter ch * 256 + t); quad (ch * 32 + i) * 256 + t takes
    bits 4 (i & 7) .. + 3 of word i >> 3, element h of the quad bit h of those; bit set = +1"""
    nq = (total + 3) // 4
    nchunk = (nq + 8191) // 8192
    u = np.stack(_lib_words(np.arange(nchunk * 256), seed)).reshape(4, nchunk, 1, 256, 1)      # [word][ch][.][t][.]
    i = np.arange(32, dtype=np.uint64).reshape(1, 32, 1, 1)
    h = np.arange(4, dtype=np.uint64).reshape(1, 1, 1, 4)
    word = np.concatenate([np.broadcast_to(u[j], (nchunk, 8, 256, 1)) for j in range(4)], axis=1)   # [ch][i][t][.] = u[i >> 3]
    bits = (word >> (np.uint64(4) * (i & np.uint64(7)) + h)) & np.uint64(1)                    # [ch][i][t][h]
    return np.where(bits.reshape(-1)[:total] == 1, 1.0, -1.0).astype(np.float32)


def compare_rademacher(got, total, seed):
    """got (total,) float32 must equal the reference element for element"""
    ref = ref_rademacher(total, seed)
    ne = np.nonzero(np.asarray(got) != ref)[0]
    assert ne.size == 0, f"{ne.size} of {total} signs differ from Philox4x32-10 (first at {ne[:5].tolist()})"


def ref_normal(total, seed):
    """fill_kernel<NORMAL>: quad q draws once (counter q); word pairs (0, 1) and (2, 3) give (rad cos, rad sin) with
    u = ((w >> 8) + 0.5) / 2^24 formed in float32 as the kernel forms it, the angle 2 pi u2 rounded to float32 as well;
    logarithm, square root, sine and cosine in float64.  Returns (values, rad) as float64 arrays of length total"""
    nq = (total + 3) // 4
    w = _lib_words(np.arange(nq), seed)
    f32 = np.float32
    u = [((x >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0) for x in w]
    out = np.empty((nq, 4))
    rad = np.empty((nq, 4))
    for hh in range(2):
        r = np.sqrt(-2.0 * np.log(u[2 * hh].astype(np.float64)))
        ang = (f32(6.283185307179586) * u[2 * hh + 1]).astype(np.float64)
        out[:, 2 * hh], out[:, 2 * hh + 1] = r * np.cos(ang), r * np.sin(ang)
        rad[:, 2 * hh] = rad[:, 2 * hh + 1] = r
    return out.reshape(-1)[:total], rad.reshape(-1)[:total]


# ------------------------------------------------------------------------------------------------ the primitives
class Filler:
    """operand values: exact -> integers in [-vmax, vmax] drawn per position; random -> randn"""

    def __init__(self, exact, seed):
        self.exact = exact
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, rows, n, vmax=2, density=1.0):
        if self.exact:
            v = torch.randint(-vmax, vmax + 1, (rows, n), generator=self.g).double()
            if density < 1.0:
                v = v * (torch.rand(rows, n, generator=self.g) < density)
            return v
        return torch.randn(rows, n, generator=self.g, dtype=F64)

    def scal(self, n, choices=(1.0, 2.0, -2.0, 4.0, 0.5)):
        """per-probe scalars: powers of two (exact) or randn away from 0"""
        if self.exact:
            idx = torch.randint(0, len(choices), (n,), generator=self.g)
            return torch.tensor(choices, dtype=F64)[idx][None]
        v = torch.randn(1, n, generator=self.g, dtype=F64)
        return v + v.sign() * 0.25


def _canary_rows(words, region, rows):
    v = region.view(words).view(torch.int32) if region.dtype != "f64" else None
    for p in rows:
        v[p] = CANARY


def _finish(prim, A, fills, args, outs, ref, exact, exact_unit=1.0, canary=(), info=None):
    words = A.words()
    for name, val in fills.items():
        A.regs[name].write(words, val.to({"f32": torch.float32, "f64": F64, "i32": torch.int32}[A.regs[name].dtype]))
    for name, rows in canary:
        _canary_rows(words, A.regs[name], rows)
    if exact and prim != "scale_store":              # exact inputs: the result equals the reference
        for o in outs.values():
            o.k = 0
    return Call(prim, A, words, args, outs, ref, exact, exact_unit, prim in ("cg_update", "multi_axpy_norm"), info or {})


def build_bdot(d, exact, seed=0):
    P, N, off = d["P"], d["N"], d.get("off", 0)
    F, A = Filler(exact, seed), Arena()
    same = d.get("same", False)
    A.alloc("X", P, N, off=off)
    if not same:
        A.alloc("Y", P, N, off=d.get("off_y", off))
    o = A.alloc("out", 1, P, off=d.get("off_o", 0))
    fills = {"X": F(P, N)}
    if not same:
        fills["Y"] = F(P, N)
    yn = "X" if same else "Y"

    def ref(get, ab, got):
        return {"out": (get("X") * get(yn)).sum(1)[None]}
    c = _finish("bdot", A, fills, None, {"out": Out(o, N + 16, N, det=False)}, ref, exact)
    c.args = lambda b: [c.ptr(b, "X"), c.ptr(b, yn), c.ptr(b, "out"), P, N]
    return c


def build_axpby(d, exact, seed=0):
    """a / b: None (null pointer) or "vec"; zero_b: rows whose b[p] is 0 (their Y rows are NaN); b_s == 0: all Y NaN"""
    P, N, off = d["P"], d["N"], d.get("off", 0)
    F, A = Filler(exact, seed), Arena()
    same = d.get("same", False)
    y = A.alloc("Y", P, N, off=off)
    if not same:
        A.alloc("X", P, N, off=d.get("off_x", off))
    xn = "Y" if same else "X"
    fills = {"Y": F(P, N)}
    if not same:
        fills["X"] = F(P, N)
    a_s = d.get("a_s", 2.0 if exact else 0.7)
    b_s = d.get("b_s", -1.0 if exact else -1.3)
    for nm in ("a", "b"):
        if d.get(nm):
            A.alloc(nm, 1, P, off=d.get("off_" + nm, 1))
            fills[nm] = F.scal(P)
    for p in d.get("zero_b", ()):
        fills["b"][0, p] = 0.0
    nan_rows = list(range(P)) if b_s == 0 else list(d.get("zero_b", ()))
    assert not (same and nan_rows)

    def ref(get, ab, got):
        ca = abs(a_s) if ab else a_s
        cb = abs(b_s) if ab else b_s
        ca = ca * (get("a") if d.get("a") else torch.ones(1, P, dtype=F64))
        cb = cb * (get("b") if d.get("b") else torch.ones(1, P, dtype=F64))
        yv = get("Y").clone()
        yv[cb[0] == 0] = 0.0                           # Y is not read where its coefficient is 0
        return {"Y": ca.T * get(xn) + cb.T * yv}
    # roundings: ca, cb, the two products, the sum
    c = _finish("axpby", A, fills, None, {"Y": Out(y, 6)}, ref, exact, exact_unit=0.5,
                canary=[("Y", nan_rows)] if nan_rows else ())
    c.args = lambda b: [c.ptr(b, "Y"), c.ptr(b, xn), c.ptr(b, "a"), a_s, c.ptr(b, "b"), b_s, P, N]
    return c


def _active(d, P):
    act = d.get("active")                           # None | list of 0 / 1
    rows = list(range(P)) if act is None else [p for p in range(P) if act[p]]
    return act, rows


def build_cg_update(d, exact, seed=0):
    P, N, off = d["P"], d["N"], d.get("off", 0)
    F, A = Filler(exact, seed), Arena()
    act, rows = _active(d, P)
    big = exact and 100 * N >= 2 ** 24               # rr_new sums squares of the updated r: smaller values for long rows
    vmax = 1 if big else 2
    dens = 0.5 if big else 1.0
    regs = {n: A.alloc(n, P, N, off=off) for n in ("x", "r", "p", "Ap")}
    fills = {n: F(P, N, vmax, dens) for n in regs}
    for n in ("rr_old", "pAp", "rr_new"):
        A.alloc(n, 1, P, off=1)
    if exact:                                        # a = rr_old / pAp = 8 / 2 (or 2 / 2)
        fills["rr_old"] = torch.full((1, P), 2.0 if big else 8.0, dtype=F64)
        fills["pAp"] = torch.full((1, P), 2.0, dtype=F64)
    else:
        fills["rr_old"], fills["pAp"] = F.scal(P).abs(), F.scal(P).abs()
    if act is not None:
        A.alloc("active", 1, P, dtype="i32", off=2)
        fills["active"] = torch.tensor([act], dtype=torch.int32)
    sel = None if act is None else rows

    def ref(get, ab, got):
        a = (get("rr_old") / get("pAp")).T
        s = 1.0 if ab else -1.0
        rr = torch.zeros(1, P, dtype=F64)
        if rows:
            rr[0, rows] = (got("r") ** 2).sum(1)
        return {"x": (get("x") + a * get("p"))[rows], "r": (get("r") + s * a * get("Ap"))[rows], "rr_new": rr}
    outs = {"x": Out(Region(regs["x"].base, P, N, N, rowsel=sel), 4), "r": Out(Region(regs["r"].base, P, N, N, rowsel=sel), 4),
            "rr_new": Out(A.regs["rr_new"], N + 16, N, det=False)}
    c = _finish("cg_update", A, fills, None, outs, ref, exact)
    c.args = lambda b: [c.ptr(b, n) for n in ("x", "r", "p", "Ap", "rr_old", "pAp", "active", "rr_new")] + [P, N]
    return c


def build_cg_direction(d, exact, seed=0):
    P, N, off = d["P"], d["N"], d.get("off", 0)
    F, A = Filler(exact, seed), Arena()
    act, rows = _active(d, P)
    regs = {n: A.alloc(n, P, N, off=off) for n in ("p", "r")}
    fills = {n: F(P, N) for n in regs}
    for n in ("rr_new", "rr_old"):
        A.alloc(n, 1, P, off=3)
    if exact:
        fills["rr_new"], fills["rr_old"] = torch.full((1, P), 8.0, dtype=F64), torch.full((1, P), 2.0, dtype=F64)
    else:
        fills["rr_new"], fills["rr_old"] = F.scal(P).abs(), F.scal(P).abs()
    if act is not None:
        A.alloc("active", 1, P, dtype="i32", off=1)
        fills["active"] = torch.tensor([act], dtype=torch.int32)

    def ref(get, ab, got):
        return {"p": (get("r") + (get("rr_new") / get("rr_old")).T * get("p"))[rows]}
    outs = {"p": Out(Region(regs["p"].base, P, N, N, rowsel=None if act is None else rows), 4)}
    c = _finish("cg_direction", A, fills, None, outs, ref, exact)
    c.args = lambda b: [c.ptr(b, n) for n in ("p", "r", "rr_new", "rr_old", "active")] + [P, N]
    return c


def _basis(A, F, d, exact, density=1.0):
    """Q (P, kmax, ldq), 16-byte aligned; rows >= k and the ldq - N padding of rows < k stay canaries"""
    P, N, k, kmax = d["P"], d["N"], d["k"], d.get("kmax", d["k"] + 2)
    ldq = (N + 3) // 4 * 4 + d.get("ldq_extra", 0)
    q = A.alloc("Q", P * kmax, N, ld=ldq)
    used = [p * kmax + j for p in range(P) for j in range(k)]
    val = torch.zeros(P * kmax, N, dtype=F64)
    val[used] = F(P * k, N, 2, density)
    return q, ldq, kmax, used, val


def _restore_unused(c, used, rows):
    """rows of the basis the call does not touch go back to canaries (write() filled whole rows)"""
    v = c.arena.regs["Q"].view(c.words).view(torch.int32)
    for r in range(rows):
        if r not in used:
            v[r] = CANARY


def build_multi_dot(d, exact, seed=0):
    P, N, k = d["P"], d["N"], d["k"]
    F, A = Filler(exact, seed), Arena()
    q, ldq, kmax, used, qv = _basis(A, F, d, exact)
    A.alloc("w", P, N, off=d.get("off", 0))
    cfull = A.alloc("c", P, kmax, off=d.get("off_c", 0))
    cout = Region(cfull.base, P, k, kmax)

    def ref(get, ab, got):
        Q = get("Q").reshape(P, kmax, N)[:, :k]
        return {"c": torch.einsum("pjn,pn->pj", Q, get("w"))}
    c = _finish("multi_dot", A, {"Q": qv, "w": F(P, N)}, None, {"c": Out(cout, N + 16, N, det=False)}, ref, exact)
    _restore_unused(c, set(used), P * kmax)
    c.args = lambda b: [c.ptr(b, "Q"), c.ptr(b, "w"), c.ptr(b, "c"), P, k, kmax, N, ldq]
    return c


def build_multi_axpy_norm(d, exact, seed=0):
    P, N, k = d["P"], d["N"], d["k"]
    F, A = Filler(exact, seed), Arena()
    q, ldq, kmax, used, qv = _basis(A, F, d, exact)
    w = A.alloc("w", P, N, off=d.get("off", 0))
    A.alloc("c", P, kmax, off=d.get("off_c", 0))
    nr = A.alloc("nrm2", 1, P, off=2)
    cv = torch.zeros(P, kmax, dtype=F64)
    if exact:                                        # at most three non-zero coefficients per probe: |w'| <= 2 + 3 * 2 * 2
        for p in range(P):
            for j in sorted({0, k // 2, k - 1}):
                cv[p, j] = (-2.0, 1.0, 2.0)[(p + j) % 3]
    else:
        cv[:, :k] = F(P, k) / math.sqrt(k)

    def ref(get, ab, got):
        Q = get("Q").reshape(P, kmax, N)[:, :k]
        s = 1.0 if ab else -1.0
        return {"w": get("w") + s * torch.einsum("pjn,pj->pn", Q, get("c")[:, :k]), "nrm2": (got("w") ** 2).sum(1)[None]}
    # the update is k sequential multiply-adds of at most two roundings each
    outs = {"w": Out(w, 2 * k + 1), "nrm2": Out(nr, N + 16, N, det=False)}
    c = _finish("multi_axpy_norm", A, {"Q": qv, "w": F(P, N), "c": cv}, None, outs, ref, exact)
    _restore_unused(c, set(used), P * kmax)
    cw = c.arena.regs["c"].view(c.words).view(torch.int32)
    cw[:, k:] = CANARY
    c.args = lambda b: [c.ptr(b, "Q"), c.ptr(b, "c"), c.ptr(b, "w"), c.ptr(b, "nrm2"), P, k, kmax, N, ldq]
    return c


def build_scale_store(d, exact, seed=0, k_bound=None):
    """Q[p][j] = w[p] rsqrt(nrm2[p]), the whole row of ldq floats written (padding zero).  inf_rows: nrm2 = +inf, w = 0"""
    P, N, j = d["P"], d["N"], d["j"]
    kmax = d.get("kmax", j + 1)
    F, A = Filler(exact, seed), Arena()
    ldq = (N + 3) // 4 * 4 + d.get("ldq_extra", 0)
    q = A.alloc("Q", P * kmax, ldq, ld=ldq)
    A.alloc("w", P, N, off=d.get("off", 0))
    A.alloc("nrm2", 1, P, off=1)
    wv = F(P, N, 1000 if exact else 2)
    if exact:                                        # powers of four: rsqrt is a power of two, the quotient exact
        nv_ = torch.tensor([[4.0 ** ((p % 5) - 1) for p in range(P)]], dtype=F64)
    else:
        nv_ = (wv ** 2).sum(1)[None] * (1 + 0.1 * torch.rand(1, P, generator=F.g, dtype=F64))
    for p in d.get("inf_rows", ()):
        nv_[0, p] = math.inf
        wv[p] = 0.0
    qout = q.sub(j, P, kmax * ldq)

    def ref(get, ab, got):
        out = torch.zeros(P, ldq, dtype=F64)
        out[:, :N] = get("w") / get("nrm2").sqrt().T
        return {"Q": out}
    c = _finish("scale_store", A, {"w": wv, "nrm2": nv_}, None, {"Q": Out(qout, k_bound if not exact else 2.0)}, ref, exact,
                exact_unit=2.0 ** -4)
    c.args = lambda b: [c.ptr(b, "w"), c.ptr(b, "nrm2"), c.ptr(b, "Q"), j, P, kmax, N, ldq]
    return c


def _nt_operands(A, F, d):
    m, n, K = d["m"], d["n"], d["K"]
    lda, ldb = K + d.get("lda_extra", 0), K + d.get("ldb_extra", 0)
    same = d.get("same", False)
    A.alloc("A", m, K, ld=lda, off=d.get("off_a", 0))
    fills = {"A": F(m, K)}
    if not same:
        A.alloc("B", n, K, ld=ldb, off=d.get("off_b", 0))
        fills["B"] = F(n, K)
    else:
        assert m == n
        ldb = lda
    return m, n, K, lda, ldb, ("A" if same else "B"), fills


def build_dot_nt_f64(d, exact, seed=0):
    F, A = Filler(exact, seed), Arena()
    m, n, K, lda, ldb, bn, fills = _nt_operands(A, F, d)
    o = A.alloc("C", m, n, dtype="f64")

    def ref(get, ab, got):
        return {"C": get("A") @ get(bn).T}
    c = _finish("dot_nt_f64", A, fills, None, {"C": Out(o, K + 16, K, det=None, unit=U53)}, ref, exact)
    c.args = lambda b: [c.ptr(b, "A"), lda, m, c.ptr(b, bn), ldb, n, K, c.ptr(b, "C")]
    return c


def build_gemm_nt(d, exact, seed=0):
    F, A = Filler(exact, seed), Arena()
    m, n, K, lda, ldb, bn, fills = _nt_operands(A, F, d)
    o = A.alloc("C", m, n, off=d.get("off_c", 0))

    def ref(get, ab, got):
        return {"C": get("A") @ get(bn).T}
    c = _finish("gemm_nt", A, fills, None, {"C": Out(o, K + 16, K, det=None)}, ref, exact)
    c.args = lambda b: [c.ptr(b, "A"), lda, m, c.ptr(b, bn), ldb, n, K, c.ptr(b, "C")]
    return c


def build_gemm_nn_axpy(d, exact, seed=0):
    """v: None (null) | "distinct" | "out" (in place)"""
    m, k, N, v = d["m"], d["k"], d["N"], d.get("v")
    F, A = Filler(exact, seed), Arena()
    ldt, ldb, ldo, ldv = k + d.get("ldt_extra", 0), N + d.get("ldb_extra", 0), N + d.get("ldo_extra", 0), N + d.get("ldv_extra", 0)
    beta = d.get("beta", -2.0 if exact else 0.37)
    A.alloc("T", m, k, ld=ldt, off=d.get("off_t", 0))
    A.alloc("B", k, N, ld=ldb, off=d.get("off_b", 0))
    o = A.alloc("Out", m, N, ld=ldo, off=d.get("off_o", 0))
    fills = {"T": F(m, k), "B": F(k, N)}
    if v == "distinct":
        A.alloc("V", m, N, ld=ldv, off=d.get("off_v", 0))
        fills["V"] = F(m, N)
    elif v == "out":
        fills["Out"] = F(m, N)
        ldv = ldo
    vn = {None: None, "distinct": "V", "out": "Out"}[v]

    def ref(get, ab, got):
        r = get("T") @ get("B")
        return {"Out": r + (abs(beta) if ab else beta) * get(vn) if vn else r}
    c = _finish("gemm_nn_axpy", A, fills, None, {"Out": Out(o, k + 2 + 16, k + 2)}, ref, exact)
    c.args = lambda b: [c.ptr(b, "T"), ldt, m, k, c.ptr(b, "B"), ldb, N, c.ptr(b, vn) if vn else 0, ldv, beta, c.ptr(b, "Out"), ldo]
    return c


def build_rows_combine(d, exact, seed=0):
    r, s, N, z = d["r"], d["s"], d["N"], d.get("z", False)
    F, A = Filler(exact, seed), Arena()
    ldy, ldz, ldo = N + d.get("ldy_extra", 0), N + d.get("ldz_extra", 0), N + d.get("ldo_extra", 0)
    zscale = d.get("zscale", 1.0)
    A.alloc("Cm", r, s, dtype="f64")
    A.alloc("Y", s, N, ld=ldy, off=d.get("off_y", 0))
    o = A.alloc("Out", r, N, ld=ldo, off=d.get("off_o", 0))
    dens = min(1.0, 256.0 / s) if exact else 1.0
    fills = {"Cm": F(r, s, 2, dens) if exact else F(r, s) / math.sqrt(s) + 1e-9, "Y": F(s, N)}
    if z:
        A.alloc("Z", r, N, ld=ldz, off=d.get("off_z", 0))
        fills["Z"] = F(r, N)

    def ref(get, ab, got):
        cm = get("Cm").float().double()               # rounded once, as the kernel rounds it
        out = cm @ get("Y")
        return {"Out": out + (abs(zscale) if ab else zscale) * get("Z") if z else out}
    c = _finish("rows_combine", A, fills, None, {"Out": Out(o, s + 3)}, ref, exact, exact_unit=0.5)
    c.args = lambda b: [c.ptr(b, "Cm"), c.ptr(b, "Y"), ldy, s, c.ptr(b, "Z"), ldz, zscale, c.ptr(b, "Out"), ldo, r, N]
    return c


BUILDERS = {"bdot": build_bdot, "axpby": build_axpby, "cg_update": build_cg_update, "cg_direction": build_cg_direction,
            "multi_dot": build_multi_dot, "multi_axpy_norm": build_multi_axpy_norm, "scale_store": build_scale_store,
            "dot_nt_f64": build_dot_nt_f64, "gemm_nt": build_gemm_nt, "gemm_nn_axpy": build_gemm_nn_axpy,
            "rows_combine": build_rows_combine}
