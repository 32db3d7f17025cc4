"""Nets, masks and float64 checkers of the part-by-part tests of the weighted-norm and eigen sweeps — TEST
INFRASTRUCTURE (a plain helper module, CPU torch only: tests/test_wnorm_parts.py feeds it what the GPU computed,
tests/test_wnorm_parts_cpu.py feeds it perturbed stand-ins).

WNORM (``lip_vjp_wnorm``).  A weight of exactly 0 makes a kernel's register weight 0 and its fma add exactly 0, so with
w = m o w0 (m in {0, 1}^D, w0 positive and float32-representable) the output is the sum of ONE part: a parameter tensor,
one output tile of ``wgrad_wnorm_kernel``, one 64-column block of ``wgrad_wnorm_dense_kernel``, one column block of
``reduce_wnorm_kernel``, one row, one column, one element.  Reference: ref[p, i] = sum_j m_j w0_j rows[p, i, j]^2 in
float64 from the per-example rows of the tape emulator.  Bound per (mask, pair), the form of
``test_kernel_routes._check_sqsum``:

    |v - ref| <= 2^-24 (K_SQ sum_j m_j w0_j |r_j| max_tensor|r| + L ref)

K_SQ = 16 is the project's constant for a row element formed by the pair walk and the tile product.  L counts the
sequential float32 roundings between the tile product and ``wnorm_finish`` (which adds a launch's partials in float64):

  wgrad_wnorm_kernel<WM,WN,TM,TN>   16 TM TN fmas per lane into s, six shuffle steps of wave_sum, WM WN wave sums added
                                    by thread 0, and 2 for the roundings of wt = w * (s * s):
                                    L = 16 TM TN + 6 + WM WN + 2   (<2,1,1,1> 26 ... <2,2,2,2> 76)
  wgrad_wnorm_dense_kernel          ceil(min(256, M) / 4) fmas per row lane per chunk of 256 rows, ceil(M / 256) chunks,
                                    three adds of the four row lanes, six shuffle steps, and 2 for (sc * sc) and its
                                    product with the lane sum:  L = ceil(min(256, M) / 4) ceil(M / 256) + 3 + 6 + 2
  reduce_wnorm_kernel               one fma joins the red0 and the red1 term, six shuffle steps, 2 for the weights:
                                    L = 1 + 6 + 2 = 9   (the column sums u0, u1 are the row elements: K_SQ's part)

The rounding of wt * v inside the fma operand and the one rounding of ``wnorm_finish`` are not counted: the first term
is at least 16 ref (|r_j| <= max|r|), which leaves room for both.  A call whose mask spans several launches (the
unmasked total, w=None) is rounded to float32 once per launch by that launch's ``wnorm_finish``, each time by at most
2^-24 of the running total, so there L = max over the launches of L + the number of launches.

EWNORM (``lip_vjp_eigen_wnorm``) and EIGEN (``lip_vjp_eigen``).  T = (At V)^T (G Ub) per (probe, example) and block; the
unit of the bound is built on the absolute-value twin |T| = (|At| |V|)^T (|G| |Ub|) (``products(absolute=True)``),
since AV and GU are each rounded to float32 before the tile product:

    EWNORM  |v - ref| <= 2^-24 (C sum_{jm} R_jm |T|_jm max_block|T| + L ref)             per (mask on R, pair)
    EIGEN   |Lam_jm - want_jm| <= 2^-24 (C sum_{p,i} |T|_jm max_block|T| + 4 want_jm)    per element

The constants C are measured on MI355X and stand in tests/test_wnorm_parts.py.

Conditions on the inputs.  A mask whose float64 reference is 0 for a pair tests nothing for that pair.  The ReLU nets
have dead elements (3 - 68 % of the row elements are zero for every pair; corner elements are dead in a/Conv_3,
c/Dense_0, d/Dense_0, d/Dense_1 and bn_maxpool/Conv_1), the tanh nets have none: the per-tensor and per-tile masks run
on every net, the edge masks (single rows, columns, elements) on the tanh twins of a and b and on lenet only.
tests/test_wnorm_parts_cpu.py asserts that every such reference is non-zero for every pair.
"""
import dataclasses
import functools
from typing import List, Tuple

import torch

import aniso_nets
import kfac_ref as kf
from lip_amd import _native as nv
from lip_amd.engine import build_consts, compile_net
from lip_amd.netspec import NetSpec
from lip_amd.toymodels import create_state
from lip_amd.utils import flatten_nn_params, param_layout
from tape_emulator import TapeMachine

F64 = torch.float64
EPS = 2.0 ** -24
K_SQ = 16.0                     # tests/test_kernel_routes.py
N_EX, N_PROBES, HEAD_C = 3, 2, 0.7
L_REDUCE = 1 + 6 + 2


# ------------------------------------------------------------------------------------------------------------ nets
def net_a(act="relu", bias=False):
    """``_net_a`` of tests/test_kernel_routes.py (tiles <2,2,1,2>, <4,1,1,2>, <2,2,2,2>, <4,1,1,1>, the dense form and
    the bias reduce) with the activation and the bias of convs 1 - 3 as arguments"""
    net = NetSpec((6, 6, 3))
    x = net.conv(0, "Conv_0", 72, 3, 1, padding=1, act=act, use_bias=True)          # M = 27, N = 72
    x = net.conv(x, "Conv_1", 40, 3, 1, padding=1, act=act, use_bias=bias)          # M = 648, N = 40
    x = net.conv(x, "Conv_2", 80, 3, 1, padding=1, act=act, use_bias=bias)          # M = 360, N = 80
    x = net.conv(x, "Conv_3", 20, 3, 1, padding=1, act=act, use_bias=bias)          # M = 720, N = 20
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 5)
    net.model_type = "classifier"
    return net


def net_b(act="relu", bias=False):
    """``_net_b`` of tests/test_kernel_routes.py (tiles <4,1,1,1>, <2,2,1,1>, <2,1,1,1>, the dense form and the bias
    reduce), likewise"""
    net = NetSpec((8, 8, 32))
    x = net.conv(0, "Conv_0", 32, 3, 1, padding=1, act=act, use_bias=True)          # M = 288, N = 32
    x = net.conv(x, "Conv_1", 48, 1, 1, padding=0, act=act, use_bias=bias)          # M = 32, N = 48
    x = net.conv(x, "Conv_2", 16, 1, 1, padding=0, act=act, use_bias=bias)          # M = 48, N = 16
    x = net.meanpool(x)
    x = net.dense(x, "Dense_0", 40, act=act)
    net.dense(x, "Dense_1", 5)
    net.model_type = "classifier"
    return net


def net_bn_maxpool():
    """``_net_bn_maxpool`` of tests/test_small_ops.py: BatchNorm (red1 live) and a 3 x 3 / 2 max pool at 64 channels"""
    net = NetSpec((12, 12, 3))
    x = net.conv(0, "Conv_0", 64, 3, 1, padding=1, bn="BatchNorm_0", act="relu")
    x = net.maxpool(x, 3, 2, padding=1)
    x = net.conv(x, "Conv_1", 24, 3, 1, padding=1, bn="BatchNorm_1", act="relu")
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 5)
    net.model_type = "classifier"
    return net


def net_lenet():
    """``_net_lenet`` of tests/test_small_ops.py: tanh throughout, channel counts that are no multiple of 4"""
    net = NetSpec((16, 16, 1))
    x = net.conv(0, "Conv_0", 6, 5, 1, padding=2, act="tanh", use_bias=True)
    x = net.avgpool(x, 2, 2)
    x = net.conv(x, "Conv_1", 10, 3, 1, padding=1, act="tanh", use_bias=True)
    x = net.avgpool(x, 2, 2)
    x = net.meanpool(x)
    x = net.dense(x, "Dense_0", 12, act="tanh")
    net.dense(x, "Dense_1", 5)
    net.model_type = "classifier"
    return net


# name -> (builder, seed of the parameters and the examples): the seeds of the tests the nets come from
NETS = {
    "a": (net_a, 7), "b": (net_b, 7),
    "c": (lambda: aniso_nets.per_example_nets()["c"], 7), "d": (lambda: aniso_nets.per_example_nets()["d"], 7),
    "bn_maxpool": (net_bn_maxpool, 9), "lenet": (net_lenet, 9),
    "a_tanh": (lambda: net_a("tanh"), 7), "b_tanh": (lambda: net_b("tanh"), 7),
    "a_bias": (lambda: net_a(bias=True), 7), "b_bias": (lambda: net_b(bias=True), 7),
}
WNORM_NETS = ["a", "b", "c", "d", "bn_maxpool", "lenet", "a_tanh", "b_tanh"]
EDGE_NETS = ["a_tanh", "b_tanh", "lenet"]
EIGEN_NETS = ["a", "b", "c", "d", "a_bias", "b_bias", "bn_maxpool"]


# ------------------------------------------------------------------------------------- launch geometry, restated
def wgrad_tile(M, N):
    """(WM, WN, TM, TN) of ``with_wgrad_tile`` (lip_mfma.hip)"""
    small = M <= 64
    if N > 64:
        return (2, 2, 1, 2) if small else (2, 2, 2, 2)
    if N > 32:
        return (2, 2, 1, 1) if small else (4, 1, 1, 2)
    return (2, 1, 1, 1) if small else (4, 1, 1, 1)


def tile_dims(t):
    """(BM, BN) of ``Tile<WM, WN, TM, TN>``"""
    return t[0] * t[2] * 32, t[1] * t[3] * 32


def tile_label(t):
    return "wgrad_wnorm<%d,%d,%d,%d>" % t


def sq_cb(N):
    """``sq_cb`` of lip_small.hip: the columns of a reduce block"""
    cb = 64
    while cb > 1 and cb // 2 >= N:
        cb //= 2
    return cb


def l_tile(t):
    return 16 * t[2] * t[3] + 6 + t[0] * t[1] + 2


def l_dense(M):
    return -(-min(256, M) // 4) * -(-M // 256) + 3 + 6 + 2


@dataclasses.dataclass
class Launch:
    """one weighted-norm launch: a weight matrix (kind 'tile' or 'dense') or a reduce with its red0 / red1 slices"""
    label: str
    kind: str                                # 'tile' | 'dense' | 'reduce'
    off: int                                 # 'tile' / 'dense': offset of the (M, N) matrix
    M: int
    N: int
    reds: Tuple[Tuple[str, int], ...] = ()   # 'reduce': (label, offset) of red0 and, under BN, red1
    L: int = 0
    route: str = ""

    def grid(self):
        """(block rows, block columns) of the launch's output blocks"""
        if self.kind == "tile":
            return tile_dims(wgrad_tile(self.M, self.N))
        if self.kind == "dense":
            return self.M, 64
        return 1, sq_cb(self.N)

    def index(self, rows=None, cols=None):
        """flat parameter indices of the (rows x cols) sub-block; None: all"""
        rows = torch.arange(self.M if self.kind != "reduce" else 1) if rows is None else torch.as_tensor(rows).reshape(-1)
        cols = torch.arange(self.N) if cols is None else torch.as_tensor(cols).reshape(-1)
        if self.kind == "reduce":
            return torch.cat([o + cols for _, o in self.reds])
        return (self.off + rows[:, None] * self.N + cols[None, :]).reshape(-1)

    def blocks(self):
        """[(label, indices)]: one entry per float of partial[block][pair]"""
        bm, bn = self.grid()
        M = self.M if self.kind != "reduce" else 1
        out = []
        for r in range(-(-M // bm)):
            for c in range(-(-self.N // bn)):
                rows = torch.arange(bm * r, min(M, bm * (r + 1)))
                cols = torch.arange(bn * c, min(self.N, bn * (c + 1)))
                out.append((f"{self.label} block ({r},{c})", self.index(rows, cols)))
        return out

    def edges(self):
        """[(label, indices)] of a weight matrix: rows 0 and M - 1 and the rows either side of every block-row
        boundary, the same for the columns, and the elements (0, 0), (M - 1, N - 1), (M - 1, 0).  The dense form has
        no block rows: its boundary is the 256-row chunk."""
        bm, bn = (256, 64) if self.kind == "dense" else self.grid()
        M, N = self.M, self.N
        rows = sorted({0, M - 1} | {m for b in range(bm, M, bm) for m in (b - 1, b)})
        cols = sorted({0, N - 1} | {c for b in range(bn, N, bn) for c in (b - 1, b)})
        out = [(f"{self.label} row {m}", self.index(rows=[m])) for m in rows]
        out += [(f"{self.label} column {c}", self.index(cols=[c])) for c in cols]
        out += [(f"{self.label} element ({m},{c})", self.index([m], [c])) for m, c in ((0, 0), (M - 1, N - 1), (M - 1, 0))]
        return out


def launches_of(net, params) -> List[Launch]:
    """the weighted-norm launches of ``lip_vjp_wnorm`` on ``net``: per conv unit the weight gradient (the tile kernel, or
    the dense form at one output pixel) and the reduce of its bias or of its BN bias (red0) and BN scale (red1)"""
    lay = {path: off for path, off, _ in param_layout(params)}
    out = []
    for u in net.units:
        if u.kind != "conv":
            continue
        name = u.kernel[-2]
        M, N = u.kh * u.kw * u.cin, u.cout
        oh, ow, _ = net.tensors[u.dst]
        if oh * ow > 1:
            t = wgrad_tile(M, N)
            out.append(Launch(f"{name}/kernel", "tile", lay[u.kernel], M, N, L=l_tile(t), route=tile_label(t)))
        else:
            out.append(Launch(f"{name}/kernel", "dense", lay[u.kernel], M, N, L=l_dense(M), route="wgrad_wnorm_dense"))
        assert u.bias is None or u.bn_scale is None
        if u.bias is not None:
            out.append(Launch(f"{name}/bias", "reduce", 0, 1, N, ((f"{name}/bias", lay[u.bias]),), L_REDUCE, "reduce_wnorm"))
        if u.bn_scale is not None:
            bn = u.bn_scale[-2]
            out.append(Launch(f"{bn}", "reduce", 0, 1, N, ((f"{bn}/bias", lay[u.bn_bias]), (f"{bn}/scale", lay[u.bn_scale])),
                              L_REDUCE, "reduce_wnorm"))
    return out


# ---------------------------------------------------------------------------------------------------- bindings
def tensor_slices(params):
    """``_tensor_slices`` of tests/test_kernel_routes.py"""
    out = []
    for path, off, shape in param_layout(params):
        n = 1
        for s in shape:
            n *= s
        out.append(("/".join(str(k) for k in path[-2:]), off, off + n))
    return out


def emulator_rows(net, state, Z, U, head, c):
    """(P, n, D) float64 per-example rows: a tape compiled for ONE example run on each example in turn (nothing in these
    nets couples the examples; ``many_pairs`` of tests/test_kernel_routes.py)"""
    P, n = U.shape[:2]
    cn1 = compile_net(net, 1, state.params)
    flat, _ = flatten_nn_params(state.params)
    consts = build_consts(cn1, state.params, state.batch_stats, "cpu", F64)
    rows = torch.zeros(P, n, cn1.D, dtype=F64)
    for i in range(n):
        tm = TapeMachine(cn1, flat, consts, Z[i:i + 1], chunk=P)
        tm.primal()
        rows[:, i] = tm.vjp(U[:, i:i + 1].contiguous(), head, c)
    return rows


@dataclasses.dataclass
class Parts:
    """float64 side of one WNORM binding: rows (P, n, D), w0 (D,), and per index the largest |row element| of its tensor"""
    rows: torch.Tensor
    w0: torch.Tensor
    slices: list
    launches: List[Launch]

    def __post_init__(self):
        self.tmax = torch.zeros(self.rows.shape[-1], dtype=F64)
        for _, a, b in self.slices:
            self.tmax[a:b] = self.rows[:, :, a:b].abs().max()
        self.launch_of = torch.full((self.rows.shape[-1],), -1, dtype=torch.long)
        for k, l in enumerate(self.launches):
            self.launch_of[l.index()] = k

    def _rows_at(self, idx):
        return self.rows if idx.numel() == self.rows.shape[-1] else self.rows[:, :, idx]

    def reference(self, idx, w=None):
        """ref (P, n) of the mask `idx` under the weights w (None: w0)"""
        w = self.w0 if w is None else w
        r = self._rows_at(idx)
        return ((r * r).reshape(-1, idx.numel()) @ w[idx]).reshape(self.rows.shape[:2])

    def bound(self, idx, w=None):
        """the bound (P, n) of the mask `idx`: 2^-24 (K_SQ sum w |r| max_tensor|r| + L ref), L as the header derives it"""
        w = self.w0 if w is None else w
        unit = (self._rows_at(idx).abs().reshape(-1, idx.numel()) @ (w[idx] * self.tmax[idx])).reshape(self.rows.shape[:2])
        ks = sorted(set(self.launch_of[idx].tolist()))
        assert ks and ks[0] >= 0
        L = max(self.launches[k].L for k in ks) + (len(ks) if len(ks) > 1 else 0)
        return EPS * (K_SQ * unit + L * self.reference(idx, w))

    def check(self, label, got, idx, w=None):
        """assert |got - ref| <= bound for every pair; returns the worst error / bound"""
        ref, bound = self.reference(idx, w), self.bound(idx, w)
        err = (got.double().cpu().reshape(ref.shape) - ref).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        assert bool((err <= bound).all()), f"{label}: |v - ref| is {ratio:.3g} x the bound (ref {ref.flatten().tolist()})"
        return ratio

    # the masks ---------------------------------------------------------------------------------------------
    def tensor_masks(self):
        return [(name, torch.arange(a, b)) for name, a, b in self.slices]

    def block_masks(self):
        """[(launch, [(label, indices)])]: the output blocks of every launch (a partition of the launch's indices)"""
        return [(l, l.blocks()) for l in self.launches]

    def edge_masks(self):
        return [m for l in self.launches if l.kind != "reduce" for m in l.edges()]

    def all_indices(self):
        return torch.arange(self.rows.shape[-1])


def positive_weights(D, seed=4):
    """w0 in [0.05, 1.05), float32-representable (the weights of tests/test_wnorm.py)"""
    return (torch.rand(D, dtype=F64, generator=torch.Generator().manual_seed(seed)) + 0.05).float().double()


@functools.lru_cache(maxsize=None)
def binding(name):
    """(net, state, Z, U) of net `name` at n = 3, P = 2: float64, the probes float32-representable"""
    build, seed = NETS[name]
    net = build()
    state = create_state(net, seed, dtype=F64)
    Z = torch.rand(N_EX, *net.tensors[0], dtype=F64, generator=torch.Generator().manual_seed(seed))
    U = torch.randn(N_PROBES, N_EX, net.tensors[net.out][2], dtype=F64, generator=torch.Generator().manual_seed(3))
    return net, state, Z, U.float().double()


@functools.lru_cache(maxsize=None)
def wnorm_parts(name) -> Parts:
    """the float64 side of the WNORM tests on net `name` (head 'l', c = 0.7); built once and never written to"""
    net, state, Z, U = binding(name)
    rows = emulator_rows(net, state, Z, U, nv.HEAD_L, HEAD_C)
    assert bool(rows.isfinite().all())
    return Parts(rows, positive_weights(rows.shape[-1]), tensor_slices(state.params), launches_of(net, state.params))


def parts_of_rows(net, params, rows) -> Parts:
    """the float64 side of a binding whose rows exist already (the 517 pairs of ``many_pairs``)"""
    return Parts(rows, positive_weights(rows.shape[-1]), tensor_slices(params), launches_of(net, params))


def run_wnorm_checks(parts: Parts, call, what, blocks=True, edges=False):
    """Every part-by-part check of one WNORM binding.  ``call(w)`` is the sweep under the (D,) float64 weights w (None:
    no weights) and returns its (P, n) result; the GPU test passes ``vjp_wnorm``, the CPU test a stand-in.  Returns the
    worst error / bound; an AssertionError names the failing mask."""
    D = parts.rows.shape[-1]
    every = parts.all_indices()
    shape = parts.rows.shape[:2]
    seen = {}

    def masked(idx):
        key = idx.numpy().tobytes()
        if key not in seen:
            w = torch.zeros(D, dtype=F64)
            w[idx] = parts.w0[idx]
            seen[key] = call(w).double().cpu().reshape(shape)
        return seen[key]

    worst = 0.0
    # the unmasked total, and w=None against w = ones
    total = call(parts.w0).double().cpu()
    worst = max(worst, parts.check(f"{what}: unmasked", total, every))
    ones = torch.ones(D, dtype=F64)
    v_none, v_ones = call(None).double().cpu(), call(ones).double().cpu()
    worst = max(worst, parts.check(f"{what}: w=None", v_none, every, ones), parts.check(f"{what}: w=ones", v_ones, every, ones))
    assert bool(((v_none - v_ones).abs().reshape(shape) <= parts.bound(every, ones)).all()), \
        f"{what}: w=None and w=ones differ by more than the bound"
    # per tensor, and their complement
    acc = torch.zeros_like(parts.reference(every))
    for name, idx in parts.tensor_masks():
        v = masked(idx)
        assert bool((parts.reference(idx) > 0).all()), f"{what}: tensor {name}: a pair with a zero reference"
        worst = max(worst, parts.check(f"{what}: tensor {name}", v, idx))
        acc += v
    assert bool(((acc - total.reshape(acc.shape)).abs() <= parts.bound(every)).all()), \
        f"{what}: the per-tensor masks do not add up to the unmasked call"
    # per output block of every launch, and their complement
    if blocks:
        for l, parts_l in parts.block_masks():
            acc = torch.zeros_like(acc)
            for label, idx in parts_l:
                v = masked(idx)
                assert bool((parts.reference(idx) > 0).all()), f"{what}: {label}: a pair with a zero reference"
                worst = max(worst, parts.check(f"{what}: {label}", v, idx))
                acc += v
            whole = masked(l.index())
            assert bool(((acc - whole).abs() <= parts.bound(l.index())).all()), \
                f"{what}: the blocks of {l.label} do not add up to the launch"
    if edges:
        for label, idx in parts.edge_masks():
            assert bool((parts.reference(idx) > 0).all()), f"{what}: {label}: a pair with a zero reference"
            worst = max(worst, parts.check(f"{what}: {label}", masked(idx), idx))
    return worst


# --------------------------------------------------------------------------------------------- EWNORM and EIGEN
@dataclasses.dataclass
class Block:
    """one layer block of the eigen sweeps: [bias (N)] + kernel (M x N) read as an (Mt, N) matrix"""
    label: str
    off: int
    Mt: int
    N: int
    T: int                                   # output pixels
    bias: bool

    def launch(self) -> Launch:
        """the weighted-norm launch of the projected pair: a 1 x 1 convolution with Mt channels"""
        if self.T > 1:
            t = wgrad_tile(self.Mt, self.N)
            return Launch(self.label, "tile", 0, self.Mt, self.N, L=l_tile(t), route=tile_label(t))
        return Launch(self.label, "dense", 0, self.Mt, self.N, L=l_dense(self.Mt), route="wgrad_wnorm_dense")

    def masks(self):
        """[(label, (Mt, N) 0/1 float64 mask on R)]: the whole block, each output block of the launch, row 0 (the bias
        row where the block has one), row Mt - 1, column N - 1"""
        l = self.launch()

        def of(idx):
            m = torch.zeros(self.Mt * self.N, dtype=F64)
            m[idx] = 1.0
            return m.reshape(self.Mt, self.N)
        out = [(f"{self.label} whole", of(l.index()))]
        out += [(lab, of(idx)) for lab, idx in l.blocks()]
        out += [(f"{self.label} row {m}", of(l.index(rows=[m]))) for m in (0, self.Mt - 1)]
        out += [(f"{self.label} column {self.N - 1}", of(l.index(cols=[self.N - 1])))]
        return out


def blocks_of(state) -> List[Block]:
    return [Block(u.kernel[-2], off, Mt, N, T, b) for u, off, Mt, N, T, b in kf.blocks_of(state)]


def householder(m, g):
    """I - 2 v v^T / v^T v (``_householder`` of tests/test_ekfac_sweep.py, on the CPU)"""
    v = torch.randn(m, generator=g, dtype=F64)
    return (torch.eye(m, dtype=F64) - (2.0 / float(v @ v)) * torch.outer(v, v)).contiguous()


def general(m, g):
    """I + 0.3 randn / sqrt(m): well conditioned, no rotation"""
    return (torch.eye(m, dtype=F64) + 0.3 * torch.randn(m, m, generator=g, dtype=F64) / m ** 0.5).contiguous()


def triples_of(blocks, kind, seed=8):
    """[(V, R, Ub)] float64 CPU: the bases of `kind` ('householder' | 'general') and positive random R"""
    g = torch.Generator().manual_seed(seed)
    make = householder if kind == "householder" else general
    return [(make(b.Mt, g), (torch.rand(b.Mt, b.N, generator=g, dtype=F64) + 0.05).float().double(), make(b.N, g)) for b in blocks]


def products(ats, Gs, triples, absolute=False):
    """``kfac_predict_sweep_ref.projected_products`` from patches and cotangents that exist already; ``absolute``: the
    twin on the absolute values of every operand"""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    return [torch.einsum("itj,iktm->ikjm", f(at) @ f(V), f(G) @ f(Ub)) for at, G, (V, _, Ub) in zip(ats, Gs, triples)]


@dataclasses.dataclass
class EigenSide:
    """float64 side of one EWNORM / EIGEN binding and basis kind: per block T and |T| under the probes U, (P, n, Mt, N)"""
    blocks: List[Block]
    triples: list
    T: list
    Tabs: list
    rem_idx: torch.Tensor
    rem_rows: torch.Tensor                   # (P, n, r): the emulator's raw rows at rem_idx
    rem_slices: list                         # [(label, positions in rem_idx)]
    rem_tmax: torch.Tensor

    def ewnorm_check(self, label, got, l, mask, C):
        """block l under R * mask: returns the worst error / unit over the pairs and asserts the bound when C is given"""
        R = self.triples[l][1] * mask
        ref = torch.einsum("jm,pijm->pi", R, self.T[l] ** 2)
        unit = EPS * torch.einsum("jm,pijm->pi", R, self.Tabs[l]) * self.Tabs[l].max()
        err = (got.double().cpu().reshape(ref.shape) - ref).abs()
        L = self.blocks[l].launch().L
        ratio = (err / unit.clamp_min(1e-300)).max().item()
        assert bool((ref > 0).all()), f"{label}: a pair with a zero reference"
        if C is not None:
            assert bool((err <= C * unit + EPS * L * ref).all()), f"{label}: error {ratio:.3g} units > {C} units + {L} x 2^-24 ref"
        return ratio

    def remainder_check(self, label, got, var, pos):
        """the reduce term of the remainder positions `pos` under the variances `var` (r,): the WNORM bound"""
        ref = (self.rem_rows[:, :, pos] ** 2 * var[pos]).sum(-1)
        unit = (self.rem_rows[:, :, pos].abs() * self.rem_tmax[pos] * var[pos]).sum(-1)
        bound = EPS * (K_SQ * unit + L_REDUCE * ref)
        err = (got.double().cpu().reshape(ref.shape) - ref).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        assert bool((ref > 0).all()), f"{label}: a pair with a zero reference"
        assert bool((err <= bound).all()), f"{label}: |v - ref| is {ratio:.3g} x the bound"
        return ratio

    def eigen_check(self, label, got, l, canary, C):
        """Lam_l (Mt, N) float64 after the ADD into `canary`: element by element; returns the worst error in units"""
        ref = (self.T[l] ** 2).sum((0, 1))
        want = canary.double().cpu() + ref
        unit = EPS * self.Tabs[l].sum((0, 1)) * self.Tabs[l].max()
        err = (got.double().cpu() - want).abs()
        ratio = (err / unit.clamp_min(1e-300)).max().item()
        if C is not None:
            bad = (err > C * unit + EPS * 4 * want).nonzero()
            assert bad.numel() == 0, (f"{label}: element {bad[0].tolist()} of Lam: error up to {ratio:.3g} units > {C} units "
                                      f"+ 4 x 2^-24 want")
        return ratio


@functools.lru_cache(maxsize=None)
def _patches(name):
    net, state, Z, U = binding(name)
    _, ats, Gs = kf.patches_and_cotangents(state, Z)
    return ats, Gs


@functools.lru_cache(maxsize=None)
def eigen_side(name, kind) -> EigenSide:
    net, state, Z, U = binding(name)
    blocks = blocks_of(state)
    triples = triples_of(blocks, kind)
    ats, Gs = _patches(name)
    T = [torch.einsum("pik,ikjm->pijm", U, t) for t in products(ats, Gs, triples)]
    Tabs = [torch.einsum("pik,ikjm->pijm", U.abs(), t) for t in products(ats, Gs, triples, absolute=True)]
    rem_idx = kf.remainder_of(state)
    rem_rows, rem_slices, rem_tmax = torch.zeros(N_PROBES, N_EX, 0, dtype=F64), [], torch.zeros(0, dtype=F64)
    if rem_idx.numel():
        rows = emulator_rows(net, state, Z, U, nv.HEAD_IN, 1.0)
        rem_rows = rows[:, :, rem_idx]
        rem_tmax = torch.zeros(rem_idx.numel(), dtype=F64)
        for lab, a, b in tensor_slices(state.params):
            pos = ((rem_idx >= a) & (rem_idx < b)).nonzero().reshape(-1)
            if pos.numel():
                assert pos.numel() == b - a
                rem_slices.append((lab, pos))
                rem_tmax[pos] = rows[:, :, a:b].abs().max()
    return EigenSide(blocks, triples, T, Tabs, rem_idx, rem_rows, rem_slices, rem_tmax)
