"""GPU: the weighted-norm and eigen sweeps part by part — ``lip_vjp_wnorm`` (WNORM) tensor by tensor, output tile by
output tile, row, column and element; ``lip_vjp_eigen_wnorm`` (EWNORM) one layer block and one tile of R at a time;
``lip_vjp_eigen`` (EIGEN) element by element of Lam — against the float64 references of tests/wnorm_part_cases.py,
whose header derives the bounds.  tests/test_wnorm_parts_cpu.py shows that the same checkers fail on a lost op, a lost
tile row, a shifted column and a wrong reduce slice.

Everything goes through ``vjp_wnorm``, ``kfac_predict_sweep(..., probes=U)`` and ``kfac_eigen_sqsums_sweep(..., probes=U)``
at n = 3, P = 2 (and the per-tensor masks on the 517 pairs of ``test_kernel_routes.many_pairs``).

Measured on MI355X (run with -s):
  WNORM, worst |v - ref| / bound over every mask of a net (bound: K_SQ = 16 units + L ref):
    a 0.044  b 0.076  c 0.055  d 0.055  bn_maxpool 0.10  lenet 0.37  a_tanh 0.096  b_tanh 0.18
    517 pairs: a 0.17  b 0.14
  EWNORM, worst |v - ref| / (2^-24 sum R |T| max|T|) over the masks of a net, Householder / general bases:
    a 0.766 / 0.744  b 0.658 / 0.618  c 0.724 / 1.39  d 0.376 / 0.978  a_bias 0.143 / 0.36  b_bias 0.26 / 0.436
    bn_maxpool 0.186 / 1.03 (its remainder, the reduce term under the WNORM bound: 0.10 of the bound)
    worst 1.39: C_EWNORM = 4 x 1.39 = 5.56
  EIGEN, worst |Lam - want| / (2^-24 sum_{p,i} |T| max|T|) over the elements of a net's blocks, likewise:
    a 1.43 / 0.727  b 0.384 / 0.429  c 2.07 / 1.64  d 1.22 / 0.936  a_bias 0.385 / 0.584  b_bias 0.572 / 0.536
    bn_maxpool 0.842 / 1.59
    worst 2.07: C_EIGEN = 4 x 2.07 = 8.28
  (``lip_vjp_sqsum``'s worst on the unprojected product is 4.2 of its unit; the twin |T| is larger than |T|, so these
  ratios come out below it)
"""
import ctypes

import pytest
import torch

import wnorm_part_cases as wc
from lip_amd import _native as nv
from lip_amd.engine import LinearizedNet
from lip_amd.ggn import clear_engine_cache

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
DEV = "cuda"

# 4 x the worst ratio measured on MI355X (the figures of the header)
C_EWNORM = 4 * 1.39
C_EIGEN = 4 * 2.07

TILES = {wc.tile_label(t) for t in ((2, 1, 1, 1), (4, 1, 1, 1), (2, 2, 1, 1), (4, 1, 1, 2), (2, 2, 1, 2), (2, 2, 2, 2))}
_ENGINES = {}


def _engine(name):
    """the binding of tests/test_kernel_routes.py::_bind on net `name`; one engine per net for the whole module"""
    if name not in _ENGINES:
        net, state, Z, U = wc.binding(name)
        _ENGINES[name] = LinearizedNet(state, Z, "classifier", workspace_bytes=1 << 28, max_chunk=wc.N_PROBES)
    return _ENGINES[name]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _ENGINES.clear()
    clear_engine_cache()


def _census(lib):
    n = lib.lip_debug_wnorm_route_count()
    counts, names = (ctypes.c_int64 * n)(), (ctypes.c_char_p * n)()
    nv.check(lib.lip_debug_wnorm_routes(counts, n, names), "lip_debug_wnorm_routes")
    return {names[i].decode(): counts[i] for i in range(n) if counts[i]}


def _labels(lib):
    n = lib.lip_debug_wnorm_route_count()
    names = (ctypes.c_char_p * n)()
    nv.check(lib.lip_debug_wnorm_routes(None, n, names), "lip_debug_wnorm_routes")
    return {names[i].decode() for i in range(n)}


def _sweep(eng, U):
    """call(w) of wnorm_part_cases.run_wnorm_checks: ``vjp_wnorm`` with head 'l', c = 0.7"""
    Ud = U.float().to(DEV)

    def call(w):
        v = eng.vjp_wnorm(Ud, None if w is None else w.float().to(DEV), "l", wc.HEAD_C)
        torch.cuda.synchronize()
        return v
    return call


# ------------------------------------------------------------------------------------------------------------ WNORM
@pytest.mark.parametrize("name", wc.WNORM_NETS)
def test_wnorm_tensor_by_tensor_tile_by_tile(name):
    parts = wc.wnorm_parts(name)
    eng = _engine(name)
    _census(eng.lib)                                             # clear
    worst = wc.run_wnorm_checks(parts, _sweep(eng, wc.binding(name)[3]), f"net {name}", edges=name in wc.EDGE_NETS)
    census = set(_census(eng.lib))
    want = {l.route for l in parts.launches} | {"wnorm_finish"}
    assert want <= census, f"net {name}: {sorted(want - census)} not launched ({sorted(census)})"
    print(f"wnorm net {name}: worst |v - ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("which", ["a", "b"])
def test_wnorm_tensor_by_tensor_on_517_pairs(which):
    """several pairs per block and a short last group: the per-tensor masks on the shared 517-pair bindings"""
    from test_kernel_routes import MANY_N, MANY_P, assert_several_pairs_per_group, many_pairs
    net, state, _, _ = wc.binding(which)
    assert_several_pairs_per_group(net, MANY_P * MANY_N)
    eng, slices, U, rows = many_pairs(which)
    parts = wc.parts_of_rows(net, state.params, rows)
    assert [(a, b) for _, a, b in slices] == [(a, b) for _, a, b in parts.slices]
    worst = wc.run_wnorm_checks(parts, _sweep(eng, U), f"net {which}, 517 pairs", blocks=False)
    print(f"wnorm net {which}, 517 pairs: worst |v - ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", wc.WNORM_NETS)
def test_wnorm_masked_calls_are_bitwise_stable_and_out_accumulates(name):
    parts = wc.wnorm_parts(name)
    eng = _engine(name)
    call = _sweep(eng, wc.binding(name)[3])
    D = parts.rows.shape[-1]
    other = wc.positive_weights(D, seed=19)
    for l, blocks in parts.block_masks():
        label, idx = blocks[-1]                                  # the ragged last block of every launch
        w = torch.zeros(D, dtype=F64)
        w[idx] = parts.w0[idx]
        a = call(w)
        assert torch.equal(a, call(w)), f"{label}: a masked call repeated differs"
        # the weights outside the mask are w0's or another vector's: the masked vector, and the result, are the same
        moved = other.clone()
        moved[idx] = parts.w0[idx]
        keep = torch.zeros(D, dtype=F64)
        keep[idx] = 1.0
        assert torch.equal(a, call(moved * keep)), f"{label}: the result depends on w0 outside the mask"
        # out=: the part is added to the pre-filled block, float(double(out0) + part), within one ulp of the sum
        out0 = (torch.rand(a.shape, generator=torch.Generator().manual_seed(5)) + 0.5).to(DEV) * a
        y = eng.vjp_wnorm(wc.binding(name)[3].float().to(DEV), w.float().to(DEV), "l", wc.HEAD_C, out=out0.clone())
        torch.cuda.synchronize()
        total = out0.double() + a.double()
        assert bool(((y.double() - total).abs() <= 2.0 ** -23 * total).all()), f"{label}: out= does not accumulate"


# ----------------------------------------------------------------------------------------------------------- EWNORM
def _device_triples(side):
    return [tuple(t.to(DEV).contiguous() for t in tr) for tr in side.triples]


NO_REM = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=F64))


@pytest.mark.parametrize("kind", ["householder", "general"])
@pytest.mark.parametrize("name", wc.EIGEN_NETS)
def test_ewnorm_block_by_block_tile_by_tile(name, kind):
    side = wc.eigen_side(name, kind)
    eng = _engine(name)
    U = wc.binding(name)[3].float()
    dev = _device_triples(side)
    zeros = [torch.zeros_like(R) for _, R, _ in dev]
    worst, worst_rem = 0.0, 0.0
    for l, b in enumerate(side.blocks):
        for label, mask in b.masks():
            fits = [(V, (R * mask.to(DEV)).contiguous() if k == l else zeros[k], Ub) for k, (V, R, Ub) in enumerate(dev)]
            got = eng.kfac_predict_sweep(fits, NO_REM, probes=U)
            torch.cuda.synchronize()
            assert got.dtype == F32 and tuple(got.shape) == (wc.N_PROBES, wc.N_EX)
            worst = max(worst, side.ewnorm_check(f"{name} ({kind}) {label}", got, l, mask, C_EWNORM))
    # all R = 0 and the remainder's variances set: the reduce term, per tensor of the remainder and whole
    if side.rem_idx.numel():
        fits = [(V, zeros[k], Ub) for k, (V, R, Ub) in enumerate(dev)]
        var = (torch.rand(side.rem_idx.numel(), dtype=F64, generator=torch.Generator().manual_seed(1)) + 0.05).float().double()
        every = torch.arange(side.rem_idx.numel())
        launches = len({label.split("/")[0] for label, _ in side.rem_slices})      # one reduce per BN layer (bias and scale)
        for label, pos in side.rem_slices + [("the whole remainder", every)]:
            v = torch.zeros_like(var)
            v[pos] = var[pos]
            got = eng.kfac_predict_sweep(fits, (side.rem_idx, v), probes=U)
            torch.cuda.synchronize()
            if pos is every:                                     # several launches, each rounded once by its finish
                ref = (side.rem_rows ** 2 * var).sum(-1)
                unit = (side.rem_rows.abs() * side.rem_tmax * var).sum(-1)
                bound = wc.EPS * (wc.K_SQ * unit + (wc.L_REDUCE + launches) * ref)
                assert bool(((got.double().cpu() - ref).abs() <= bound).all()), f"{name}: the whole remainder"
            else:
                worst_rem = max(worst_rem, side.remainder_check(f"{name} remainder {label}", got, var, pos))
    print(f"ewnorm net {name} ({kind}): worst error {worst:.3g} x 2^-24 sum R |T| max|T|; remainder {worst_rem:.3g} x the bound")


def test_ewnorm_bindings_launch_every_wnorm_route():
    """the twin of tests/test_wnorm.py::test_all_six_tiles_are_covered_by_the_two_nets for ``lip_vjp_eigen_wnorm``: the
    union over the bindings is every label of the census"""
    lib = nv.load()
    union = set()
    for name in wc.EIGEN_NETS:
        side = wc.eigen_side(name, "householder")
        eng = _engine(name)
        var = torch.full((side.rem_idx.numel(),), 0.5, dtype=F64)
        torch.cuda.synchronize()
        _census(lib)                                             # clear
        eng.kfac_predict_sweep(_device_triples(side), (side.rem_idx, var), probes=wc.binding(name)[3].float())
        torch.cuda.synchronize()
        census = set(_census(lib))
        want = {b.launch().route for b in side.blocks} | ({"reduce_wnorm"} if side.rem_idx.numel() else set()) | {"wnorm_finish"}
        assert census == want, f"net {name}: launched {sorted(census)}, expected {sorted(want)}"
        union |= census
    assert union == _labels(lib) == TILES | {"wgrad_wnorm_dense", "reduce_wnorm", "wnorm_finish"}


# ------------------------------------------------------------------------------------------------------------ EIGEN
@pytest.mark.parametrize("kind", ["householder", "general"])
@pytest.mark.parametrize("name", wc.EIGEN_NETS)
def test_eigen_second_moments_element_by_element(name, kind):
    side = wc.eigen_side(name, kind)
    eng = _engine(name)
    U = wc.binding(name)[3].float()
    bases = [(V, Ub) for V, _, Ub in _device_triples(side)]
    g = torch.Generator().manual_seed(6)
    canaries = [((torch.rand(b.Mt, b.N, dtype=F64, generator=g) + 0.5) * (T ** 2).sum((0, 1)).mean()).to(DEV)
                for b, T in zip(side.blocks, side.T)]
    lams = eng.kfac_eigen_sqsums_sweep(bases, [c.clone() for c in canaries], probes=U)
    torch.cuda.synchronize()
    again = eng.kfac_eigen_sqsums_sweep(bases, [c.clone() for c in canaries], probes=U)
    torch.cuda.synchronize()
    worst = 0.0
    for l, b in enumerate(side.blocks):
        assert torch.equal(lams[l], again[l]), f"{name} {b.label}: a second run differs"
        worst = max(worst, side.eigen_check(f"{name} ({kind}) {b.label}", lams[l], l, canaries[l], C_EIGEN))
    print(f"eigen net {name} ({kind}): worst error {worst:.3g} x 2^-24 sum |T| max|T|")
