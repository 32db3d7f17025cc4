"""CPU: the checkers of tests/wnorm_part_cases.py bite, their masks are partitions, and every reference they divide by
is non-zero.

The stand-in for the GPU result is the float64 reference rounded to float32, computed with the weights a subtly wrong
kernel would see: (1) one op's weights lost, (2) the last row of one tile lost, (3) one column weighted with its
neighbour's weights, (4) red1 weighted with red0's slice.  The old criterion (max|v - ref| <= 1e-5 max ref on the
unmasked total, tests/test_wnorm.py) passes (1) and (2) on net a; the part-by-part checks fail all four.

(1) needs an op below 1e-5 of the total.  Under the uniform weights of the tests the smallest op of net a, the bias of
Conv_0, is 7e-4 of it, so the old criterion is tried with that bias weighted 2^-7 as low as the rest — the variances of
a diagonal posterior spread over far more than two orders of magnitude.  (2) takes row 639 of a/Conv_1, the last row of
its fifth 128-row tile: 6e-6 of the total as the weights stand.
"""
import pytest
import torch

import kfac_predict_sweep_ref as pr
import wnorm_part_cases as wc

F64 = torch.float64
OLD_TOL = 1e-5                                               # tests/test_wnorm.py


def _standin(parts, see=None):
    """call(w) -> (P, n) float32: the float64 weighted norms under the weights the kernel sees, rounded once"""
    D = parts.rows.shape[-1]

    def call(w):
        w = torch.ones(D, dtype=F64) if w is None else w.clone()
        return ((parts.rows ** 2) @ (see(w) if see else w)).float()
    return call


def _old_criterion_passes(parts, call, w):
    ref = parts.reference(parts.all_indices(), w)
    return ((call(w).double() - ref).abs().max() / ref.max()).item() <= OLD_TOL


def _mask_fails(parts, call, idx):
    """does the check of the mask `idx` alone fail on the stand-in?"""
    w = torch.zeros_like(parts.w0)
    w[idx] = parts.w0[idx]
    try:
        parts.check("mask", call(w), idx)
    except AssertionError:
        return True
    return False


def _launch(parts, label):
    return next(l for l in parts.launches if l.label == label)


def _lose(idx):
    def see(w):
        w[idx] = 0.0
        return w
    return see


def _shift_column(l, c):
    """column c of the matrix of launch l is weighted with the weights of column c - 1"""
    def see(w):
        w[l.index(cols=[c])] = w[l.index(cols=[c - 1])]
        return w
    return see


def _red1_with_red0(l):
    (_, o0), (_, o1) = l.reds

    def see(w):
        w[o1:o1 + l.N] = w[o0:o0 + l.N]
        return w
    return see


@pytest.mark.parametrize("name", wc.WNORM_NETS)
def test_unperturbed_stand_in_passes_and_no_reference_is_zero(name):
    """run_wnorm_checks asserts a non-zero reference for every pair of every per-tensor and per-block mask, and of every
    edge mask on the nets the edge masks run on"""
    parts = wc.wnorm_parts(name)
    worst = wc.run_wnorm_checks(parts, _standin(parts), f"net {name}", edges=name in wc.EDGE_NETS)
    assert worst <= 1.0
    if name in wc.EDGE_NETS:
        assert bool((parts.rows != 0).all()), "a tanh net with a dead row element"


def test_old_criterion_passes_a_lost_op_and_a_lost_tile_row_on_net_a():
    parts = wc.wnorm_parts("a")
    bias = _launch(parts, "Conv_0/bias")
    w = parts.w0.clone()
    w[bias.index()] *= 2.0 ** -7
    assert _old_criterion_passes(parts, _standin(parts, _lose(bias.index())), w)                  # (1): the gap
    conv1 = _launch(parts, "Conv_1/kernel")
    assert conv1.grid() == (128, 64)
    assert _old_criterion_passes(parts, _standin(parts, _lose(conv1.index(rows=[639]))), parts.w0)  # (2): the gap
    # ... and it is not blind: a lost op of ordinary size fails it
    assert not _old_criterion_passes(parts, _standin(parts, _lose(_launch(parts, "Conv_2/kernel").index())), parts.w0)


def test_part_checks_fail_a_lost_op():
    parts = wc.wnorm_parts("a")
    idx = _launch(parts, "Conv_0/bias").index()
    call = _standin(parts, _lose(idx))
    with pytest.raises(AssertionError, match="net a: unmasked"):                   # 7e-4 of the total: 86 x the bound
        wc.run_wnorm_checks(parts, call, "net a")
    assert _mask_fails(parts, call, idx)                                            # its own mask: 0 against ref > 0
    # at 2^-7 of its weight, where the old criterion passes it, the weighted total passes too; its own mask does not
    w = parts.w0.clone()
    w[idx] *= 2.0 ** -7
    light = wc.Parts(parts.rows, w, parts.slices, parts.launches)
    light.check("net a: unmasked", _standin(light, _lose(idx))(w), light.all_indices())
    assert _mask_fails(light, _standin(light, _lose(idx)), idx)
    with pytest.raises(AssertionError, match="net a"):
        wc.run_wnorm_checks(light, _standin(light, _lose(idx)), "net a")


def test_part_checks_fail_a_lost_tile_row():
    parts = wc.wnorm_parts("a")
    conv1 = _launch(parts, "Conv_1/kernel")
    call = _standin(parts, _lose(conv1.index(rows=[639])))
    with pytest.raises(AssertionError, match="net a"):
        wc.run_wnorm_checks(parts, call, "net a")
    label, tile = conv1.blocks()[4]
    assert label == "Conv_1/kernel block (4,0)" and _mask_fails(parts, call, tile)  # the tile that lost its last row
    assert not _mask_fails(parts, call, conv1.blocks()[3][1])                       # ... and no other
    # on the tanh twin the single-row mask sees a lost row whatever its size
    twin = wc.wnorm_parts("a_tanh")
    conv2 = _launch(twin, "Conv_2/kernel")
    call = _standin(twin, _lose(conv2.index(rows=[127])))
    assert "Conv_2/kernel row 127" in [lab for lab, _ in twin.edge_masks()]
    assert _mask_fails(twin, call, conv2.index(rows=[127])) and not _mask_fails(twin, call, conv2.index(rows=[128]))
    with pytest.raises(AssertionError, match="net a_tanh"):
        wc.run_wnorm_checks(twin, call, "net a_tanh", edges=True)


def test_part_checks_fail_a_shifted_column():
    parts = wc.wnorm_parts("a_tanh")
    l = _launch(parts, "Conv_3/kernel")
    call = _standin(parts, _shift_column(l, l.N - 1))
    assert "Conv_3/kernel column 19" in [lab for lab, _ in parts.edge_masks()]
    assert _mask_fails(parts, call, l.index(cols=[19])) and _mask_fails(parts, call, l.index(cols=[18]))
    assert not _mask_fails(parts, call, l.index(cols=[17]))
    assert _mask_fails(parts, call, l.index())                                      # the tensor's mask sees it too
    with pytest.raises(AssertionError, match="net a_tanh"):
        wc.run_wnorm_checks(parts, call, "net a_tanh", edges=True)


def test_part_checks_fail_red1_weighted_with_the_slice_of_red0():
    parts = wc.wnorm_parts("bn_maxpool")
    l = _launch(parts, "BatchNorm_1")
    assert [lab for lab, _ in l.reds] == ["BatchNorm_1/bias", "BatchNorm_1/scale"]
    call = _standin(parts, _red1_with_red0(l))
    masks = dict(parts.tensor_masks())
    assert _mask_fails(parts, call, masks["BatchNorm_1/scale"])                     # weighted 0: nothing comes back
    assert not _mask_fails(parts, call, masks["BatchNorm_0/scale"])
    with pytest.raises(AssertionError, match="net bn_maxpool"):
        wc.run_wnorm_checks(parts, call, "net bn_maxpool")


# ------------------------------------------------------------------------------------------------- mask bookkeeping
@pytest.mark.parametrize("name", sorted(wc.NETS))
def test_every_partition_covers_each_index_once_and_the_tiles_are_those_of_the_dispatcher(name):
    net, state, Z, U = wc.binding(name)
    slices = wc.tensor_slices(state.params)
    launches = wc.launches_of(net, state.params)
    D = slices[-1][2]
    count = torch.zeros(D, dtype=torch.long)
    for _, a, b in slices:
        count[a:b] += 1
    assert bool((count == 1).all())                                                 # the tensors partition D
    count.zero_()
    for l in launches:
        inner = torch.zeros(D, dtype=torch.long)
        for _, idx in l.blocks():
            inner[idx] += 1
        assert torch.equal(inner.nonzero().reshape(-1), l.index().sort().values) and int(inner.max()) == 1, l.label
        count += inner
        if l.kind == "tile":
            # with_wgrad_tile, the way _grouped_launches of tests/test_kernel_routes.py restates it
            bm, bn = (64 if l.M <= 64 else 128), (128 if l.N > 64 else 64 if l.N > 32 else 32)
            assert l.grid() == (bm, bn) and len(l.blocks()) == -(-l.M // bm) * -(-l.N // bn), l.label
            for k, (_, idx) in enumerate(l.blocks()):                               # block k = tile_m * tiles_n + tile_n
                r, c = divmod(k, -(-l.N // bn))
                m, col = (idx - l.off) // l.N, (idx - l.off) % l.N
                assert int(m.min()) == bm * r and int(m.max()) == min(l.M, bm * (r + 1)) - 1
                assert int(col.min()) == bn * c and int(col.max()) == min(l.N, bn * (c + 1)) - 1
        elif l.kind == "dense":
            assert len(l.blocks()) == -(-l.N // 64)
        else:
            cb = l.grid()[1]
            assert cb <= 64 and (cb == 1 or cb // 2 < l.N) and (cb == 64 or cb >= l.N) and len(l.blocks()) == -(-l.N // cb)
        if l.kind != "reduce":
            for label, idx in l.edges():
                assert idx.numel() in (1, l.M, l.N) and bool(inner[idx].all()), label
            labels = [lab for lab, _ in l.edges()]
            assert f"{l.label} row 0" in labels and f"{l.label} row {l.M - 1}" in labels
            assert f"{l.label} column 0" in labels and f"{l.label} column {l.N - 1}" in labels
    assert bool((count == 1).all())                                                 # the launches' blocks partition D
    # the tile labels are those the census of the library lists
    assert {wc.tile_label(wc.wgrad_tile(M, N)) for M in (64, 65) for N in (32, 33, 64, 65)} == \
        {f"wgrad_wnorm<{t}>" for t in ("2,1,1,1", "4,1,1,1", "2,2,1,1", "4,1,1,2", "2,2,1,2", "2,2,2,2")}
    assert wc.l_tile((2, 2, 2, 2)) == 76 and wc.l_tile((2, 1, 1, 1)) == 26 and wc.l_dense(960) == 267


def test_restated_nets_are_the_nets_of_the_tests_they_come_from():
    import test_kernel_routes as kr
    import test_small_ops as so
    for mine, theirs in ((wc.net_a(), kr._net_a()), (wc.net_b(), kr._net_b()), (wc.net_bn_maxpool(), so._net_bn_maxpool()),
                         (wc.net_lenet(), so._net_lenet())):
        assert mine.units == theirs.units and mine.tensors == theirs.tensors
    net, state, Z, U = wc.binding("a")
    assert [(n, a, b) for n, a, b in wc.tensor_slices(state.params)] == \
        [("/".join(map(str, n[-2:])), a, b) for n, a, b in kr._tensor_slices(state.params)]
    for twin, act in (("a_tanh", "tanh"), ("b_tanh", "tanh")):
        assert all(u.act == act for u in wc.binding(twin)[0].units[:-1] if u.kind == "conv")
    for twin in ("a_bias", "b_bias"):
        assert all(u.bias is not None for u in wc.binding(twin)[0].units if u.kind == "conv")


# ------------------------------------------------------------------------------------------------- EWNORM and EIGEN
def test_the_eigen_bindings_reach_every_tile_with_odd_row_counts():
    routes, odd_wide = set(), set()
    for name in wc.EIGEN_NETS:
        state = wc.binding(name)[1]
        for b in wc.blocks_of(state):
            l = b.launch()
            routes.add(l.route)
            if l.kind == "tile" and b.Mt % 2 == 1 and (l.grid()[0] == 128 or l.grid()[1] >= 64):
                odd_wide.add(l.route)
    assert routes == {wc.tile_label(t) for t in ((2, 1, 1, 1), (4, 1, 1, 1), (2, 2, 1, 1), (4, 1, 1, 2), (2, 2, 1, 2), (2, 2, 2, 2))} | \
        {"wgrad_wnorm_dense"}
    # an odd C = Mt on the 128-row tiles and on the 64- and 128-column tiles
    assert {"wgrad_wnorm<4,1,1,2>", "wgrad_wnorm<2,2,2,2>", "wgrad_wnorm<4,1,1,1>", "wgrad_wnorm<2,2,1,1>"} <= odd_wide
    assert wc.binding("bn_maxpool")[1] is not None and wc.eigen_side("bn_maxpool", "householder").rem_idx.numel() == 2 * (64 + 24)


@pytest.mark.parametrize("name", ["b", "bn_maxpool"])
def test_eigen_references_are_those_of_the_float64_helper(name):
    net, state, Z, U = wc.binding(name)
    side = wc.eigen_side(name, "general")
    want = pr.block_terms(state, Z, side.triples, U)
    for l, (b, t) in enumerate(zip(side.blocks, want)):
        got = torch.einsum("jm,pijm->pi", side.triples[l][1], side.T[l] ** 2)
        assert ((got - t).abs().max() / t.abs().max()).item() <= 1e-13, b.label
        assert bool((side.Tabs[l] >= side.T[l].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("kind", ["householder", "general"])
@pytest.mark.parametrize("name", wc.EIGEN_NETS)
def test_eigen_checkers_pass_the_rounded_reference_and_fail_a_lost_row(name, kind):
    side = wc.eigen_side(name, kind)
    for l, b in enumerate(side.blocks):
        R = side.triples[l][1]
        for label, mask in b.masks():
            ref = torch.einsum("jm,pijm->pi", R * mask, side.T[l] ** 2)                # (asserted non-zero by the checker)
            assert side.ewnorm_check(f"{name} {label}", ref.float(), l, mask, 1.0) <= 1.0
        # a kernel that loses the bias row of a block: nothing comes back under the mask of row 0.  (Without a bias
        # row 0 is one direction of the basis among Mt, and in a reflector's basis it can be as small as the unit.)
        if b.bias:
            row0 = next(m for lab, m in b.masks() if lab.endswith("row 0"))
            with pytest.raises(AssertionError, match="row 0"):
                side.ewnorm_check(f"{name} {b.label} row 0", torch.zeros(wc.N_PROBES, wc.N_EX), l, row0, 64.0)
        canary = torch.full((b.Mt, b.N), 0.25, dtype=F64)
        lam = canary + (side.T[l] ** 2).sum((0, 1))
        assert side.eigen_check(f"{name} {b.label}", lam, l, canary, 1.0) <= 1.0
        j = int((lam - canary).sum(1).argmax())                                    # the ADD of one row is lost
        lam[j] = canary[j]
        with pytest.raises(AssertionError, match=rf"element \[{j}, "):
            side.eigen_check(f"{name} {b.label}", lam, l, canary, 64.0)
    for label, pos in side.rem_slices:
        var = torch.rand(side.rem_idx.numel(), dtype=F64, generator=torch.Generator().manual_seed(1)) + 0.05
        ref = (side.rem_rows[:, :, pos] ** 2 * var[pos]).sum(-1)
        assert side.remainder_check(f"{name} {label}", ref.float(), var, pos) <= 1.0
