"""CPU: the infrastructure of tests/test_krylov_ops.py is itself right — the float64 references against independent
torch expressions, the numpy Philox4x32-10 against the Random123 known answers and a scalar re-implementation of the two
fill layouts, what the case table covers (through the Python mirrors of the launch arithmetic), the exactness condition
of every exact input, and that the comparison bites."""
import numpy as np
import pytest
import torch

import krylov_harness as kh
from krylov_cases import (CASES, BY_NAME, FILL_CASES, KRYLOV_ROUTES, REFUSALS, ROW_LAUNCH, VALU_ONLY, dot_nt_plan,
                          gemm_nt_plan, nn_blocks, row_plan, rows_combine_plan, split_row)

F64 = torch.float64


# ---------------------------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(x[0]) for x in kh.philox4x32(ctr, key))
        assert got == want, [hex(g) for g in got]


def _philox_scalar(ctr64, seed):
    c = [ctr64 & 0xFFFFFFFF, ctr64 >> 32, 0x9E3779B9, 0xBB67AE85]
    k = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    for _ in range(10):
        m0, m1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(m1 >> 32) ^ c[1] ^ k[0], m1 & 0xFFFFFFFF, (m0 >> 32) ^ c[3] ^ k[1], m0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("seed", [0, 2 ** 32 + 5, 2 ** 64 - 1])
def test_rademacher_layout_against_a_scalar_loop(seed):
    total = 2 * 32 * 256 * 4 + 37
    ref = kh.ref_rademacher(total, seed)
    assert ref.shape == (total,) and set(np.unique(ref)) == {-1.0, 1.0}
    for e in (0, 1, 5, 1023, 1024, 4 * 255 + 3, 4 * 256, 4 * 256 * 7 + 2, 4 * 256 * 8, 4 * 256 * 31 + 1023, 32768, 32768 + 4 * 300 + 1,
              total - 1):
        q, h = divmod(e, 4)
        ch, rem = divmod(q, 32 * 256)
        i, t = divmod(rem, 256)
        u = _philox_scalar(ch * 256 + t, seed)
        bit = (u[i >> 3] >> (4 * (i & 7) + h)) & 1
        assert ref[e] == (1.0 if bit else -1.0), e
    assert abs(ref.mean()) < 0.02


def test_normal_layout_against_a_scalar_loop():
    import math
    total, seed = 1027, 2 ** 32 + 1
    ref, rad = kh.ref_normal(total, seed)
    for e in (0, 1, 2, 3, 4, 517, 1026):
        q, h = divmod(e, 4)
        u = _philox_scalar(q, seed)
        u1 = float(np.float32(np.float32(u[2 * (h // 2)] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24))
        u2 = float(np.float32(np.float32(u[2 * (h // 2) + 1] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24))
        ang = float(np.float32(6.283185307179586) * np.float32(u2))
        r = math.sqrt(-2.0 * math.log(u1))
        want = r * (math.cos(ang) if h % 2 == 0 else math.sin(ang))
        assert abs(ref[e] - want) <= 1e-14 * max(1.0, r) and abs(rad[e] - r) <= 1e-14 * max(1.0, r)
    big, _ = kh.ref_normal(200000, 3)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01


# ---------------------------------------------------------------------------------------------- references
def _ops(call):
    return {n: r.view(call.words).double() for n, r in call.arena.regs.items()}


def _sim(name, exact=False):
    c = BY_NAME[name]
    call = kh.BUILDERS[c.prim](c.d, exact, seed=5)
    words = kh.simulate(call)
    return c, call, words, {n: o.region.read(words).double() for n, o in call.outs.items()}


def test_references_against_independent_expressions():
    c, call, w, out = _sim("bdot/N43/off1")
    o = _ops(call)
    assert torch.allclose(out["out"][0], torch.einsum("pn,pn->p", o["X"], o["Y"]).float().double(), rtol=0, atol=0)

    c, call, w, out = _sim("axpby/a_vec/b_vec")
    o = _ops(call)
    a_s, b_s = 0.7, -1.3
    want = torch.stack([a_s * o["a"][0, p] * o["X"][p] + b_s * o["b"][0, p] * o["Y"][p] for p in range(3)])
    assert torch.equal(out["Y"], want.float().double())

    c, call, w, out = _sim("cg_update/active_mixed")
    o = _ops(call)
    for i, p in enumerate((0, 3)):
        a = o["rr_old"][0, p] / o["pAp"][0, p]
        assert torch.equal(out["x"][i], torch.add(o["x"][p], o["p"][p], alpha=a.item()).float().double())
        rr = torch.sub(o["r"][p], o["Ap"][p], alpha=a.item()).float().double()
        assert torch.equal(out["r"][i], rr)
        assert out["rr_new"][0, p].item() == pytest.approx(torch.linalg.vector_norm(rr).item() ** 2, rel=1e-6)
    assert out["rr_new"][0, 1] == 0 and out["rr_new"][0, 2] == 0

    c, call, w, out = _sim("cg_direction/active_ones")
    o = _ops(call)
    want = o["r"] + (o["rr_new"] / o["rr_old"]).T * o["p"]
    assert torch.equal(out["p"], want.float().double())

    c, call, w, out = _sim("multi_dot/k257")
    o = _ops(call)
    P, k, kmax, N = c.d["P"], c.d["k"], c.d["kmax"], c.d["N"]
    Q = o["Q"].reshape(P, kmax, N)
    want = torch.stack([Q[p, :k] @ o["w"][p] for p in range(P)])
    assert torch.allclose(out["c"], want.float().double(), rtol=0, atol=0)

    c, call, w, out = _sim("multi_axpy_norm/k257")
    o = _ops(call)
    P, k, kmax, N = c.d["P"], c.d["k"], c.d["kmax"], c.d["N"]
    Q = o["Q"].reshape(P, kmax, N)
    want = torch.stack([o["w"][p] - o["c"][p, :k] @ Q[p, :k] for p in range(P)]).float().double()
    assert torch.allclose(out["w"], want, rtol=0, atol=1e-7)
    assert torch.allclose(out["nrm2"][0], torch.linalg.vector_norm(out["w"], dim=1) ** 2, rtol=1e-6)

    c, call, w, out = _sim("scale_store/N2049")
    o = _ops(call)
    N = c.d["N"]
    want = o["w"] / o["nrm2"][0].sqrt()[:, None]
    assert torch.equal(out["Q"][:, :N], want.float().double()) and not out["Q"][:, N:].any()

    for name in ("dot_nt_f64/tile_part", "gemm_nt/K1023"):
        c, call, w, out = _sim(name)
        o = _ops(call)
        want = torch.einsum("mk,nk->mn", o["A"], o["B"])
        assert torch.allclose(out["C"], want, rtol=1e-15 if "f64" in name else 2e-7, atol=1e-13 if "f64" in name else 1e-5)

    c, call, w, out = _sim("gemm_nn_axpy/k6")
    o = _ops(call)
    want = torch.einsum("mk,kn->mn", o["T"], o["B"]) + 0.37 * o["Out"]
    assert c.d["v"] == "out" and torch.allclose(out["Out"], want, rtol=2e-7, atol=1e-6)

    c, call, w, out = _sim("rows_combine/r13")
    o = _ops(call)
    want = torch.stack([sum(float(np.float32(o["Cm"][i, j].item())) * o["Y"][j] for j in range(c.d["s"])) for i in range(c.d["r"])])
    want = want + c.d["zscale"] * o["Z"] if c.d.get("z") else want
    assert torch.allclose(out["Out"], want.float().double(), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------- coverage of the table
def _of(prim):
    return [c for c in CASES if c.prim == prim]


@pytest.mark.parametrize("prim", list(ROW_LAUNCH))
def test_table_covers_the_row_split(prim):
    pairs, g0, blocks, trips, capped, smallN = set(), set(), set(), set(), False, set()
    for c in _of(prim):
        if c.d.get("same") or "off_y" in c.d or "off_x" in c.d:
            continue
        rows, nb, tr, cap = row_plan(prim, c.d["P"], c.d["N"], c.d.get("off", 0))
        for (h, G, t), p in zip(rows, range(c.d["P"])):
            if G > 0:
                pairs.add((h, t))
            else:
                g0.add(c.d["N"])
                if c.d["N"] < (4 - (c.d.get("off", 0) + p * c.d["N"]) % 4) % 4:
                    smallN.add(c.d["N"])
        blocks.add(nb)
        trips.add(tr)
        capped |= cap
    assert pairs == {(h, t) for h in range(4) for t in range(4)}, sorted(pairs)
    assert {1, 2, 3} <= g0 and smallN, (g0, smallN)
    assert 1 in blocks and any(b > 1 for b in blocks) and any(t > 1 for t in trips)
    if prim == "bdot":
        assert capped


def test_split_row_mirror():
    for mis in range(4):
        for N in range(1, 40):
            h, G, t = split_row(mis, N)
            assert h + 4 * G + t == N and 0 <= t < 4 and (G == 0 or (mis + h) % 4 == 0) and h <= 3


def test_table_holds_the_listed_cases():
    d = lambda prim: [c.d for c in _of(prim)]                                   # noqa: E731
    ax = d("axpby")
    assert {(bool(x.get("a")), bool(x.get("b"))) for x in ax} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(x.get("b_s") == 0.0 for x in ax) and any(x.get("zero_b") for x in ax) and any(x.get("same") for x in ax)
    for prim in ("multi_dot", "multi_axpy_norm", "scale_store"):
        Ns = {x["N"] for x in d(prim)}
        assert {1, 2, 3, 4, 5, 2047, 2048, 2049, 4095, 4097} <= Ns
        assert {x.get("ldq_extra", 0) for x in d(prim)} >= {0, 8} and {x["P"] for x in d(prim)} >= {1, 3}
        assert {x.get("off", 0) for x in d(prim)} == {0, 1, 2, 3}
    for prim in ("multi_dot", "multi_axpy_norm"):
        assert {1, 255, 256, 257, 600} <= {x["k"] for x in d(prim)} and all(x.get("kmax", x["k"] + 2) > x["k"] for x in d(prim))
    ss = d("scale_store")
    assert any(x["j"] == 0 for x in ss) and any(x["j"] == x["kmax"] - 1 and x["j"] > 0 for x in ss) and any(x.get("inf_rows") for x in ss)
    for prim in ("cg_update", "cg_direction"):
        acts = [tuple(x["active"]) if x.get("active") else None for x in d(prim)]
        assert None in acts and (1, 1, 1, 1) in acts and (0, 0, 0, 0) in acts and any(a and 0 < sum(a) < 4 for a in acts)
    dn = d("dot_nt_f64")
    assert {1, 31, 32, 33, 63, 64, 65, 70, 900} <= {x["m"] for x in dn} | {x["n"] for x in dn}
    assert {1, 15, 16, 17, 31, 32, 33, 511, 512, 4099, 100003, 1084586} <= {x["K"] for x in dn}
    assert any(x.get("same") for x in dn) and any(x.get("lda_extra", 0) != x.get("ldb_extra", 0) for x in dn)
    assert {x.get("off_a", 0) for x in dn} >= {1, 2, 3} and {x.get("off_b", 0) for x in dn} >= {1, 2, 3}
    plans = {(x["m"], x["n"], x["K"]): dot_nt_plan(x["m"], x["n"], x["K"]) for x in dn}
    assert plans[(900, 900, 600)][0] == "dot_nt/quad/atomic" and plans[(900, 900, 600)][1][2] == 4
    assert plans[(850, 850, 2000)][0] == "dot_nt/tile/part"
    assert plans[(70, 70, 100003)][0] == "dot_nt/quad/part" and plans[(70, 70, 100003)][1][:2] == (3, 3)
    assert plans[(3, 5, 241)][0] == "dot_nt/tile/atomic" and plans[(8, 33, 4099)][0] == "dot_nt/tile/part"
    assert any(lbl.startswith("dot_nt/quad") and tm % 2 and tn % 2 for lbl, (tm, tn, _, _) in plans.values())
    assert any(K % kper for (_, _, K), (_, (_, _, ks, kper)) in plans.items() if ks > 1)
    rc = d("rows_combine")
    got = {(x["r"], rows_combine_plan(x["r"], x["s"])[1]) for x in rc}
    assert {(1, 4), (4, 4), (5, 12), (12, 12), (13, 12), (25, 12)} <= got
    assert any(x["r"] == 9 and x["s"] == 1366 for x in rc) and any(x["r"] == 5 and x["s"] == 1365 for x in rc)
    assert any(x["r"] == 5 and x["s"] == 4096 for x in rc)
    assert max(rows_combine_plan(x["r"], x["s"])[3] for x in rc) == 65536
    assert {1, 2, 3, 4, 5, 1023, 1024, 1025, 4099} <= {x["N"] for x in rc}
    assert {x.get("zscale", 1.0) for x in rc if x.get("z")} >= {0.0, 1.0, -0.5} and any(not x.get("z") for x in rc)
    assert any(len({x.get("ldy_extra", 0), x.get("ldz_extra", 0), x.get("ldo_extra", 0)}) == 3 and x.get("z") for x in rc)
    gn = d("gemm_nt")
    assert {1, 127, 128, 129, 257} <= {x["m"] for x in gn} | {x["n"] for x in gn}
    assert {1, 3, 4, 15, 16, 17, 1023, 16383, 16385, 1084586} <= {x["K"] for x in gn}
    assert {gemm_nt_plan(x["m"], x["n"], x["K"])[0] for x in gn} == {"gemm_nt/ks1", "gemm_nt/ks"}
    nn = d("gemm_nn_axpy")
    assert {4, 5, 6, 7, 15, 16, 17, 33, 450} <= {x["k"] for x in nn} and {4, 5, 127, 128, 129, 1300, 100003} <= {x["N"] for x in nn}
    assert {1, 127, 128, 129, 256} <= {x["m"] for x in nn} and {1, 7, 8, 9, 16, 17} <= {nn_blocks(x["m"], x["N"]) for x in nn}
    assert {x.get("v") for x in nn} == {None, "distinct", "out"}
    assert any(len({x.get("ldt_extra", 0), x.get("ldb_extra", 0), x.get("ldo_extra", 0), x.get("ldv_extra", 0)}) == 4 for x in nn)
    table = {c.route for c in CASES if c.route} | {"fill_normal", "fill_rademacher"}
    assert KRYLOV_ROUTES - table == VALU_ONLY
    totals = {t for t, _, _ in FILL_CASES}
    assert {1, 3, 4, 5, 1023, 1024, 1025, 32767, 32768, 32769} <= totals
    assert {o for _, o, _ in FILL_CASES} == {0, 1, 2, 3} and {s for _, _, s in FILL_CASES} >= {0, 1, 2 ** 32, 2 ** 64 - 1}
    want = {"mixed_alignment", "ldq_mod4", "ldq_lt_N", "unaligned_Q", "k_gt_kmax", "k_gt_8192", "lda_lt_K", "out_is_Y", "out_is_Z",
            "s_gt_4096", "k_lt_4", "out_is_B", "V_overlaps_out"}
    assert want <= {r[0].split("/")[1] for r in REFUSALS}
    assert {r[1] for r in REFUSALS if "mixed_alignment" in r[0]} == set(ROW_LAUNCH)


# ---------------------------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize("case", [c for c in CASES if c.exact], ids=[c.name for c in CASES if c.exact])
def test_exact_inputs_are_exact_in_any_order(case):
    call = kh.BUILDERS[case.prim](case.d, True, seed=1)
    kh.assert_exact_inputs(call)
    for name, r in call.arena.regs.items():          # position-dependent: no operand row is constant
        v = r.view(call.words)
        if r.dtype == "f32" and r.n >= 40 and name not in call.outs and torch.isfinite(v).all():
            assert (v.max(1).values > v.min(1).values).any(), f"{case.name}: operand {name} is constant along its rows"


def test_exactness_condition_refuses_large_inputs():
    call = kh.build_bdot(dict(P=1, N=2 ** 23), True, seed=1)
    call.arena.regs["X"].view(call.words).fill_(2.0)
    call.arena.regs["Y"].view(call.words).fill_(2.0)
    with pytest.raises(AssertionError, match="sum of absolute terms"):
        kh.assert_exact_inputs(call)


# ---------------------------------------------------------------------------------------------- the checks bite
def _perfect(name, exact):
    c = BY_NAME[name]
    call = kh.BUILDERS[c.prim](c.d, exact, seed=7)
    if c.prim == "scale_store" and not exact:
        call.outs["Q"].k = 2.0                       # a correctly rounded quotient (the GPU test has the measured bound)
    return call, kh.simulate(call)


@pytest.mark.parametrize("exact", [True, False])
def test_a_perfect_kernel_passes(exact):
    for name in ("bdot/N43/off1", "axpby/bp0_nan_row", "cg_update/active_mixed", "cg_direction/active_zero", "multi_dot/N2049",
                 "multi_axpy_norm/k257", "scale_store/inf", "dot_nt_f64/tile_atomic", "gemm_nt/K17", "gemm_nn_axpy/k7",
                 "rows_combine/r13"):
        call, w = _perfect(name, exact)
        kh.compare(call, w, w.clone(), name, det_override=True)


@pytest.mark.parametrize("name", ["bdot/blocks", "multi_dot/N4097", "dot_nt_f64/tile_part", "gemm_nt/K1023"])
def test_bites_one_element_dropped_from_a_sum(name):
    """exact inputs: the sum without one non-zero term; random inputs at N = 24581: the bound alone would not see it"""
    call, w = _perfect(name, True)
    oname, o = next(iter(call.outs.items()))
    a = call.arena.regs["X" if call.prim == "bdot" else ("Q" if call.prim == "multi_dot" else "A")].view(call.words).double()
    b = call.arena.regs["Y" if call.prim == "bdot" else ("w" if call.prim == "multi_dot" else "B")].view(call.words).double()
    prod = a[0] * b[0]
    i = int(torch.nonzero(prod)[-1])                 # the last non-zero term of output (0, 0)
    v = o.region.view(w)
    v[0, 0] = v[0, 0] - prod[i].to(v.dtype)
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        kh.compare(call, w, None, name)


def test_bites_one_element_shifted():
    call, w = _perfect("axpby/a_vec/b_vec", True)
    v = call.outs["Y"].region.view(w)
    row = v[1].clone()
    assert not torch.equal(row[1:], row[:-1])
    v[1, 1:] = row[:-1]
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        kh.compare(call, w, None)
    call, w = _perfect("rows_combine/r13", False)    # random inputs: far outside the bound
    v = call.outs["Out"].region.view(w)
    row = v[2].clone()
    v[2, 1:] = row[:-1]
    with pytest.raises(AssertionError, match="units of Mag"):
        kh.compare(call, w, None)


def test_bites_canary_overwritten_and_input_changed():
    call, w = _perfect("multi_axpy_norm/N2049", False)
    q = call.arena.regs["Q"]
    bad = w.clone()
    bad[q.base + c_pad(q)] = 0                       # one float of the ldq - N padding of the first basis row
    with pytest.raises(AssertionError, match="outside the outputs changed"):
        kh.compare(call, bad, None)
    bad = w.clone()
    bad[q.base + 5] ^= 1                             # one bit of an input
    with pytest.raises(AssertionError, match="outside the outputs changed"):
        kh.compare(call, bad, None)
    bad = w.clone()
    bad[call.arena.regs["w"].base - 1] = 0           # the guard word in front of an output
    with pytest.raises(AssertionError, match="outside the outputs changed"):
        kh.compare(call, bad, None)
    call, w = _perfect("cg_update/active_mixed", False)
    bad = w.clone()
    x = call.arena.regs["x"]
    bad[x.base + x.ld * 1 + 7] ^= 1                  # a row of an inactive probe
    with pytest.raises(AssertionError, match="outside the outputs changed"):
        kh.compare(call, bad, None)
    bad = w.clone()
    call.outs["x"].region.view(bad).view(torch.int32)[0, 3] = kh.CANARY      # an output element left unwritten
    with pytest.raises(AssertionError, match="not written"):
        kh.compare(call, bad, None)


def c_pad(q):
    assert q.ld > q.n
    return q.n


def test_bites_second_run_and_rms():
    call, w = _perfect("gemm_nn_axpy/k7", False)
    again = w.clone()
    call.outs["Out"].region.view(again).view(torch.int32)[0, 0] ^= 1
    with pytest.raises(AssertionError, match="second run"):
        kh.compare(call, w, again)
    call, w = _perfect("multi_dot/k257", False)      # every output at 60 % of its worst-case bound: only the RMS sees it
    ref, mag = call.reference(w)
    o = call.outs["c"]
    o.region.write(w, (ref["c"] + 0.6 * o.k * kh.U24 * mag["c"]).float())
    with pytest.raises(AssertionError, match="RMS"):
        kh.compare(call, w, None)


def test_bites_one_sign_flipped():
    total, seed = 32 * 256 * 4, 2 ** 32
    good = kh.ref_rademacher(total, seed)
    kh.compare_rademacher(good, total, seed)
    bad = good.copy()
    bad[20011] = -bad[20011]
    with pytest.raises(AssertionError, match="signs differ"):
        kh.compare_rademacher(bad, total, seed)
    # the mutation the issue names: shift (i & 7) instead of 4 (i & 7) reuses bits, the marginals stay perfect
    nq = total // 4
    u = np.stack(kh._lib_words(np.arange(256), seed))
    out = np.empty((32, 256, 4), dtype=np.float32)
    for i in range(32):
        bits = u[i >> 3] >> np.uint64(i & 7)
        for h in range(4):
            out[i, :, h] = np.where((bits >> np.uint64(h)) & np.uint64(1), 1.0, -1.0)
    assert nq == 32 * 256 and abs(out.mean()) < 0.02
    with pytest.raises(AssertionError, match="signs differ"):
        kh.compare_rademacher(out.reshape(-1), total, seed)
