"""CPU: the float64 reference of MAP training and its anchors, ``NetSpec.forward(train=True)``, the train tapes of
``engine.compile_net`` executed by the float64 emulator against autograd, their structure, and the host optimizer."""
import hashlib
import json
import math
import os

import pytest
import torch

import train_map_ref as ref
from lip_amd import _native as nv
from lip_amd.engine import build_consts, compile_net
from train_map_cases import CASES, make_case
from train_map_parent_forward import parent_forward
from train_tape_emulator import TrainTapeMachine

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_IDS = [(name, n) for name, (_, _, ns, _) in CASES.items() for n in ns]


# ---- the reference's anchors: hand-computed ---------------------------------------------------------------------------------
def test_ref_batch_norm_three_values():
    # one channel, values 1, 2, 6: mean 3, biased variance (4 + 1 + 9) / 3 = 14 / 3
    y = torch.tensor([1.0, 2.0, 6.0], dtype=F64).reshape(3, 1, 1, 1)
    out, xhat, mean, var = ref.batch_norm_train(y, torch.tensor([2.0], dtype=F64), torch.tensor([0.5], dtype=F64), 0.0)
    assert mean.item() == 3.0 and abs(var.item() - 14.0 / 3.0) < 1e-15
    s = math.sqrt(14.0 / 3.0)
    want = torch.tensor([-2.0 / s, -1.0 / s, 3.0 / s], dtype=F64)
    assert torch.allclose(xhat.reshape(-1), want, rtol=0, atol=1e-15)
    assert torch.allclose(out.reshape(-1), 2.0 * want + 0.5, rtol=0, atol=1e-15)


def test_ref_running_statistics_take_the_biased_variance():
    from lip_amd.netspec import NetSpec
    net = NetSpec((1, 1, 1))
    net.conv(0, "Conv_0", 1, 1, 1, bn="BatchNorm_0")
    params = {"params": {"Conv_0": {"kernel": torch.ones(1, 1, 1, 1, dtype=F64)},
                         "BatchNorm_0": {"scale": torch.ones(1, dtype=F64), "bias": torch.zeros(1, dtype=F64)}}}
    stats = {"BatchNorm_0": {"mean": torch.tensor([10.0], dtype=F64), "var": torch.tensor([2.0], dtype=F64)}}
    x = torch.tensor([1.0, 2.0, 6.0], dtype=F64).reshape(3, 1, 1, 1)
    _, new = ref.forward_train(net, params, stats, x)
    assert abs(new["BatchNorm_0"]["mean"].item() - (0.99 * 10.0 + 0.01 * 3.0)) < 1e-14
    assert abs(new["BatchNorm_0"]["var"].item() - (0.99 * 2.0 + 0.01 * 14.0 / 3.0)) < 1e-14


def test_ref_losses():
    # two equal logits: log 2 whatever the label; logits (0, log 3), label 1: log(4 / 3)
    assert abs(ref.classifier_nll(torch.zeros(1, 2, dtype=F64), torch.tensor([0])).item() - math.log(2.0)) < 1e-15
    lg = torch.tensor([[0.0, math.log(3.0)]], dtype=F64)
    assert abs(ref.classifier_nll(lg, torch.tensor([1])).item() - math.log(4.0 / 3.0)) < 1e-15
    # f = 1, y = 0, logvar = 0: 0.5 (log 2 pi + 1); logvar = log 4: 0.5 (log 2 pi + log 4 + 1 / 4)
    f, y = torch.ones(1, 1, dtype=F64), torch.zeros(1, 1, dtype=F64)
    assert abs(ref.regressor_nll(f, y, torch.tensor(0.0, dtype=F64)).item() - 0.5 * (math.log(2 * math.pi) + 1.0)) < 1e-15
    lv = torch.tensor(math.log(4.0), dtype=F64)
    assert abs(ref.regressor_nll(f, y, lv).item() - 0.5 * (math.log(2 * math.pi) + math.log(4.0) + 0.25)) < 1e-15


def test_ref_adam_first_and_second_step():
    # t = 1: m_hat = g, v_hat = g^2, so the step is lr g / (|g| + eps) whatever the betas
    th, m, v = ref.adam_step(torch.tensor([1.0], dtype=F64), torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64),
                             torch.tensor([0.5], dtype=F64), 1, lr=0.1)
    assert abs(th.item() - (1.0 - 0.1 * 0.5 / (0.5 + 1e-8))) < 1e-15
    assert abs(m.item() - 0.05) < 1e-16 and abs(v.item() - 0.00025) < 1e-18
    # t = 2 with g = -0.5: m = 0.9 * 0.05 - 0.05 = -0.005, v = 0.999 * 0.00025 + 0.00025
    th2, m2, v2 = ref.adam_step(th, m, v, torch.tensor([-0.5], dtype=F64), 2, lr=0.1)
    mh, vh = -0.005 / (1 - 0.81), (0.999 * 0.00025 + 0.00025) / (1 - 0.999 ** 2)
    assert abs(th2.item() - (th.item() - 0.1 * mh / (math.sqrt(vh) + 1e-8))) < 1e-15


def test_ref_prior_vector_spares_the_regressor_biases():
    net, st, _, _, _ = make_case("sine_regressor", 6)
    a = ref.prior_vector(st.params, 0.7, "regressor")
    off = 0
    for path, leaf in ref.walk(ref.theta_tree(st.params)):
        want = 0.0 if path[-1] == "bias" else 0.7
        assert bool((a[off:off + leaf.numel()] == want).all())
        off += leaf.numel()
    assert off == a.numel() and bool((ref.prior_vector(st.params, 0.7, "classifier") == 0.7).all())


# ---- NetSpec.forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASE_IDS)
def test_forward_train_matches_the_reference(name, n):
    net, st, x, _, _ = make_case(name, n)
    out, new = net.forward(st.params, st.batch_stats, x, train=True)
    want, want_new = ref.forward_train(net, st.params, st.batch_stats, x)
    assert (out - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    assert sorted(p for p, _ in ref.walk(new)) == sorted(p for p, _ in ref.walk(want_new))
    for path, leaf in ref.walk(want_new):
        assert (ref.get(new, path) - leaf).abs().max().item() <= 1e-13 * max(1.0, leaf.abs().max().item())


@pytest.mark.parametrize("name,n", CASE_IDS)
def test_forward_eval_is_bitwise_unchanged(name, n):
    net, st, x, _, _ = make_case(name, n)
    want = parent_forward(net, st.params, st.batch_stats, x)
    assert torch.equal(net.forward(st.params, st.batch_stats, x), want)
    assert torch.equal(net.forward(st.params, st.batch_stats, x, train=False), want)
    assert torch.equal(net.forward(st.params, st.batch_stats, x[0]), parent_forward(net, st.params, st.batch_stats, x[0]))


def test_apply_fn_follows_flax_in_train_mode():
    net, st, x, _, _ = make_case("resnet_tiny", 3)
    variables = {"params": st.params["params"], "batch_stats": st.batch_stats}
    out, new_vars = st.apply_fn(variables, x, train=True, mutable=["batch_stats"])
    want, want_new = net.forward(st.params, st.batch_stats, x, train=True)
    assert torch.equal(out, want) and list(new_vars) == ["batch_stats"]
    for path, leaf in ref.walk(want_new):
        assert torch.equal(ref.get(new_vars["batch_stats"], path), leaf)
    assert torch.equal(st.apply_fn(variables, x, train=False, mutable=False), net.forward(st.params, st.batch_stats, x))


# ---- the train tapes, executed in float64 --------------------------------------------------------------------------------------
def _compiled(name, n):
    net, st, x, y, mt = make_case(name, n)
    net.model_type = mt
    return net, st, x, y, mt, compile_net(net, n, st.params, train=True)


@pytest.mark.parametrize("name,n", CASE_IDS)
def test_train_tapes_give_the_autograd_gradient(name, n):
    net, st, x, y, mt, cn = _compiled(name, n)
    consts = build_consts(cn, st.params, st.batch_stats, "cpu", F64)
    m = TrainTapeMachine(cn, ref.flatten(st.params), consts, x)
    m.train_primal()
    m.refresh()
    r = ref.loss_and_grad(net, st.params, st.batch_stats, x, y, mt, ref.prior_vector(st.params, 0.0, mt))
    f = m.logits()
    if mt == "classifier":
        U = (torch.softmax(f, -1) - torch.nn.functional.one_hot(y, cn.K).to(F64)) / n
    else:
        U = (f - y) * torch.exp(-st.params["logvar"]["logvar"]) / f.numel()
    g = m.train_backward(U)
    assert (f - r["out"]).abs().max().item() <= 1e-10 * max(1.0, r["out"].abs().max().item())
    for path, off, shape in [(p, o, s) for p, (o, s) in cn.offsets.items()]:
        k = int(torch.Size(shape).numel())
        want = r["grad"][off:off + k]
        assert (g[off:off + k] - want).abs().max().item() <= 1e-10 * max(want.abs().max().item(), r["grad"].abs().max().item() * 1e-3), path
    run = m.running_stats()
    assert sorted(run) == sorted(p for p, _ in ref.walk(r["stats"]))
    for path, got in run.items():
        want = ref.get(r["stats"], path)
        assert (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item()), path


# ---- structure ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASE_IDS)
def test_train_tape_structure(name, n):
    net, st, x, y, mt, cn = _compiled(name, n)
    bn_units = [u for u in net.units if u.kind == "conv" and u.bn_scale is not None]
    primal, backward = cn.train_tapes
    stats_at = [i for i, op in enumerate(primal) if op.kind == nv.OP_BN_STATS]
    assert len(stats_at) == len(bn_units)
    for i in stats_at:                                     # IGEMM -> BN_STATS -> PRIMAL_POST on the same z, the statistics in CONST
        assert primal[i - 1].kind == nv.OP_IGEMM and primal[i + 1].kind == nv.OP_PRIMAL_POST
        assert primal[i - 1].out.off == primal[i].seg[0].a.off == primal[i + 1].seg[0].a.off
        assert (primal[i].aux0.off, primal[i].aux1.off) == (primal[i + 1].aux0.off, primal[i + 1].aux1.off)
        assert all(r.space == nv.SP_CONST for r in (primal[i].aux0, primal[i].aux1, primal[i].scale, primal[i].out, primal[i].out2))
    assert [op.kind for op in primal if op.kind != nv.OP_BN_STATS] == [op.kind for op in cn.tapes[0] if op.kind != nv.OP_SOFTMAX]
    corr_at = [i for i, op in enumerate(backward) if op.kind == nv.OP_BN_TRAIN_BWD]
    assert len(corr_at) == len(bn_units)
    assert [op.kind for op in backward if op.kind != nv.OP_BN_TRAIN_BWD] == [op.kind for op in cn.tapes[2]]
    corrected = {}                                          # uncorrected cotangent offset -> corrected offset, while live
    for i, op in enumerate(backward):
        if op.kind == nv.OP_BN_TRAIN_BWD:
            g, gq = op.seg[0].a, op.out
            assert g.space == gq.space == nv.SP_WORK and g.off != gq.off          # a tensor of its own
            assert op.e0.space == op.e1.space == nv.SP_YOUT and op.xhat.space == nv.SP_PRIM
            nxt = backward[i + 1]                            # the unit's weight gradient reads the corrected cotangent
            assert nxt.kind == nv.OP_WGRAD and nxt.seg[0].b.off == gq.off and nxt.scale.space == nv.SP_CONST
            corrected[g.off] = gq.off
    # residual refs point at an uncorrected cotangent: never at the output of a BN_TRAIN_BWD
    outs = {op.out.off for op in backward if op.kind == nv.OP_BN_TRAIN_BWD}
    n_res = 0
    for op in backward:
        if op.kind == nv.OP_IGEMM and op.res.space != nv.SP_NONE:
            n_res += 1
            live = {o.out.off for o in backward[:backward.index(op)] if o.kind == nv.OP_BN_TRAIN_BWD}
            assert op.res.space == nv.SP_WORK and op.res.off not in live
    assert n_res == sum(1 for u in net.units if u.res is not None and any(p.dst == u.res and p.kind == "conv" and any(
        c.src == u.res and c.kind == "conv" for c in net.units) for p in net.units))
    assert outs or not bn_units


@pytest.mark.parametrize("name,n", CASE_IDS)
def test_existing_tapes_are_the_parents(name, n):
    """the three tapes, op by op, against the hashes recorded from ``compile_net`` before the train tapes existed"""
    want = json.load(open(os.path.join(GOLDEN, "train_map_parent_tapes.json")))[f"{name}/{n}"]
    for train in (False, True):
        net, st, x, y, mt = make_case(name, n)
        net.model_type = mt
        cn = compile_net(net, n, st.params, train=train)
        got = [[hashlib.sha256(bytes(op)).hexdigest()[:16] for op in tape] for tape in cn.tapes]
        assert got == want["tapes"] and cn.work_pp == want["work_pp"] and cn.prim_floats == want["prim_floats"]
    assert not compile_net(net, n, st.params).train_tapes


# ---- the host optimizer -----------------------------------------------------------------------------------------------------------
def test_adam_and_cosine_schedule_closed_forms():
    from lip_amd.train_map import Adam, cosine_decay_schedule
    sched = cosine_decay_schedule(0.2, 10, alpha=0.25)
    assert sched(0) == pytest.approx(0.2, abs=1e-16) and sched(10) == pytest.approx(0.05, abs=1e-16)
    assert sched(5) == pytest.approx(0.2 * (0.75 * 0.5 + 0.25), abs=1e-16) and sched(99) == sched(10)
    for k in range(12):
        assert sched(k) == pytest.approx(ref.cosine_decay(k, 0.2, 10, 0.25), abs=1e-16)
    opt = Adam(sched)
    assert (opt.b1, opt.b2, opt.eps) == (0.9, 0.999, 1e-8) and opt.lr_at(0) == sched(0) and Adam(0.3).lr_at(7) == 0.3
    # t = 1: the step is lr g / (|g| + eps); then two more steps against the float64 reference
    d, mu, nu = opt.scalar_update(0.5, 0, 0.0, 0.0)
    assert d == pytest.approx(-0.2 * 0.5 / (0.5 + 1e-8), abs=1e-16)
    th = torch.tensor([1.0], dtype=F64)
    m, v = torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64)
    x, mu, nu = 1.0, 0.0, 0.0
    for t, g in enumerate((0.5, -0.25, 2.0), start=1):
        th, m, v = ref.adam_step(th, m, v, torch.tensor([g], dtype=F64), t, lr=sched(t - 1))
        d, mu, nu = opt.scalar_update(g, t - 1, mu, nu)
        x += d
        assert x == pytest.approx(th.item(), abs=1e-15)


def test_src_alias_and_docstring():
    import src.train_alpha
    import src.train_map
    import lip_amd.train_map
    assert src.train_map is lip_amd.train_map
    assert "out of scope" not in src.train_alpha.__doc__ and callable(src.train_alpha.train_map_then_alpha)
