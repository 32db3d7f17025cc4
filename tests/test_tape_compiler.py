"""CPU: the NetSpec -> op-tape compiler + the op semantics of include/lip.h reproduce the oracle
(float64, 1e-12) for every model family, including BN / residual / stride-2 projection / mean-pool."""
import math

import pytest
import torch

from lip_amd import _native as nv
from lip_amd.engine import build_consts, compile_net
from lip_amd.scalemodels import LargeClassifier, LeNet5, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state
from lip_amd.utils import flatten_nn_params
from oracle.ggn import compute_ggn_vp, compute_W_vps
from tape_emulator import TapeMachine

F64 = torch.float64
G = torch.Generator().manual_seed(0)
CASES = {
    "regressor": (SimpleRegressor(8, 4), torch.randn(5, 1, dtype=F64, generator=G), "regressor", 20),
    "classifier": (SimpleClassifier(16, 2, 2), torch.randn(6, 2, dtype=F64, generator=G), "classifier", None),
    "large": (LargeClassifier((6, 6, 1), [24, 16], 2, 5), torch.rand(4, 6, 6, 1, dtype=F64, generator=G), "classifier", 11),
    "resnet": (ResNet1M(4, input_shape=(8, 8, 3), widths=(4, 8, 12), blocks_per_stage=2),
               torch.rand(3, 8, 8, 3, dtype=F64, generator=G), "classifier", None),
    "resnet50_tiny": (ResNet50(6, input_shape=(20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
                      torch.rand(2, 20, 20, 3, dtype=F64, generator=G), "classifier", 9),
    "lenet5_small": (LeNet5(5, input_shape=(16, 16, 1)), torch.rand(2, 16, 16, 1, dtype=F64, generator=G), "classifier", 7),
    "resnet_gray": (ResNet1M(3, input_shape=(8, 8, 1), widths=(4, 8), blocks_per_stage=1),
                    torch.rand(3, 8, 8, 1, dtype=F64, generator=G), "classifier", None),
}
# non-square inputs: per-axis SAME padding (pad_h != pad_w at stride 2 on 10 x 7 and 11 x 8) and the flat kernels of a
# Dense layer on a non-square map (KH != KW)
from aniso_nets import compiler_cases  # noqa: E402
CASES.update(compiler_cases(G))


@pytest.mark.parametrize("name", list(CASES))
def test_tapes_reproduce_oracle(name):
    net, Z, model_type, full = CASES[name]
    st = create_state(net, 3, dtype=F64, logvar=-0.3)
    n, P = Z.shape[0], 2
    cn = compile_net(net, n, st.params)
    flat, _ = flatten_nn_params(st.params)
    tm = TapeMachine(cn, flat, build_consts(cn, st.params, st.batch_stats, "cpu", F64), Z, chunk=P)
    tm.primal()
    f_or = st.apply_fn({"params": st.params["params"]}, Z, return_logvar=False)
    o = cn.a_off[net.out]
    assert torch.allclose(tm.prim[o:o + n * cn.K].reshape(n, cn.K), f_or, atol=1e-12)
    V = torch.randn(P, cn.D, dtype=F64, generator=torch.Generator().manual_seed(1))
    N = full or n
    lv = st.params["logvar"]["logvar"].item() if model_type == "regressor" else 0.0
    Y = tm.ggn_vp(V, N / n * math.exp(-lv), 0.37)
    vp = compute_ggn_vp(st, Z, model_type, full_set_size=full)
    Yo = torch.stack([vp(v) + 0.37 * v for v in V])
    assert (Y - Yo).abs().max() <= 1e-11 * Yo.abs().max(), (Y - Yo).abs().max()
    Wf, WTf = compute_W_vps(st, Z, model_type, full_set_size=full)
    c = math.sqrt(N / n) * math.exp(-0.5 * lv)
    U = tm.jvp(V, nv.HEAD_LT, c)
    Uo = torch.stack([WTf(v).reshape(n, -1) for v in V])
    assert (U - Uo).abs().max() <= 1e-11 * Uo.abs().max().clamp_min(1.0)
    Ur = torch.randn(P, n, cn.K, dtype=F64, generator=torch.Generator().manual_seed(2))
    Yw = tm.vjp(Ur, nv.HEAD_L, c)
    Ywo = torch.stack([Wf(u if model_type == "classifier" else u.reshape(n)) for u in Ur])
    assert (Yw - Ywo).abs().max() <= 1e-11 * Ywo.abs().max()


def test_resnet1m_layout_matches_survey():
    """D and MACs/example of the headline workload (1 084 586 and 162 366 720)."""
    net = ResNet1M(10)
    st = create_state(net, 0)
    flat, _ = flatten_nn_params(st.params)
    assert flat.numel() == 1_084_586 and net.macs_per_example() == 162_366_720
    cn = compile_net(net, 50, st.params)
    assert cn.D == 1_084_586 and cn.K == 10
    # the tapes' FLOP count is the 8 * MACs model of SURVEY §8d minus the input layer's two absent terms
    from lip_amd.engine import tape_flops_per_probe
    fl = sum(tape_flops_per_probe(cn).values())
    first = 32 * 32 * 27 * 32
    assert fl == 50 * (8 * 162_366_720 - 4 * first)
    # executed matrix-pipe FLOPs with the Winograd route on (bench.py's roofline.executed): the 3x3 / stride-1 / pad-1
    # layers with 32 | C and 32 | N — 18 of the net's 3x3 convolutions: 6 per stage (stage 1: both convs of its three
    # blocks; stages 2, 3: all but the stride-2 first conv, i.e. 5) ... counted from the net itself — at 4/9, the rest as is
    from lip_amd.engine import tape_executed_flops_per_probe
    ex = sum(tape_executed_flops_per_probe(cn).values())
    macs_wino = 0
    for u in net.units:
        if u.kind == "conv" and u.kh == 3 and u.kw == 3 and u.stride == 1 and u.cin % 32 == 0 and u.cout % 32 == 0:
            oh, ow, _ = net.tensors[u.dst]
            macs_wino += oh * ow * 9 * u.cin * u.cout
    assert macs_wino > 0.9 * (162_366_720 - 2 * first)          # ~95 % of the forward MACs
    # every eligible layer contributes 8 MACs-worth of algorithmic FLOPs (4 tangent + 2 data gradient + 2 weight
    # gradient), all of them on the route
    assert ex == fl - 50 * (8 * macs_wino - (8 * macs_wino) * 4 // 9) or abs(ex - (fl - 50 * 8 * macs_wino * 5 / 9)) <= 64
    assert 0.45 < ex / fl < 0.50


def test_resnet50_parameter_count():
    """BASELINE configs[4]: the locally defined ResNet-50 has torchvision's parameter count (25 557 032 trainable
    incl. BN affine parameters; running statistics are not part of theta)."""
    net = ResNet50(1000)
    st = create_state(net, 0)
    flat, _ = flatten_nn_params(st.params)
    assert flat.numel() == 25_557_032


def test_lenet5_parameter_count():
    """src/scalemodels.py:12 "~60 k parameters": 156 + 2416 + 48120 + 10164 + 850."""
    net = LeNet5()
    st = create_state(net, 0)
    assert flatten_nn_params(st.params)[0].numel() == 61706
    assert st.params["params"]["Dense_0"]["kernel"].shape == (400, 120)
    assert st.apply_fn({"params": st.params["params"]}, torch.rand(3, 28, 28, 1)).shape == (3, 10)
