"""The nets of the MAP-training tests — TEST INFRASTRUCTURE.  Each is the smallest shape that still takes a distinct
path of the train tapes (``engine.compile_net(..., train=True)``):

  mlp_ragged      Dense 7 -> 5 -> 3, tanh, no BN, K = 3; batches of 1 and 5
  sine_regressor  SimpleRegressor(8, 4) with logvar = -0.3; batch of 6
  lenet_tiny      conv 3x3 VALID + 2x2 avg pool + flat-kernel Dense on a 6 x 5 input: a non-square map, no BN
  resnet_tiny     6 x 5 x 3 input, ReLU, K = 4: stem conv3x3 + BN, a stride-1 block with an identity residual, a stride-2
                  block with a 1x1 projection + BN on the residual branch, mean pool, Dense; 5 and 12 channels
  bn_edge         one conv + BN layer (then mean pool and a Dense) whose R = n OH OW is 2, and the statistics kernel's
                  row chunk plus 1
"""
import torch

from lip_amd.netspec import NetSpec
from lip_amd.scalemodels import ResNet1M
from lip_amd.toymodels import SimpleRegressor, create_state

STATS_CHUNK = 256           # rows per partial of the batch-statistics kernel (csrc/lip_train.hip: TRAIN_STATS_ROWS)


def mlp_ragged() -> NetSpec:
    net = NetSpec((7,))
    t = net.dense(0, "Dense_0", 5, act="tanh")
    net.dense(t, "Dense_1", 3)
    net.model_type = "classifier"
    return net


def sine_regressor() -> NetSpec:
    return SimpleRegressor(8, 4)


def lenet_tiny() -> NetSpec:
    net = NetSpec((6, 5, 2))
    x = net.conv(0, "Conv_0", 3, 3, 1, padding="VALID", act="relu", use_bias=True)      # 4 x 3 x 3
    x = net.avgpool(x, 2, 2)                                                             # 2 x 1 x 3
    net.dense(x, "Dense_0", 3)
    net.model_type = "classifier"
    return net


def resnet_tiny() -> NetSpec:
    return ResNet1M(4, input_shape=(6, 5, 3), widths=(5, 12), blocks_per_stage=1)


def bn_edge(hw=(1, 1)) -> NetSpec:
    """R = n * hw[0] * hw[1] rows in the one BN layer"""
    net = NetSpec((hw[0], hw[1], 3))
    x = net.conv(0, "Conv_0", 5, 1, 1, bn="BatchNorm_0", act="relu")
    x = net.meanpool(x)
    net.dense(x, "Dense_0", 2)
    net.model_type = "classifier"
    return net


# name -> (net factory, model type, batch sizes, create_state keywords)
CASES = {
    "mlp_ragged": (mlp_ragged, "classifier", (1, 5), {}),
    "sine_regressor": (sine_regressor, "regressor", (6,), dict(logvar=-0.3)),
    "lenet_tiny": (lenet_tiny, "classifier", (4,), {}),
    "resnet_tiny": (resnet_tiny, "classifier", (3, 7), {}),
    "bn_edge_2": (lambda: bn_edge((1, 1)), "classifier", (2,), {}),
    "bn_edge_chunk": (lambda: bn_edge((STATS_CHUNK + 1, 1)), "classifier", (1,), {}),      # R = STATS_CHUNK + 1
}


def make_case(name: str, n: int, seed: int = 0, dtype=torch.float64):
    """``(net, state, x (n, ...), y, model_type)``: seeded float64 state and batch of a case"""
    factory, model_type, _, kw = CASES[name]
    net = factory()
    state = create_state(net, seed=11 + seed, dtype=dtype, **kw)
    g = torch.Generator().manual_seed(1000 * (seed + 1) + n)
    x = torch.randn((n,) + tuple(net.input_shape_raw), generator=g, dtype=torch.float64).to(dtype)
    if model_type == "classifier":
        y = torch.randint(0, net.num_outputs, (n,), generator=g)
    else:
        y = torch.randn(n, net.num_outputs, generator=g, dtype=torch.float64).to(dtype)
    return net, state, x, y, model_type
