"""Nets on non-square inputs shared by the engine-level tests — TEST INFRASTRUCTURE (a plain helper module).

Flax SAME padding at stride 2 gives pad_h != pad_w when one side is even and the other odd (10 x 7 -> a 3 x 3 conv with
pad_h = 0, pad_w = 1); a Dense layer on a flattened non-square map compiles to a conv with KH != KW (LeNet5 on 16 x 20:
a 2 x 3 kernel).  The float64 tape emulator reproduces the oracle on all of them (tests/test_tape_compiler.py).
"""
import torch

from lip_amd.netspec import NetSpec
from lip_amd.scalemodels import LeNet5, ResNet1M, ResNet50

F64 = torch.float64


def stem_net(shape=(11, 8, 3), width=4, classes=3):
    """stride-2 conv + BN + ReLU, overlapping 3 x 3 / 2 max pool, conv, 2 x 2 average pool, Dense on the flattened
    (non-square) map"""
    net = NetSpec(tuple(shape))
    x = net.conv(0, "Conv_0", width, 3, 2, padding="SAME", bn="BatchNorm_0", act="relu")
    x = net.maxpool(x, 3, 2, padding=1)
    x = net.conv(x, "Conv_1", width, 3, 1, padding=1, bn="BatchNorm_1", act="relu")
    x = net.avgpool(x, 2, 2, padding="SAME")
    x = net.dense(x, "Dense_0", 6, act="relu")
    net.dense(x, "Dense_1", classes)
    net.model_type = "classifier"
    return net


def compiler_cases(g):
    """name -> (net, Z, model type, full set size): the five nets of tests/test_tape_compiler.py"""
    def Z(n, *shape):
        return torch.rand(n, *shape, dtype=F64, generator=g)
    return {
        "an_resnet_8x12": (ResNet1M(4, input_shape=(8, 12, 3), widths=(4, 8, 12), blocks_per_stage=2), Z(3, 8, 12, 3), "classifier", None),
        "an_resnet_10x7": (ResNet1M(4, input_shape=(10, 7, 3), widths=(4, 8, 12), blocks_per_stage=1), Z(3, 10, 7, 3), "classifier", 7),
        "an_resnet50_tiny_20x14": (ResNet50(6, input_shape=(20, 14, 3), stem=8, widths=(4, 8), blocks=(2, 1)), Z(2, 20, 14, 3), "classifier", 9),
        "an_lenet5_16x20": (LeNet5(5, input_shape=(16, 20, 1)), Z(2, 16, 20, 1), "classifier", 7),
        "an_stem_11x8": (stem_net(), Z(3, 11, 8, 3), "classifier", None),
    }


def engine_cases(g):
    """name -> (net, Z, model type, probes): sized to reach the MFMA and Winograd routes (widths 32 / 64: the 3 x 3
    layers of the first are Winograd-eligible on 16 x 24 and 8 x 12)"""
    def Z(n, *shape):
        return torch.rand(n, *shape, dtype=F64, generator=g)
    return {
        "an_resnet_16x24_wino": (ResNet1M(10, input_shape=(16, 24, 3), widths=(32, 64), blocks_per_stage=1), Z(3, 16, 24, 3), "classifier", 3),
        "an_resnet_10x7": (ResNet1M(5, input_shape=(10, 7, 3), widths=(16, 32), blocks_per_stage=1), Z(4, 10, 7, 3), "classifier", 2),
        "an_resnet50_tiny_20x14": (ResNet50(6, input_shape=(20, 14, 3), stem=8, widths=(4, 8), blocks=(2, 1)), Z(2, 20, 14, 3), "classifier", 2),
        "an_resnet50_small_24x40": (ResNet50(20, input_shape=(24, 40, 3), stem=16, widths=(16, 32), blocks=(1, 1)), Z(3, 24, 40, 3), "classifier", 2),
        "an_lenet5_16x20": (LeNet5(10, input_shape=(16, 20, 1)), Z(5, 16, 20, 1), "classifier", 3),
        "an_stem_11x8": (stem_net(width=16), Z(3, 11, 8, 3), "classifier", 2),
    }


def per_example_nets():
    """two nets on non-square inputs that between them reach every tile of the per-example square-sum / weighted-norm
    dispatchers, and their dense form, on a non-square geometry (M = 9 C_in, N = C_out; the tile follows M <= 64 and
    N <= 32 / <= 64 / > 64).  They keep the depth of the two square nets of tests/test_kernel_routes.py (five layers): the
    constant K_SQ presumes that a row element is off by at most 8 x 2^-24 max|r| of its tensor, and the rounding of a
    backward sweep grows with the layers it crosses, whatever the shape of the maps (a nine-layer net with 5- and
    6-channel stages measured 21 units on 10 x 7 and 23 on 10 x 10 inputs alike, its square sums equal to the squares of
    the engine's own rows).

    c: a 10 x 7 input through a stride-2 SAME stage (pad_h = 0, pad_w = 1) onto 5 x 4 maps, Dense on the flattened map
    d: a 6 x 10 map with few channels, Dense on the flattened 6 x 10 map"""
    c = NetSpec((10, 7, 3))
    x = c.conv(0, "Conv_0", 72, 3, 2, padding="SAME", act="relu", use_bias=True)     # M = 27, N = 72: <2,2,1,2>
    x = c.conv(x, "Conv_1", 40, 3, 1, padding=1, act="relu")                         # M = 648, N = 40: <4,1,1,2>
    x = c.conv(x, "Conv_2", 80, 3, 1, padding=1, act="relu")                         # M = 360, N = 80: <2,2,2,2>
    x = c.conv(x, "Conv_3", 20, 3, 1, padding=1, act="relu")                         # M = 720, N = 20: <4,1,1,1>
    c.dense(x, "Dense_0", 5)                                                         # a 5 x 4 kernel, one output pixel
    c.model_type = "classifier"
    d = NetSpec((6, 10, 6))
    x = d.conv(0, "Conv_0", 48, 3, 1, padding=1, act="relu", use_bias=True)          # M = 54, N = 48: <2,2,1,1>
    x = d.conv(x, "Conv_1", 4, 3, 1, padding=1, act="relu")                          # M = 432, N = 4: <4,1,1,1>
    x = d.conv(x, "Conv_2", 16, 3, 1, padding=1, act="relu")                         # M = 36, N = 16: <2,1,1,1>
    x = d.dense(x, "Dense_0", 40, act="relu")                                        # a 6 x 10 kernel
    d.dense(x, "Dense_1", 5)
    d.model_type = "classifier"
    return {"c": c, "d": d}
