"""Float64 yardstick of the Kronecker-factored last-layer posterior (CPU torch; no product code on its path).

The features come from ``last_layer_ref.features64``.  With phit_i = [1, phi_i] and the flat index f K + k of theta_L,

    A = sum_i phit_i phit_i^T,   Bf = sum_i diag(p_i) - p_i p_i^T  (classifier)  or  M I  (regressor),
    precision = c kron(A, Bf) + diag(a_f (x) 1_K),   c = recal / M,

built with ``torch.kron`` and inverted densely (the classifier's Bf is centred, C Bf C with C = I - 1 1^T / K, as the
package does).  ``tests/test_last_layer_kron_cpu.py`` pins the package's factored algebra against this dense route;
``factored`` restates the factored route so that the GPU tests have a yardstick where DL is too large for a dense one.
"""
import torch

import last_layer_ref as ref
from lip_amd.netspec import NetSpec
from lip_amd.prior import GroupedPrior
from lip_amd.scalemodels import LargeClassifier, ResNet1M, ResNet50
from lip_amd.toymodels import SimpleClassifier, SimpleRegressor, create_state

F64 = torch.float64
N_FULL = 40


def flat_head_net():
    """a final Dense directly on a 3 x 3 x 4 feature map (the ``flat_kernel`` path)"""
    net = NetSpec((3, 3, 2))
    c = net.conv(0, "Conv_0", 4, 3, act="relu", use_bias=True)
    net.dense(c, "Dense_0", 3)
    return net


def cases():
    """the nets, inputs and seeds of tests/test_last_layer.py::_cases"""
    g = torch.Generator().manual_seed(0)
    return {
        "sine_regressor": (SimpleRegressor(8, 4), torch.randn(16, 1, dtype=F64, generator=g), "regressor"),
        "xor_classifier": (SimpleClassifier(16, 2, 2), torch.randn(32, 2, dtype=F64, generator=g), "classifier"),
        "mlp_ragged": (LargeClassifier((6, 6, 1), [40, 24], 2, 5), torch.rand(9, 6, 6, 1, dtype=F64, generator=g),
                       "classifier"),
        "resnet_tiny": (ResNet1M(4, input_shape=(8, 8, 3), widths=(4, 8, 12), blocks_per_stage=2),
                        torch.rand(3, 8, 8, 3, dtype=F64, generator=g), "classifier"),
        "resnet50_tiny": (ResNet50(6, input_shape=(20, 20, 3), stem=8, widths=(4, 8), blocks=(2, 1)),
                          torch.rand(2, 20, 20, 3, dtype=F64, generator=g), "classifier"),
        "flat_head": (flat_head_net(), torch.rand(7, 3, 3, 2, dtype=F64, generator=g), "classifier"),
    }


NETS = list(cases())
SMALL = ["sine_regressor", "xor_classifier", "mlp_ragged", "flat_head"]


def make_case(name):
    net, Z, model_type = cases()[name]
    return create_state(net, 3, dtype=F64, logvar=-0.3), Z, model_type


def split_prior(state, alpha):
    """two groups cutting theta_L between the final bias and the final kernel: a_0 = alpha, a_f = 2 alpha for f >= 1"""
    kernel = state.net.units[-1].kernel
    return GroupedPrior(state.params, [alpha, 2.0 * alpha], lambda path: "head_kernel" if path == kernel else "rest")


def new_points(Z, B, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B,) + tuple(Z.shape[1:])
    return torch.randn(shape, dtype=F64, generator=g) if Z.dim() == 2 else torch.rand(shape, dtype=F64, generator=g)


def factors_ref(state, Z, model_type):
    """(A (Ft, Ft), Bf (K, K) uncentred, M) by einsum"""
    f, phit, p = ref.features64(state, Z)
    M, K = f.shape
    A = torch.einsum("if,ig->fg", phit, phit)
    if model_type == "classifier":
        Bf = (torch.diag_embed(p) - p[:, :, None] * p[:, None, :]).sum(0)
    else:
        Bf = M * torch.eye(K, dtype=phit.dtype)
    return A, Bf, M


def centre(Bf):
    K = Bf.shape[0]
    C = torch.eye(K, dtype=Bf.dtype) - torch.full((K, K), 1.0 / K, dtype=Bf.dtype)
    return C @ Bf @ C


def head_factor(Bf, model_type):
    return centre(Bf) if model_type == "classifier" else Bf


def c_of(state, M, model_type, full_set_size=None):
    return ref.recal(state, M, model_type, full_set_size) / M


def alpha_for(A, Bf, c):
    """1e-3 c lam_max(A) mu_max(Bf): condition <= 1002 with either prior of the tests"""
    return 1e-3 * c * float(torch.linalg.eigvalsh(A).max()) * float(torch.linalg.eigvalsh(Bf).max())


def precision_dense(A, Bf, c, a_rows, model_type):
    K = Bf.shape[0]
    a = torch.as_tensor(a_rows, dtype=F64).expand(A.shape[0]).repeat_interleave(K)
    return c * torch.kron(A, head_factor(Bf, model_type)) + torch.diag(a), a


def covariance_dense(A, Bf, c, a_rows, model_type):
    """(S (DL, DL), log det(diag(a)^-1 P)) through a dense solve; asserts that the solve is trustworthy"""
    P, a = precision_dense(A, Bf, c, a_rows, model_type)
    P = 0.5 * (P + P.T)
    lam = torch.linalg.eigvalsh(P)
    assert float(lam.max() / lam.min()) <= 1002.0 * (1 + 1e-12)
    S = torch.linalg.solve(P, torch.eye(P.shape[0], dtype=F64))
    d = a.rsqrt()
    logdet = torch.log(torch.linalg.eigvalsh(d[:, None] * P * d[None, :])).sum()
    return S, float(logdet)


def predict_dense(phit, S, K):
    Ft = phit.shape[1]
    return torch.einsum("bf,bg,fkgl->bkl", phit, phit, S.reshape(Ft, K, Ft, K))


def factored(A, Bf, c, a_rows, model_type):
    """(V, R, Ub, lam, mu) of the factored posterior, restated: d = a^(-1/2), d A d = Ut lam Ut^T, Bf = Ub mu Ub^T,
    V = d Ut, R = 1 / (c lam mu^T + 1)"""
    d = torch.as_tensor(a_rows, dtype=F64).expand(A.shape[0]).rsqrt()
    At = torch.diag(d) @ A @ torch.diag(d)
    lam, Ut = torch.linalg.eigh(0.5 * (At + At.T))
    Bc = head_factor(Bf, model_type)
    mu, Ub = torch.linalg.eigh(0.5 * (Bc + Bc.T))
    lam, mu = lam.clamp_min(0.0), mu.clamp_min(0.0)
    return torch.diag(d) @ Ut, 1.0 / (c * torch.outer(lam, mu) + 1.0), Ub, lam, mu


def predict_factored(phit, V, R, Ub):
    """(B, K, K): Ub diag(s_b) Ub^T with s_b = ((V^T phit_b)^2) R"""
    s = (phit @ V) ** 2 @ R
    return torch.einsum("kl,bl,ml->bkm", Ub, s, Ub)
