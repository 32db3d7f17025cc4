"""Float64 yardstick of the Kronecker-factored posterior over all layers (CPU torch; no product code on its path).

The ``NetSpec`` forward is restated over ``net.units`` with a zero ``requires_grad`` tensor added to each raw
convolution output (before bias and BN); autograd with respect to those tensors gives dF_k / dz_{i,t}.  With at_{i,t}
the im2col patch in (kh, kw, ci) order (explicit padding and slicing; a leading 1 for a bias),

    A_l = sum_{i,t} at_{i,t} at_{i,t}^T,    S_l = sum_{i,t} G_{it} H_i G_{it}^T,    G_{it}[:, k] = dF_k / dz_{i,t},

H_i = diag(p_i) - p_i p_i^T (classifier) or I (regressor).  A layer block is [bias (N)] + kernel (M x N row-major) read
as an (Mt, N) matrix; its precision c_l kron(A_l, S_l) + diag(a) is built with ``torch.kron`` and inverted densely,
block by block (the covariance is block-diagonal).  The parameters outside every block get the exact GGN diagonal from
the autograd Jacobian of ``last_layer_ref.jac64``.
"""
import math

import torch
import torch.nn.functional as F

import aniso_nets
import last_layer_kron_ref as kref
import last_layer_ref as ref
from lip_amd.netspec import _get, act_fn
from lip_amd.toymodels import create_state
from lip_amd.utils import flatten_nn_params, param_layout

F64 = torch.float64
N_FULL = kref.N_FULL
NETS = kref.NETS + ["stem_net"]
DENSE_ONLY = ["sine_regressor", "xor_classifier", "mlp_ragged"]


def make_case(name):
    if name == "stem_net":
        g = torch.Generator().manual_seed(11)
        return create_state(aniso_nets.stem_net(), 3, dtype=F64, logvar=-0.3), torch.rand(3, 11, 8, 3, dtype=F64, generator=g), "classifier"
    return kref.make_case(name)


def blocks_of(state):
    """[(unit, offset, Mt, N, T, has bias)] per conv unit, restated from ``param_layout``"""
    net = state.net
    lay = {path: off for path, off, _ in param_layout(state.params)}
    out = []
    for u in net.units:
        if u.kind != "conv":
            continue
        oh, ow, _ = net.tensors[u.dst]
        M, N = u.kh * u.kw * u.cin, u.cout
        if u.bias is not None:
            assert lay[u.kernel] == lay[u.bias] + N
            out.append((u, lay[u.bias], M + 1, N, oh * ow, True))
        else:
            out.append((u, lay[u.kernel], M, N, oh * ow, False))
    return out


def _pad_hi(n_in, n_out, k, stride, lo):
    return max((n_out - 1) * stride + k - n_in - lo, 0)


def patches(a, u, oh, ow, bias):
    """(n, oh ow, Mt): the patch of ``a`` (n, h, w, c) at every output position, elements in (kh, kw, ci) order"""
    n, h, w, c = a.shape
    ap = F.pad(a, (0, 0, u.pad_w, _pad_hi(w, ow, u.kw, u.stride, u.pad_w), u.pad_h, _pad_hi(h, oh, u.kh, u.stride, u.pad_h)))
    cols = []
    for kh in range(u.kh):
        for kw in range(u.kw):
            cols.append(ap[:, kh:kh + (oh - 1) * u.stride + 1:u.stride, kw:kw + (ow - 1) * u.stride + 1:u.stride, :])
    P = torch.stack(cols, dim=3).reshape(n, oh * ow, u.kh * u.kw * c)
    if bias:
        P = torch.cat([torch.ones(n, oh * ow, 1, dtype=a.dtype), P], dim=2)
    return P


def forward_taps(state, X):
    """(out (n, K), [tap (n, oh, ow, N) per conv unit], [input (n, h, w, c) per conv unit]): the forward of
    ``NetSpec.forward`` restated, z = conv + tap with tap a zero leaf"""
    net, params, stats = state.net, state.params, state.batch_stats
    xb = net.prepare_input(X)
    vals = {0: xb}
    taps, inputs = [], []
    for u in net.units:
        a = vals[u.src]
        if u.kind == "view":
            vals[u.dst] = a.reshape((a.shape[0],) + net.tensors[u.dst])
            continue
        if u.kind == "meanpool":
            vals[u.dst] = a.mean(dim=(1, 2), keepdim=True)
            continue
        oh, ow, _ = net.tensors[u.dst]
        if u.kind in ("maxpool", "avgpool"):
            h, w = a.shape[1], a.shape[2]
            fill = float("-inf") if u.kind == "maxpool" else 0.0
            an = F.pad(a.permute(0, 3, 1, 2), (u.pad_w, _pad_hi(w, ow, u.kw, u.stride, u.pad_w), u.pad_h,
                                               _pad_hi(h, oh, u.kh, u.stride, u.pad_h)), value=fill)
            pool = F.max_pool2d if u.kind == "maxpool" else F.avg_pool2d
            vals[u.dst] = pool(an, (u.kh, u.kw), stride=u.stride).permute(0, 2, 3, 1)
            continue
        W = _get(params, u.kernel).reshape(u.kh * u.kw * u.cin, u.cout)
        P = patches(a, u, oh, ow, False)
        tap = torch.zeros(a.shape[0], oh, ow, u.cout, dtype=a.dtype, requires_grad=True)
        z = (P @ W).reshape(a.shape[0], oh, ow, u.cout) + tap
        taps.append(tap)
        inputs.append(a.detach())
        if u.bias is not None:
            z = z + _get(params, u.bias)
        if u.bn_scale is not None:
            mean, var = _get(stats, u.bn_mean), _get(stats, u.bn_var)
            z = (z - mean) * torch.rsqrt(var + u.bn_eps) * _get(params, u.bn_scale) + _get(params, u.bn_bias)
        if u.res is not None:
            z = z + vals[u.res]
        vals[u.dst] = act_fn(u.act, z)
    return vals[net.out].reshape(xb.shape[0], -1), taps, inputs


def patches_and_cotangents(state, X):
    """(f (n, K), [at (n, T, Mt)], [G (n, K, T, N)]) per block; example i's outputs depend on example i only"""
    out, taps, inputs = forward_taps(state, X)
    n, K = out.shape
    Gs = [torch.zeros(n, K, t.shape[1] * t.shape[2], t.shape[3], dtype=F64) for t in taps]
    for k in range(K):
        grads = torch.autograd.grad(out[:, k].sum(), taps, retain_graph=True, allow_unused=True)
        for G, g in zip(Gs, grads):
            if g is not None:
                G[:, k] = g.reshape(n, -1, g.shape[3])
    ats = [patches(a, u, state.net.tensors[u.dst][0], state.net.tensors[u.dst][1], b)
           for (u, _, _, _, _, b), a in zip(blocks_of(state), inputs)]
    return out.detach(), ats, Gs


def head_hessians(f, model_type):
    n, K = f.shape
    if model_type != "classifier":
        return torch.eye(K, dtype=F64).expand(n, K, K)
    p = torch.softmax(f, dim=-1)
    return torch.diag_embed(p) - p[:, :, None] * p[:, None, :]


def factors_from(f, ats, Gs, model_type):
    """([A_l (Mt, Mt)], [S_l (N, N)] uncentred, M) by einsum"""
    H = head_hessians(f, model_type)
    As = [torch.einsum("ite,itf->ef", at, at) for at in ats]
    Ss = [torch.einsum("iktn,ikm,imtp->np", G, H, G) for G in Gs]
    return As, Ss, f.shape[0]


def factors_ref(state, Z, model_type):
    return factors_from(*patches_and_cotangents(state, Z), model_type)


def is_final(state, u):
    return u is state.net.units[-1]


def head_factor(state, u, S, model_type):
    return kref.centre(S) if (model_type == "classifier" and is_final(state, u)) else S


def remainder_of(state):
    D = flatten_nn_params(state.params)[0].numel()
    keep = torch.ones(D, dtype=torch.bool)
    for _, off, Mt, N, _, _ in blocks_of(state):
        keep[off:off + Mt * N] = False
    return keep.nonzero().reshape(-1)


def ggn_diag_ref(state, Z, model_type, full_set_size=None):
    """(D,) exact GGN diagonal recal sum_i diag(J_i^T H_i J_i) from the autograd Jacobian"""
    f, J = ref.jac64(state, Z, model_type)
    H = head_hessians(f, model_type)
    return ref.recal(state, Z.shape[0], model_type, full_set_size) * torch.einsum("ikd,ikm,imd->d", J, H, J)


def alpha_for(state, As, Ss, M, model_type, full_set_size=None):
    """1e-3 max_l c_l lam_max(A_l) mu_max(S_l): the condition of every block's dense solve is at most 1002 with either
    prior of the tests"""
    recal = ref.recal(state, M, model_type, full_set_size)
    top = 0.0
    for (u, _, _, _, T, _), A, S in zip(blocks_of(state), As, Ss):
        S = head_factor(state, u, S, model_type)
        top = max(top, recal / (M * T) * float(torch.linalg.eigvalsh(A).max()) * float(torch.linalg.eigvalsh(S).max()))
    return 1e-3 * top


def split_prior(state, alpha):
    """two groups: the final kernel at 2 alpha, everything else at alpha (constant along every row of every block)"""
    return kref.split_prior(state, alpha)


def prior_vector(state, alpha, grouped):
    D = flatten_nn_params(state.params)[0].numel()
    return split_prior(state, alpha).vector("cpu", F64) if grouped else torch.full((D,), float(alpha), dtype=F64)


def covariance_blocks(state, As, Ss, M, model_type, a, full_set_size=None):
    """[(offset, S_l (Mt N, Mt N))] and the summed log det(diag(a)^-1 P_l): every block's dense precision
    c_l kron(A_l, S_l) + diag(a_l), solved densely; asserts that every solve is trustworthy"""
    recal = ref.recal(state, M, model_type, full_set_size)
    out, logdet = [], 0.0
    for (u, off, Mt, N, T, _), A, S in zip(blocks_of(state), As, Ss):
        al = a[off:off + Mt * N]
        P = recal / (M * T) * torch.kron(A, head_factor(state, u, S, model_type)) + torch.diag(al)
        P = 0.5 * (P + P.T)
        lam = torch.linalg.eigvalsh(P)
        assert float(lam.max() / lam.min()) <= 1002.0 * (1 + 1e-12)
        out.append((off, torch.linalg.solve(P, torch.eye(P.shape[0], dtype=F64))))
        d = al.rsqrt()
        logdet += float(torch.log(torch.linalg.eigvalsh(d[:, None] * P * d[None, :])).sum())
    return out, logdet


def variance_ref(state, cov_blocks, rem, rem_var):
    D = flatten_nn_params(state.params)[0].numel()
    v = torch.zeros(D, dtype=F64)
    for off, S in cov_blocks:
        v[off:off + S.shape[0]] = torch.diagonal(S)
    v[rem] = rem_var
    return v


def predict_dense(J, cov_blocks, rem, rem_var):
    """(B, K, K): J Sigma J^T for the block-diagonal Sigma; J (B, K, D)"""
    out = torch.einsum("bkd,d,bmd->bkm", J[:, :, rem], rem_var, J[:, :, rem])
    for off, S in cov_blocks:
        Jb = J[:, :, off:off + S.shape[0]]
        out = out + Jb @ S @ Jb.transpose(1, 2)
    return out


def spectrum_ref(state, As, Ss, M, model_type, diag1):
    """the evidence spectrum at N/M = 1: outer(lam_l, mu_l) / (M T_l) (x exp(-logvar) for the regressor) per block and
    the remainder's GGN diagonal ``diag1`` (built at N/M = 1)"""
    scale = math.exp(-float(state.params["logvar"]["logvar"])) if model_type == "regressor" else 1.0
    parts = []
    for (u, _, _, _, T, _), A, S in zip(blocks_of(state), As, Ss):
        lam = torch.linalg.eigvalsh(A).clamp_min(0.0)
        mu = torch.linalg.eigvalsh(head_factor(state, u, S, model_type)).clamp_min(0.0)
        parts.append(scale * torch.outer(lam, mu).reshape(-1) / (M * T))
    parts.append(diag1[remainder_of(state)].clamp_min(0.0))
    return torch.cat(parts)
