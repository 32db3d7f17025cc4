"""Float64 reference of MAP training — TEST INFRASTRUCTURE, plain torch on the CPU.

Three parts, none of which calls the code under test (``NetSpec.forward``, the engine, ``train_map``):

  * ``forward_train``: the train-mode forward of a NetSpec layer program written out from the unit fields alone:
    convolutions as sums of shifted slices, Flax ``BatchNorm`` defaults in train mode (batch mean, BIASED batch variance,
    running = 0.99 running + 0.01 batch for both, the biased variance included), residuals before the activation, pools;
  * the two losses of the reference's ``_map_step`` (``src/train_map.py:52-88``) with ``torch.autograd`` gradients:
    mean softmax cross-entropy, and 0.5 mean(log(2 pi var) + (f - y)^2 / var); plus 0.5 sum a theta^2;
  * the optax ``adam`` update (``eps_root = 0``), dtype-generic, so that the same trajectory runs in float32 and float64.

Pinned by the hand-computed anchors of ``tests/test_train_map_cpu.py``.
"""
import math

import torch

F64 = torch.float64
MOMENTUM = 0.99
_GELU_C = math.sqrt(2.0 / math.pi)


# ---- parameter trees -----------------------------------------------------------------------------------------------------
def walk(tree, prefix=()):
    """(path, leaf) in sorted-key order: the order of the flat parameter vector"""
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from walk(tree[k], prefix + (k,))
    else:
        yield prefix, tree


def theta_tree(params):
    return {k: v for k, v in params.items() if k not in ("logvar", "batch_stats")}


def flatten(params, dtype=F64):
    return torch.cat([torch.as_tensor(leaf).detach().to(dtype).reshape(-1) for _, leaf in walk(theta_tree(params))])


def unflatten(params, flat):
    """the tree of ``params`` (without logvar) with its leaves taken from ``flat`` (views: differentiable)"""
    out, off = {}, 0
    for path, leaf in walk(theta_tree(params)):
        n = torch.as_tensor(leaf).numel()
        t = out
        for k in path[:-1]:
            t = t.setdefault(k, {})
        t[path[-1]] = flat[off:off + n].reshape(tuple(torch.as_tensor(leaf).shape))
        off += n
    return out


def get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def put(tree, path, value):
    for k in path[:-1]:
        tree = tree.setdefault(k, {})
    tree[path[-1]] = value


def prior_vector(params, alpha, model_type, dtype=F64):
    """(D,) precisions of the reference's ``_nl_prior``: ``alpha`` everywhere for the classifier; for the regressor 0 on
    every leaf named ``bias`` (``bias_precision = 0``, ``src/train_map.py:20-30,76``)"""
    parts = []
    for path, leaf in walk(theta_tree(params)):
        n = torch.as_tensor(leaf).numel()
        zero = model_type == "regressor" and path[-1] == "bias"
        parts.append(torch.full((n,), 0.0 if zero else float(alpha), dtype=dtype))
    return torch.cat(parts)


# ---- train-mode forward --------------------------------------------------------------------------------------------------
def _act(name, y):
    if name == "none":
        return y
    if name == "relu":
        return torch.clamp_min(y, 0.0)
    if name == "tanh":
        return torch.tanh(y)
    if name == "gelu":
        return 0.5 * y * (1.0 + torch.tanh(_GELU_C * (y + 0.044715 * y ** 3)))
    raise ValueError(name)


def _windows(a, kh, kw, stride, pad_h, pad_w, oh, ow, fill):
    """yield (i, j, the (n, oh, ow, c) slice of tap (i, j)) of ``a`` (n, h, w, c) padded with ``fill``"""
    n, h, w, c = a.shape
    hi_h = max((oh - 1) * stride + kh - h - pad_h, 0)
    hi_w = max((ow - 1) * stride + kw - w - pad_w, 0)
    ap = torch.full((n, h + pad_h + hi_h, w + pad_w + hi_w, c), fill, dtype=a.dtype)
    ap[:, pad_h:pad_h + h, pad_w:pad_w + w, :] = a
    for i in range(kh):
        for j in range(kw):
            yield i, j, ap[:, i:i + stride * (oh - 1) + 1:stride, j:j + stride * (ow - 1) + 1:stride, :]


def batch_norm_train(y, gamma, beta, eps):
    """Flax BatchNorm(use_running_average=False) over all axes but the last: (out, xhat, mean, biased var)"""
    flat = y.reshape(-1, y.shape[-1])
    mean = flat.sum(0) / flat.shape[0]
    var = ((flat - mean) ** 2).sum(0) / flat.shape[0]
    xhat = (y - mean) / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat, mean, var


def forward_train(net, params, batch_stats, x, momentum=MOMENTUM):
    """``(out (n, K), new_batch_stats)`` of the layer program ``net`` in train mode; differentiable in ``params``"""
    h0, w0, c0 = net.tensors[0]
    t = net.tile_channels
    xb = x.reshape(-1, h0, w0, c0 // t)
    if t > 1:
        xb = torch.cat([xb] * t, dim=-1)
    vals = {0: xb}
    new_stats = {}
    for u in net.units:
        a = vals[u.src]
        oh, ow, oc = net.tensors[u.dst]
        if u.kind == "view":
            vals[u.dst] = a.reshape(a.shape[0], oh, ow, oc)
        elif u.kind == "meanpool":
            vals[u.dst] = a.sum((1, 2), keepdim=True) / (a.shape[1] * a.shape[2])
        elif u.kind == "maxpool":
            out = None
            for _, _, win in _windows(a, u.kh, u.kw, u.stride, u.pad_h, u.pad_w, oh, ow, float("-inf")):
                out = win if out is None else torch.maximum(out, win)
            vals[u.dst] = out
        elif u.kind == "avgpool":
            out = 0.0
            for _, _, win in _windows(a, u.kh, u.kw, u.stride, u.pad_h, u.pad_w, oh, ow, 0.0):
                out = out + win
            vals[u.dst] = out / (u.kh * u.kw)
        else:
            W = get(params, u.kernel).reshape(u.kh, u.kw, u.cin, u.cout)      # HWIO; a Dense kernel is the 1x1 / flat case
            z = 0.0
            for i, j, win in _windows(a, u.kh, u.kw, u.stride, u.pad_h, u.pad_w, oh, ow, 0.0):
                z = z + win @ W[i, j]
            if u.bias is not None:
                z = z + get(params, u.bias)
            if u.bn_scale is not None:
                z, _, mean, var = batch_norm_train(z, get(params, u.bn_scale), get(params, u.bn_bias), u.bn_eps)
                put(new_stats, u.bn_mean, (momentum * get(batch_stats, u.bn_mean) + (1 - momentum) * mean).detach())
                put(new_stats, u.bn_var, (momentum * get(batch_stats, u.bn_var) + (1 - momentum) * var).detach())
            if u.res is not None:
                z = z + vals[u.res]
            vals[u.dst] = _act(u.act, z)
    return vals[net.out].reshape(xb.shape[0], -1), new_stats


# ---- losses --------------------------------------------------------------------------------------------------------------
def classifier_nll(logits, y):
    """mean softmax cross-entropy (``optax.softmax_cross_entropy`` then ``jnp.mean``)"""
    lse = torch.logsumexp(logits, dim=-1)
    return (lse - logits.gather(1, y.reshape(-1, 1).long())[:, 0]).sum() / logits.shape[0]


def regressor_nll(f, y, logvar):
    """0.5 mean(log(2 pi var) + (f - y)^2 / var), var = exp(logvar)"""
    return 0.5 * (math.log(2 * math.pi) + logvar + (f - y.reshape(f.shape)) ** 2 * torch.exp(-logvar)).sum() / f.numel()


def loss_and_grad(net, params, batch_stats, x, y, model_type, a_vec, dtype=F64):
    """``dict(loss, nll, grad (D,), dlogvar, stats, out)`` of the train-mode MAP loss nll + 0.5 sum a theta^2 at the
    parameters ``params`` (any dtype; computed in ``dtype``)"""
    theta = flatten(params, dtype).requires_grad_(True)
    tree = unflatten(params, theta)
    stats = {}
    for path, leaf in walk(batch_stats):
        put(stats, path, torch.as_tensor(leaf).detach().to(dtype))
    out, new_stats = forward_train(net, tree, stats, x.to(dtype))
    logvar = None
    if model_type == "regressor":
        logvar = torch.as_tensor(params["logvar"]["logvar"]).detach().to(dtype).clone().requires_grad_(True)
        nll = regressor_nll(out, y.to(dtype), logvar)
    else:
        nll = classifier_nll(out, y)
    loss = nll + 0.5 * (a_vec.to(dtype) * theta ** 2).sum()
    grads = torch.autograd.grad(loss, [theta] + ([logvar] if logvar is not None else []))
    return dict(loss=loss.detach(), nll=nll.detach(), grad=grads[0], dlogvar=grads[1] if logvar is not None else None,
                stats=new_stats, out=out.detach())


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def adam_step(theta, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """optax.adam at step t >= 1 (``scale_by_adam`` with ``eps_root = 0``, then ``-lr``): ``(theta, m, v)``, in the dtype
    of the inputs"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mhat = m / (1 - b1 ** t)
    vhat = v / (1 - b2 ** t)
    return theta - lr * mhat / (torch.sqrt(vhat) + eps), m, v


def cosine_decay(step, init_value, decay_steps, alpha=0.0):
    """optax.cosine_decay_schedule (exponent 1): init (( 1 - alpha) 0.5 (1 + cos(pi min(step, T) / T)) + alpha)"""
    c = min(step, decay_steps) / decay_steps
    return init_value * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * c)) + alpha)


def train_full_batch(net, state, x, y, model_type, alpha, steps, lr, dtype):
    """``steps`` full-batch Adam steps on (x, y) from ``state`` in ``dtype``: the list of the losses each step reports
    (the loss at the parameters BEFORE its update), and the final (flat theta, logvar)"""
    params = {k: v for k, v in state.params.items()}
    theta = flatten(params, dtype)
    a = prior_vector(params, alpha, model_type, dtype)
    stats = {}
    for path, leaf in walk(state.batch_stats):
        put(stats, path, torch.as_tensor(leaf).detach().to(dtype))
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    lv = ml = vl = None
    if model_type == "regressor":
        lv = torch.as_tensor(params["logvar"]["logvar"]).detach().to(dtype).clone()
        ml, vl = torch.zeros_like(lv), torch.zeros_like(lv)
    losses = []
    for t in range(1, steps + 1):
        cur = unflatten(params, theta)
        if lv is not None:
            cur["logvar"] = {"logvar": lv}
        r = loss_and_grad(net, cur, stats, x, y, model_type, a, dtype)
        losses.append(float(r["loss"]))
        stats = r["stats"] if r["stats"] else stats
        theta, m, v = adam_step(theta, m, v, r["grad"].detach(), t, lr)
        if lv is not None:
            lv, ml, vl = adam_step(lv, ml, vl, r["dlogvar"].detach(), t, lr)
    return losses, theta, lv
