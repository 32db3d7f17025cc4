"""``NetSpec.forward`` as it stood before train mode was added, verbatim — TEST INFRASTRUCTURE.

``tests/test_train_map_cpu.py`` runs it next to the current ``NetSpec.forward(..., train=False)`` on the same inputs and
asks for bitwise equal outputs: the same torch calls in the same order on the same machine.  ``self`` is the NetSpec.
"""
from typing import Any, Dict

import torch
import torch.nn.functional as F

from lip_amd.netspec import _get, act_fn


def parent_forward(self, params: Dict[str, Any], batch_stats: Dict[str, Any], x: torch.Tensor,
            return_all: bool = False):
    """Torch functional forward, any dtype/device, differentiable in ``params``.

    ``x`` is one example (``input_shape``) or a batch ``(B, *input_shape)``;
    returns ``(K,)`` or ``(B, K)``.  ``params`` is the tree containing
    ``param_root`` (e.g. ``{'params': {...}}``).
    """
    raw = self.input_shape_raw
    if tuple(x.shape) == raw:
        single = True
        xb = self.prepare_input(x[None])
    else:
        single = False
        xb = self.prepare_input(x)
    vals: Dict[int, torch.Tensor] = {0: xb}
    for u in self.units:
        a = vals[u.src]
        if u.kind == "view":
            vals[u.dst] = a.reshape((a.shape[0],) + self.tensors[u.dst])
            continue
        if u.kind == "meanpool":
            vals[u.dst] = a.mean(dim=(1, 2), keepdim=True)
            continue
        if u.kind == "maxpool":
            oh, ow, _ = self.tensors[u.dst]
            h, w = a.shape[1], a.shape[2]
            hi_h = max((oh - 1) * u.stride + u.kh - h - u.pad_h, 0)
            hi_w = max((ow - 1) * u.stride + u.kw - w - u.pad_w, 0)
            an = F.pad(a.permute(0, 3, 1, 2), (u.pad_w, hi_w, u.pad_h, hi_h), value=float("-inf"))
            vals[u.dst] = F.max_pool2d(an, (u.kh, u.kw), stride=u.stride).permute(0, 2, 3, 1)
            continue
        if u.kind == "avgpool":
            oh, ow, _ = self.tensors[u.dst]
            h, w = a.shape[1], a.shape[2]
            hi_h = max((oh - 1) * u.stride + u.kh - h - u.pad_h, 0)
            hi_w = max((ow - 1) * u.stride + u.kw - w - u.pad_w, 0)
            an = F.pad(a.permute(0, 3, 1, 2), (u.pad_w, hi_w, u.pad_h, hi_h))
            vals[u.dst] = F.avg_pool2d(an, (u.kh, u.kw), stride=u.stride).permute(0, 2, 3, 1)
            continue
        W = _get(params, u.kernel)
        if u.flat_kernel:
            z = (a.reshape(a.shape[0], -1) @ W).reshape(a.shape[0], 1, 1, u.cout)
        elif u.kh == 1 and u.kw == 1 and u.stride == 1:
            z = a @ W.reshape(u.cin, u.cout)
        elif u.kh == 1 and u.kw == 1:
            z = a[:, ::u.stride, ::u.stride, :] @ W.reshape(u.cin, u.cout)
        else:
            oh, ow, _ = self.tensors[u.dst]
            h, w = a.shape[1], a.shape[2]
            pad_hi_h = max((oh - 1) * u.stride + u.kh - h - u.pad_h, 0)
            pad_hi_w = max((ow - 1) * u.stride + u.kw - w - u.pad_w, 0)
            an = F.pad(a.permute(0, 3, 1, 2), (u.pad_w, pad_hi_w, u.pad_h, pad_hi_h))
            z = F.conv2d(an, W.permute(3, 2, 0, 1), stride=u.stride).permute(0, 2, 3, 1)
        if u.bias is not None:
            z = z + _get(params, u.bias)
        if u.bn_scale is not None:
            mean, var = _get(batch_stats, u.bn_mean), _get(batch_stats, u.bn_var)
            z = (z - mean) * torch.rsqrt(var + u.bn_eps) * _get(params, u.bn_scale) + _get(params, u.bn_bias)
        if u.res is not None:
            z = z + vals[u.res]
        vals[u.dst] = act_fn(u.act, z)
    out = vals[self.out].reshape(xb.shape[0], -1)
    if return_all:
        return out, vals
    return out[0] if single else out
