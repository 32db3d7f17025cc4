"""MAP training on the HIP engine — the reference's ``src/train_map.py`` (``train_map`` ``:111-144``, ``_map_step``
``:52-88``) without JAX.

The gradient of the mean negative log-likelihood of a minibatch is ``sum_i J_i^T u_i`` with the head cotangents
``u_i = (p_i - e_{y_i}) / n`` (classifier) or ``(f_i - y_i) exp(-logvar) / n`` (regressor): ONE pass of the engine's
backward tape over a binding whose examples are the minibatch.  Train-mode BatchNorm adds a per-channel statistics pass
between a unit's convolution and its normalisation (``LIP_OP_BN_STATS``) and the correction
``g' = g - (d beta + xhat d gamma) / R`` of its cotangent (``LIP_OP_BN_TRAIN_BWD``); see DESIGN.md section 4.

A step is six C calls whatever the depth: load the batch, ``lip_train_primal``, ``lip_train_refresh`` (the transposed,
BN-scaled kernels of the data gradients, from the new batch statistics), ``lip_train_loss_head``,
``lip_train_backward``, ``lip_train_adam`` (the prior folded in).  There is no CPU fallback.

The loss is the reference's: the MEAN NLL of the batch plus ``0.5 sum_j a_j theta_j^2`` (not divided by the data set
size).  A classifier puts the precision on every parameter; a regressor on every parameter that is not named ``bias``
(``bias_precision = 0``), and trains its scalar ``logvar`` on the host with the same Adam formula and no prior (theta
excludes it; the reference's tree walk would also penalise it).  A :class:`prior.GroupedPrior` is taken as it is.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Any, Callable, Dict, Iterable, Optional, Tuple, Union

import torch

from . import _native as nv
from .engine import build_consts, compile_net
from .prior import GroupedPrior, check_dim
from .utils import TrainState, flatten_nn_params, param_layout


def cosine_decay_schedule(init_value: float, decay_steps: int, alpha: float = 0.0) -> Callable[[int], float]:
    """``optax.cosine_decay_schedule`` (exponent 1), as ``scale_experiments/train.py:76-81`` uses it:
    ``step -> init_value * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)``."""
    if decay_steps <= 0:
        raise ValueError("cosine_decay_schedule needs a positive number of decay steps")

    def schedule(step: int) -> float:
        c = min(max(int(step), 0), decay_steps) / decay_steps
        return init_value * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * c)) + alpha)

    return schedule


@dataclasses.dataclass
class Adam:
    """``optax.adam`` (``eps_root = 0``): ``lr`` a float or a schedule ``step -> lr`` evaluated at the number of updates
    already applied (0 for the first), as optax's ``scale_by_schedule`` counts."""
    lr: Union[float, Callable[[int], float]]
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8

    def lr_at(self, count: int) -> float:
        return float(self.lr(count)) if callable(self.lr) else float(self.lr)

    def scalar_update(self, grad: float, count: int, mu: float, nu: float) -> Tuple[float, float, float]:
        """the update of one host scalar at its (count + 1)-th step: ``(delta, mu, nu)``"""
        t = count + 1
        mu = self.b1 * mu + (1 - self.b1) * grad
        nu = self.b2 * nu + (1 - self.b2) * grad * grad
        return -self.lr_at(count) * (mu / (1 - self.b1 ** t)) / (math.sqrt(nu / (1 - self.b2 ** t)) + self.eps), mu, nu


class _Binding:
    """the engine handle, primal buffer and head buffers of one batch size; theta, the constants and the workspace are
    the trainer's"""

    def __init__(self, tr: "MapTrainer", n: int):
        lib, dev = tr.lib, tr.device
        self.n = n
        self.cn = cn = compile_net(tr.net, n, tr.params_like, train=True)
        if tr.consts is None:
            tr.consts = build_consts(cn, tr.params_like, tr.stats_like, dev)
            tr.const_plan = cn.const_plan
        elif tr.consts.numel() != cn.const_floats:
            raise nv.NativeError("the constants layout depends on the batch size")
        self.prim = torch.zeros(cn.prim_floats, device=dev, dtype=torch.float32)
        self.U = torch.zeros(n * cn.K, device=dev, dtype=torch.float32)
        work_pp = max(cn.work_pp, cn.train_work_pp)
        if tr.work is None or tr.work.numel() < work_pp:
            tr.work = torch.empty(work_pp, device=dev, dtype=torch.float32)
            for b in tr.bindings.values():                  # every handle follows the grown workspace
                b.bind(tr)
        doubles = 0
        for op in cn.train_tapes[0]:
            if op.kind == nv.OP_BN_STATS:
                q = C.c_int64(0)
                nv.check(lib.lip_train_bn_stats_scratch(op.n_img * op.OH * op.OW, op.N, C.byref(q)), "lip_train_bn_stats_scratch")
                doubles = max(doubles, q.value)
        self.stats_scratch = torch.empty(max(2, doubles), device=dev, dtype=torch.float64)
        h = C.c_void_p()
        nv.check(lib.lip_engine_create(C.byref(h), cn.D, n, cn.K), "lip_engine_create")
        self.h = h
        self._tapes = []
        for which, tape in ((nv.TAPE_PRIMAL, cn.tapes[0]), (nv.TAPE_TRAIN_PRIMAL, cn.train_tapes[0]),
                            (nv.TAPE_TRAIN_BACKWARD, cn.train_tapes[1])):
            arr = (nv.Op * len(tape))(*tape)
            self._tapes.append(arr)
            nv.check(lib.lip_engine_set_tape(h, which, arr, len(tape)), "lip_engine_set_tape")
        rows = []
        for item in cn.const_plan:
            if item[0] == "wt":
                _, u, wo, so = item
                rows += [cn.offsets[u.kernel][0], wo, -1 if so is None else so, u.kh * u.kw, u.cin, u.cout]
        table = (C.c_int64 * max(1, len(rows)))(*rows)
        nv.check(lib.lip_engine_set_refresh(h, table, len(rows) // 6), "lip_engine_set_refresh")
        self.bind(tr)

    def bind(self, tr: "MapTrainer") -> None:
        lib = tr.lib
        nv.check(lib.lip_engine_bind(self.h, nv.ptr(tr.theta), nv.ptr(tr.consts), nv.ptr(self.prim), nv.ptr(tr.work),
                                     tr.work.numel(), 1), "lip_engine_bind")
        nv.check(lib.lip_engine_train_bind(self.h, nv.ptr(tr.consts), self.stats_scratch.data_ptr(),
                                           self.stats_scratch.numel()), "lip_engine_train_bind")

    def destroy(self, lib) -> None:
        if self.h is not None and self.h.value:
            lib.lip_engine_destroy(self.h)
        self.h = None


class MapTrainer:
    """The bindings, the flat ``theta`` and the optimizer state of a MAP training run.

    ``loss_and_grad(x, y)`` evaluates without updating, ``step(x, y)`` applies one Adam step and returns the loss,
    ``state()`` writes ``theta`` and the running statistics back into a ``TrainState`` every ``posterior_lla_*`` accepts.
    One binding per distinct batch size is kept (an epoch's tail batch is smaller); they share ``theta``, the Adam
    moments, the constants (batch and running statistics, transposed kernels) and the workspace.
    """

    def __init__(self, state, model_type: str, alpha, optimizer: Optional[Adam] = None, device=None):
        net = getattr(state, "net", None)
        if net is None:
            raise TypeError("MAP training needs state.net (a NetSpec layer program); there is no CPU fallback")
        if model_type not in ("classifier", "regressor"):
            raise ValueError("model_type must be 'classifier' or 'regressor'")
        self.lib = nv.load()
        if not torch.cuda.is_available():
            raise nv.NativeError("no GPU: MAP training runs on the HIP engine and has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda")
        net.model_type = model_type
        self.net, self.model_type, self.classifier = net, model_type, model_type == "classifier"
        self.opt = optimizer if optimizer is not None else Adam(1e-3)
        self._state0 = state
        self.params_like, self.stats_like = state.params, state.batch_stats
        flat, self._unravel = flatten_nn_params(state.params)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.theta = flat.detach().to(**f32).contiguous().clone()
        self.D = self.theta.numel()
        self.K = net.num_outputs
        self.m, self.v, self.grad = (torch.zeros(self.D, **f32) for _ in range(3))
        self.count = 0                                   # updates applied
        self.logvar = float(state.params["logvar"]["logvar"]) if not self.classifier else 0.0
        self._lv_mu = self._lv_nu = 0.0
        # the regressor's bias_precision = 0 (src/train_map.py:20-30,76): a 0 / 1 mask over theta
        self._mask = None
        if not self.classifier:
            mask = torch.ones(self.D)
            for path, off, shape in param_layout(state.params):
                if path[-1] == "bias":
                    mask[off:off + int(torch.Size(shape).numel())] = 0.0
            self._mask = mask.to(**f32)
        self.set_alpha(alpha)
        self.consts: Optional[torch.Tensor] = None
        self.const_plan = None
        self.work: Optional[torch.Tensor] = None
        self.bindings: Dict[int, _Binding] = {}
        q = C.c_int64(0)
        nv.check(self.lib.lip_train_adam_scratch(self.D, C.byref(q)), "lip_train_adam_scratch")
        self._adam_scratch = torch.empty(q.value, device=self.device, dtype=torch.float64)
        self._out = torch.zeros(3, device=self.device, dtype=torch.float64)      # summed NLL, d logvar, 0.5 sum a theta^2

    def __del__(self):
        for b in getattr(self, "bindings", {}).values():
            try:
                b.destroy(self.lib)
            except Exception:
                pass

    # ------------------------------------------------------------------------------------------ the prior
    def set_alpha(self, alpha) -> None:
        """the prior precision of the steps that follow: a float or a :class:`prior.GroupedPrior`"""
        self.alpha = alpha
        if isinstance(alpha, GroupedPrior):
            self._a_vec, self._a_scalar = check_dim(alpha, self.D).vector(self.device, torch.float32).contiguous(), 0.0
        elif self._mask is not None:
            self._a_vec, self._a_scalar = (self._mask * float(alpha)).contiguous(), 0.0
        else:
            self._a_vec, self._a_scalar = None, float(alpha)

    def prior_vector(self) -> torch.Tensor:
        """(D,) float32 precisions a_j on the device"""
        if self._a_vec is not None:
            return self._a_vec
        return torch.full((self.D,), self._a_scalar, device=self.device, dtype=torch.float32)

    # ------------------------------------------------------------------------------------------ one pass
    def _binding(self, n: int) -> _Binding:
        b = self.bindings.get(n)
        if b is None:
            b = _Binding(self, n)
            self.bindings[n] = b
        return b

    def _load(self, x: torch.Tensor, y: torch.Tensor) -> Tuple[_Binding, torch.Tensor]:
        n = int(x.shape[0])
        if n < 1:
            raise ValueError("empty batch")
        b = self._binding(n)
        xin = self.net.prepare_input(x.detach().to(device=self.device, dtype=torch.float32)).reshape(-1)
        if xin.numel() != n * math.prod(self.net.tensors[0]):
            raise ValueError(f"batch of shape {tuple(x.shape)} does not match the network input {self.net.input_shape_raw}")
        b.prim[b.cn.input_off:b.cn.input_off + xin.numel()] = xin
        if self.classifier:
            t = y.detach().reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
            if t.numel() != n:
                raise ValueError(f"{n} examples need {n} labels, got {tuple(y.shape)}")
        else:
            t = y.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
            if t.numel() != n * self.K:
                raise ValueError(f"{n} examples need ({n}, {self.K}) targets, got {tuple(y.shape)}")
        return b, t

    def _logits_ptr(self, b: _Binding) -> int:
        return b.prim.data_ptr() + 4 * b.cn.a_off[self.net.out]

    def _loss_head(self, b: _Binding, t: torch.Tensor) -> None:
        nv.check(self.lib.lip_train_loss_head(self._logits_ptr(b), t.data_ptr(), b.n, self.K, int(self.classifier),
                                              float(self.logvar), nv.ptr(b.U), self._out.data_ptr(), nv.stream_ptr()),
                 "lip_train_loss_head")

    def _forward_backward(self, b: _Binding, t: torch.Tensor) -> None:
        """train primal, refresh, loss head, backward: the data gradient in ``self.grad``, the sums in ``self._out``"""
        st = nv.stream_ptr()
        nv.check(self.lib.lip_train_primal(b.h, st), "lip_train_primal")
        nv.check(self.lib.lip_train_refresh(b.h, st), "lip_train_refresh")
        self._loss_head(b, t)
        nv.check(self.lib.lip_train_backward(b.h, nv.ptr(b.U), nv.ptr(self.grad), st), "lip_train_backward")

    def _count(self, b: _Binding) -> int:
        return b.n if self.classifier else b.n * self.K

    def loss_and_grad(self, x: torch.Tensor, y: torch.Tensor):
        """``(loss, nll, grad (D,), new_batch_stats)`` of the train-mode MAP loss at the current theta, nothing updated:
        ``nll`` the mean NLL of the batch, ``loss = nll + 0.5 sum a theta^2``, ``grad`` its gradient in theta (float32, on
        the device) and ``new_batch_stats`` the running statistics a step on this batch would leave.  For a regressor
        ``self.dlogvar`` holds d nll / d logvar afterwards."""
        b, t = self._load(x, y)
        keep = self.consts.clone()
        self._forward_backward(b, t)
        out = self._out.cpu()
        new_stats = self._stats_tree()
        self.consts.copy_(keep)                            # the running statistics are not advanced
        a = self.prior_vector()
        reg = 0.5 * float((a.double() * self.theta.double() ** 2).sum())
        nll = float(out[0]) / self._count(b)
        self.dlogvar = float(out[1])
        return nll + reg, nll, self.grad + a * self.theta, new_stats

    def step(self, x: torch.Tensor, y: torch.Tensor) -> float:
        """one Adam step on the batch; returns the loss at the parameters before the update"""
        b, t = self._load(x, y)
        self._forward_backward(b, t)
        o = self.opt
        nv.check(self.lib.lip_train_adam(nv.ptr(self.theta), nv.ptr(self.m), nv.ptr(self.v), nv.ptr(self.grad), nv.ptr(self._a_vec),
                                         self._a_scalar, o.lr_at(self.count), o.b1, o.b2, o.eps, self.count + 1, self.D,
                                         self._out.data_ptr() + 16, self._adam_scratch.data_ptr(), self._adam_scratch.numel(),
                                         nv.stream_ptr()), "lip_train_adam")
        out = self._out.cpu()
        if not self.classifier:
            delta, self._lv_mu, self._lv_nu = o.scalar_update(float(out[1]), self.count, self._lv_mu, self._lv_nu)
            self.logvar += delta
        self.count += 1
        return float(out[0]) / self._count(b) + float(out[2])

    # ------------------------------------------------------------------------------------------ evaluation
    def _eval_consts(self) -> None:
        """the BN constants of the eval-mode primal tape from the running statistics (``build_consts``' formulas)"""
        if self.consts is None:
            return
        run = {item[1].dst: item for item in self.const_plan if item[0] == "run"}
        layout = {path: off for path, off, _ in param_layout(self.params_like)}
        for item in self.const_plan:
            if item[0] == "bn":
                _, u, so, mo, ro = item
                _, _, rm, rv = run[u.dst]
                N = u.cout
                rstd = torch.rsqrt(self.consts[rv:rv + N] + u.bn_eps)
                g0 = layout[u.bn_scale]
                self.consts[so:so + N] = self.theta[g0:g0 + N] * rstd
                self.consts[mo:mo + N] = self.consts[rm:rm + N]
                self.consts[ro:ro + N] = rstd

    def evaluate(self, loader: Iterable) -> Tuple[float, Optional[float]]:
        """eval mode with the running statistics: ``(mean of the batches' mean NLL, mean of their accuracies)`` over a
        re-iterable of ``(x, y)`` (``_eval_classification`` / ``_eval_regression``, ``src/train_map.py:91-109,131-137``);
        the accuracy is None for a regressor"""
        nlls, accs = [], []
        first = True
        for x, y in loader:
            b, t = self._load(x, y)
            if first:
                self._eval_consts()
                first = False
            nv.check(self.lib.lip_engine_primal(b.h, nv.stream_ptr()), "lip_engine_primal")
            self._loss_head(b, t)
            nlls.append(float(self._out[0]) / self._count(b))
            if self.classifier:
                o = b.cn.a_off[self.net.out]
                logits = b.prim[o:o + b.n * self.K].reshape(b.n, self.K)
                accs.append(float((logits.argmax(1) == t).double().mean()))
        if not nlls:
            raise ValueError("evaluate: the loader yielded no batch")
        return sum(nlls) / len(nlls), (sum(accs) / len(accs) if self.classifier else None)

    # ------------------------------------------------------------------------------------------ the state
    def _stats_tree(self) -> Dict[str, Any]:
        tree: Dict[str, Any] = {}
        if self.consts is None:
            return tree
        for item in self.const_plan:
            if item[0] == "run":
                _, u, mo, vo = item
                for path, off in ((u.bn_mean, mo), (u.bn_var, vo)):
                    node = tree
                    for k in path[:-1]:
                        node = node.setdefault(k, {})
                    node[path[-1]] = self.consts[off:off + u.cout].clone()
        return tree

    def state(self) -> TrainState:
        """``theta`` and the running statistics as a ``TrainState`` on the device and in the dtype of the state the
        trainer was built from (``net`` and a fresh ``apply_fn`` attached; ``logvar`` for a regressor)"""
        like = next(iter(torch.as_tensor(l) for _, l in _leaves(self.params_like)))
        to = lambda t: t.to(device=like.device, dtype=like.dtype)
        params = self._unravel(to(self.theta.clone()))
        if not self.classifier:
            params["logvar"] = {"logvar": torch.tensor(self.logvar, device=like.device, dtype=like.dtype)}
        stats = _map_tree(to, self._stats_tree()) if self.consts is not None else _map_tree(to, self.stats_like)
        return self._state0.replace(params=params, batch_stats=stats, apply_fn=self.net.make_apply_fn(self.model_type, stats))


def _leaves(tree, prefix=()):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], prefix + (k,))
    else:
        yield prefix, tree


def _map_tree(fn, tree):
    if isinstance(tree, dict):
        return {k: _map_tree(fn, v) for k, v in tree.items()}
    return fn(torch.as_tensor(tree))


def train_map(state, train_loader: Iterable, test_loader: Iterable, *, model_type: str, num_epochs: int, alpha,
              optimizer: Optional[Adam] = None, log: Optional[Callable[[Dict[str, Any]], None]] = None) -> TrainState:
    """``src/train_map.py:111-144``: ``num_epochs`` passes of Adam steps over ``train_loader`` on the loss
    mean NLL + 0.5 sum a theta^2, then the state with the trained parameters and running statistics.  The loaders are
    re-iterables of ``(x, y)`` tensors (a list of batches, a ``DataLoader``); ``alpha`` a float or a
    :class:`prior.GroupedPrior`; ``optimizer`` an :class:`Adam` (default ``Adam(1e-3)``; the reference's state carries its
    optax optimizer).  After every epoch the test NLL, and for a classifier the accuracy, are taken in eval mode with the
    running statistics and handed to ``log`` as ``dict(epoch, train_loss, test_nll, test_acc)``."""
    trainer = MapTrainer(state, model_type, alpha, optimizer)
    for epoch in range(int(num_epochs)):
        loss = float("nan")
        for x, y in train_loader:
            loss = trainer.step(x, y)
        if log is not None:
            nll, acc = trainer.evaluate(test_loader)
            log(dict(epoch=epoch, train_loss=loss, test_nll=nll, test_acc=acc))
    return trainer.state()
