"""Monte-Carlo and empirical Fisher fits for the diagonal and the Kronecker-factored posteriors.  Not a reference function.

The exact GGN fits push K one-hot probes per example through a backward sweep: fine at K = 10, a thousand sweeps per
example chunk at ResNet-50's K = 1000.  The sweeps take any head cotangent, so the curvature can also be

    (1 / divisor) sum_p sum_i J_i^T u_pi u_pi^T J_i

for raw cotangents u_pi (P, M, K).  A *curvature spec* names them:

* :class:`MCFisher` — ``u = e_yhat - p_i`` with ``yhat ~ p(y | x_i)`` drawn on the device (``lip_head_sample``),
  ``num_samples`` draws per example, divisor S: unbiased for the GGN, S sweeps instead of K.  Regressor: standard
  normals (``lip_fill_normal``), whose second moment is the identity head Hessian.
* :class:`EmpiricalFisher` — ``u = e_y - p_i`` at the true label (regressor: ``(y - f) exp(-logvar / 2)``), one sweep.
* :class:`Cotangents` — a block supplied by the caller.
* ``None`` / ``"ggn"`` — the exact route; this module is not on its path.

The N/M (x exp(-logvar)) factor of ``compute_ggn_vp`` multiplies all of them alike.  The draws of :class:`MCFisher` are
defined per (sample, global example index), so they do not depend on how the examples are chunked over bindings.
"""
from __future__ import annotations

import hashlib
import math
from typing import Optional, Tuple

import torch

MAX_CLASSES = 8192                # lip_head_sample's K


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class MCFisher:
    """``num_samples`` label draws per example from the model's own predictive, reproducible from ``seed``"""

    def __init__(self, num_samples: int, seed: int = 0):
        if not _is_int(num_samples) or num_samples < 1:
            raise ValueError(f"num_samples must be a positive integer, got {num_samples!r}")
        if not _is_int(seed):
            raise ValueError(f"seed must be an integer, got {seed!r}")
        self.num_samples, self.seed = num_samples, seed & (2 ** 64 - 1)

    def key(self):
        return ("mc", self.num_samples, self.seed)

    def check(self, M: int, K: int, model_type: str) -> None:
        if model_type != "regressor" and K > MAX_CLASSES:
            raise ValueError(f"the head sampler takes at most {MAX_CLASSES} classes, the net has {K}")


class EmpiricalFisher:
    """the gradient at the true targets: integer labels (M,) for a classifier, (M, K) values for a regressor"""

    def __init__(self, targets):
        self.targets = torch.as_tensor(targets).detach()

    def key(self):
        t = self.targets.cpu().contiguous()
        return ("ef", str(t.dtype), tuple(t.shape), hashlib.sha1(t.numpy().tobytes()).hexdigest())

    def check(self, M: int, K: int, model_type: str) -> None:
        t = self.targets
        if model_type == "regressor":
            if not t.dtype.is_floating_point:
                raise ValueError(f"regression targets must be floating point, got {t.dtype}")
            if tuple(t.shape) != (M, K):
                raise ValueError(f"regression targets must have shape ({M}, {K}), got {tuple(t.shape)}")
            return
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"class labels must be integers, got {t.dtype}")
        if tuple(t.shape) != (M,):
            raise ValueError(f"class labels must have shape ({M},), got {tuple(t.shape)}")
        if M and (int(t.min()) < 0 or int(t.max()) >= K):
            raise ValueError(f"class labels must lie in 0..{K - 1}")


class Cotangents:
    """raw head cotangents ``U`` (P, M, K) of the caller; the curvature is (1 / divisor) sum_p sum_i J_i^T u u^T J_i"""

    def __init__(self, U, divisor: float = 1.0):
        self.U = torch.as_tensor(U).detach()
        self.divisor = float(divisor)
        if not (self.divisor > 0.0 and math.isfinite(self.divisor)):
            raise ValueError(f"divisor must be positive and finite, got {divisor!r}")

    def key(self):
        return ("cot", self.U.data_ptr(), self.U._version, str(self.U.dtype), tuple(self.U.shape), self.divisor)

    def check(self, M: int, K: int, model_type: str) -> None:
        if not self.U.dtype.is_floating_point:
            raise ValueError(f"cotangents must be floating point, got {self.U.dtype}")
        if self.U.dim() != 3 or tuple(self.U.shape[1:]) != (M, K) or self.U.shape[0] < 1:
            raise ValueError(f"cotangents must have shape (P, {M}, {K}) with P >= 1, got {tuple(self.U.shape)}")


def resolve(curvature):
    """``None`` for the exact route (``None`` / ``"ggn"``), the spec otherwise; anything else raises ``ValueError``"""
    if curvature is None or (isinstance(curvature, str) and curvature == "ggn"):
        return None
    if isinstance(curvature, (MCFisher, EmpiricalFisher, Cotangents)):
        return curvature
    raise ValueError(f"curvature must be None, 'ggn', MCFisher, EmpiricalFisher or Cotangents, got {curvature!r}")


def spec_key(curvature):
    """the hashable cache key of a curvature argument (``None`` for the exact route)"""
    spec = resolve(curvature)
    return None if spec is None else spec.key()


def checked(curvature, state, Z, model_type):
    """:func:`resolve`, with the spec checked against (len(Z), the net's outputs, model_type) before anything is bound"""
    spec = resolve(curvature)
    if spec is not None:
        spec.check(int(Z.shape[0]), int(state.net.num_outputs), model_type)
    return spec


def sample_head_cotangents(probs: torch.Tensor, num_samples: int, seed: int, example_offset: int = 0,
                           return_labels: bool = False):
    """``U (S, n, K)`` float32 with ``U[s, i] = e_yhat - probs[i]``, ``yhat ~ probs[i]`` (``lip_head_sample``: the draw
    of (s, example_offset + i) is a pure function of the row, the seed and those two indices); with ``return_labels``
    also the (S, n) int32 labels.  ``probs`` is a contiguous float32 device (n, K) tensor and is only read."""
    from . import _native as nv
    if not (torch.is_tensor(probs) and probs.dim() == 2 and probs.dtype == torch.float32):
        raise ValueError("probs must be a float32 (n, K) tensor")
    n, K = probs.shape
    S = int(num_samples)
    lib = nv.load()
    U = torch.empty(S, n, K, device=probs.device, dtype=torch.float32)
    labels = torch.empty(S, n, device=probs.device, dtype=torch.int32) if return_labels else None
    nv.check(lib.lip_head_sample(nv.ptr(probs), n, K, S, int(seed) & (2 ** 64 - 1), int(example_offset), nv.ptr(U),
                                 nv.ptr(labels), nv.stream_ptr()), "lip_head_sample")
    return (U, labels) if return_labels else U


def _probs_view(eng) -> torch.Tensor:
    """the engine's own (n, K) probability slice of ``prim`` (no clone)"""
    o = eng.cn.prob_off
    return eng.prim[o:o + eng.n * eng.K].view(eng.n, eng.K)


class CotangentSource:
    """The cotangents of one fit over M examples, binding by binding: ``source(eng, example_offset) -> (U, divisor)``
    with U (P, eng.n, K) float32 on the engine's device.  Whatever spans the whole set is made once (the regressor's
    normal block of :class:`MCFisher`: ``fill_normal(S, M K, seed)`` read as (S, M, K), sliced per binding)."""

    def __init__(self, spec, M: int, model_type: str, logvar: Optional[float] = None):
        self.spec, self.M, self.model_type, self.logvar = spec, int(M), model_type, logvar
        self._normals = None

    def __call__(self, eng, example_offset: int) -> Tuple[torch.Tensor, float]:
        spec, off, n, K = self.spec, int(example_offset), eng.n, eng.K
        spec.check(self.M, K, self.model_type)
        if off < 0 or off + n > self.M:
            raise ValueError(f"examples {off}..{off + n} lie outside the {self.M} examples of the fit")
        regressor = self.model_type == "regressor"
        if isinstance(spec, MCFisher):
            if not regressor:
                return sample_head_cotangents(_probs_view(eng), spec.num_samples, spec.seed, off), float(spec.num_samples)
            if self._normals is None:
                from . import krylov
                self._normals = krylov.fill_normal(spec.num_samples, self.M * K, spec.seed, eng.device).view(
                    spec.num_samples, self.M, K)
            return self._normals[:, off:off + n].contiguous(), float(spec.num_samples)
        if isinstance(spec, EmpiricalFisher):
            if regressor:
                if self.logvar is None:
                    raise ValueError("the regressor's empirical Fisher needs logvar")
                y = spec.targets[off:off + n].to(device=eng.device, dtype=torch.float32)
                return ((y - eng.outputs()) * math.exp(-0.5 * float(self.logvar)))[None].contiguous(), 1.0
            y = spec.targets[off:off + n].to(device=eng.device, dtype=torch.int64)
            hot = torch.zeros(n, K, device=eng.device, dtype=torch.float32)
            hot[torch.arange(n, device=eng.device), y] = 1.0
            return (hot - _probs_view(eng))[None].contiguous(), 1.0
        U = spec.U[:, off:off + n].to(device=eng.device, dtype=torch.float32).contiguous()
        return U, spec.divisor


def cotangents_for(spec, eng, example_offset: int, model_type: str, logvar: Optional[float] = None,
                   num_examples: Optional[int] = None) -> Tuple[torch.Tensor, float]:
    """``(U_chunk (P, eng.n, K), divisor)`` of one binding whose first example is number ``example_offset`` of the
    ``num_examples`` of the fit (default: the binding is the last one).  MC classifier: the head sampler on the engine's
    probabilities, divisor S; MC regressor: the slice of the (S, M, K) normal block, divisor S; empirical Fisher:
    ``e_y - p`` resp. ``(y - f) exp(-logvar / 2)``, divisor 1; :class:`Cotangents`: the slice and its divisor."""
    M = int(example_offset) + eng.n if num_examples is None else int(num_examples)
    return CotangentSource(spec, M, model_type, logvar)(eng, example_offset)


def _engines_with_offsets(state, Z, model_type, full_set_size, example_chunk):
    from . import ggn as _ggn
    M = Z.shape[0]
    if example_chunk is None or example_chunk >= M:
        return [(_ggn.get_engine(state, Z, model_type), 0)]
    engines = _ggn.ExampleChunkedGGN(state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk).engines
    return [(eng, j * example_chunk) for j, eng in enumerate(engines)]


def source_for(spec, state, Z, model_type) -> CotangentSource:
    from . import ggn as _ggn
    return CotangentSource(spec, Z.shape[0], model_type, _ggn._logvar(state) if model_type == "regressor" else None)


def compute_ggn_diag(state, Z, model_type, spec, full_set_size=None, example_chunk: Optional[int] = None) -> torch.Tensor:
    """diag((recal / divisor) sum_p sum_i J_i^T u_pi u_pi^T J_i) -> (D,) float32 on the device: the cotangents of ``spec``
    through one square-accumulating backward sweep per binding (:meth:`LinearizedNet.vjp_sqsum`, 'raw'), with the
    N/M (x exp(-logvar)) factor and the chunking of :func:`ggn.compute_ggn_diag`; chunk j's examples start at
    ``example_offset = j * example_chunk``."""
    spec.check(int(Z.shape[0]), int(state.net.num_outputs), model_type)
    from . import ggn as _ggn
    M = Z.shape[0]
    recal = (full_set_size or M) / M
    if model_type == "regressor":
        recal *= math.exp(-_ggn._logvar(state))
    source = source_for(spec, state, Z, model_type)
    bound = _engines_with_offsets(state, Z, model_type, full_set_size, example_chunk)
    Y = torch.zeros(bound[0][0].D, device=bound[0][0].device, dtype=torch.float32)
    divisor = 1.0
    for eng, off in bound:
        U, divisor = source(eng, off)
        eng.vjp_sqsum(U, "raw", 1.0, out=Y)
    return Y.mul_(recal / divisor)
