"""Layer-wise prior precisions for the diagonal, KFAC and EKFAC posteriors by marginal likelihood.  Not a reference
function.

With a prior that is constant on every Kronecker block, the eigenbasis of a block does not depend on the precisions, so
the curvature is diagonalised once and the evidence in all log alpha_g is two sums per group over the curvature
eigenvalues x that belong to the group (r = N / M):

    L_g = sum_x log1p(r x / alpha_g),        T_g = sum_x (r x / alpha_g) / (1 + r x / alpha_g),
    value  = -1/2 sum_g alpha_g ||theta_g||^2 - 1/2 sum_g L_g,
    grad_g = -1/2 alpha_g ||theta_g||^2 + 1/2 T_g            (with respect to log alpha_g),

the convention of ``train_alpha._lml_from_spectrum``, in which the D_g log alpha_g terms cancel.  x runs over
c_l lam_i mu_j of a KFAC block, the entries of a block's second-moment matrix Lam_l for EKFAC, and GGN diagonal entries
for the diagonal posterior and the parameters outside every block.

An :class:`EvidencePlan` holds one float64 value pool and a segment table over it (``KRON``: rows + cols numbers that
stand for rows * cols eigenvalues; ``LIST``: the eigenvalues themselves), built once per fit.  On the GPU
``plan.terms`` is ``lip_evidence_terms``: one streaming kernel over fixed chunks of ``CHUNK`` terms and a second launch
that folds every group's chunks in order, bitwise reproducible, reading log alpha from device memory; a KFAC block's
outer product is never written.  On CPU tensors the same definition is evaluated in float64 torch, which keeps the
host algebra testable without a device (as ``kfac.fit_blocks`` is).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ggn as _ggn
from . import kfac as _kfac
from .prior import GroupedPrior, check_dim
from .train_alpha import Adam, _adam_update
from .utils import flatten_nn_params

CHUNK = 32768                       # terms per chunk: one workgroup of the kernel reduces one chunk
KRON, LIST = 0, 1                   # LIP_EV_KRON, LIP_EV_LIST


class Segment(NamedTuple):
    """``KRON``: the terms scale * max(lam_i, 0) * max(mu_j, 0), lam = vals[off : off + rows], mu the ``cols`` values
    right behind it; ``LIST``: the terms scale * max(vals[off + i], 0), i < rows (cols = 1).  ``group``: the prior group
    that owns the terms."""
    kind: int
    off: int
    rows: int
    cols: int
    scale: float
    group: int

    @property
    def terms(self) -> int:
        return self.rows * self.cols if self.kind == KRON else self.rows


def _checked_segments(segments, n_vals: int, G: int) -> List[Segment]:
    out = []
    for k, s in enumerate(segments):
        s = Segment(int(s[0]), int(s[1]), int(s[2]), int(s[3]), float(s[4]), int(s[5]))
        if s.kind not in (KRON, LIST):
            raise ValueError(f"segment {k}: unknown kind {s.kind}")
        if not 0 <= s.group < G:
            raise ValueError(f"segment {k}: group {s.group} outside [0, {G})")
        if s.rows <= 0 or s.cols <= 0 or (s.kind == LIST and s.cols != 1):
            raise ValueError(f"segment {k}: rows and cols must be positive (cols = 1 for a list), got {s.rows} x {s.cols}")
        if not (math.isfinite(s.scale) and s.scale >= 0.0):
            raise ValueError(f"segment {k}: the scale must be finite and not negative, got {s.scale}")
        need = s.rows + s.cols if s.kind == KRON else s.rows
        if s.off < 0 or s.off + need > n_vals:
            raise ValueError(f"segment {k}: values [{s.off}, {s.off + need}) run past the pool of {n_vals}")
        out.append(s)
    if not out:
        raise ValueError("an evidence plan needs at least one segment")
    return out


def chunk_table(segments: Sequence[Segment], chunk: int = CHUNK) -> List[Tuple[int, int]]:
    """[(segment index, first term)]: every segment, in table order, cut into chunks of ``chunk`` consecutive terms, the
    last chunk of a segment shorter; the chunks cover every term exactly once"""
    return [(k, start) for k, s in enumerate(segments) for start in range(0, s.terms, chunk)]


def group_chunks(segments: Sequence[Segment], chunks: Sequence[Tuple[int, int]], G: int) -> Tuple[List[int], List[int]]:
    """``(ptr (G + 1), idx (n_chunks))``: the chunks of group g are idx[ptr[g] : ptr[g + 1]], in chunk order"""
    per = [[] for _ in range(G)]
    for c, (k, _) in enumerate(chunks):
        per[segments[k].group].append(c)
    ptr = [0]
    for p in per:
        ptr.append(ptr[-1] + len(p))
    return ptr, [c for p in per for c in p]


def _upload(array, device) -> torch.Tensor:
    """the bytes of a ctypes array as a device tensor"""
    return torch.frombuffer(bytearray(array), dtype=torch.uint8).to(device)


class EvidencePlan:
    """The curvature spectrum of one fit as a value pool with a segment table, and what the evidence needs beside it.

    ``vals``: (n,) float64 on the device of the fit (CPU included); ``segments``: :class:`Segment` tuples over it;
    ``theta_sqnorms`` (G,): ||theta_g||^2 (``GroupedPrior.group_sqnorms``); ``names``: the G group names.  The chunk and
    group-to-chunks tables are made here on the host and, for a device pool, uploaded once."""

    def __init__(self, vals: torch.Tensor, segments, theta_sqnorms: torch.Tensor, names: Sequence[str], chunk: int = CHUNK):
        if vals.dim() != 1 or vals.dtype != torch.float64 or vals.numel() == 0:
            raise ValueError("the value pool must be a non-empty float64 vector")
        self.vals = vals.detach().contiguous()
        self.names = [str(n) for n in names]
        self.G = len(self.names)
        self.chunk = int(chunk)
        if self.chunk < 1:
            raise ValueError("chunk must be positive")
        self.segments = _checked_segments(segments, self.vals.numel(), self.G)
        self.theta_sqnorms = torch.as_tensor(theta_sqnorms, dtype=torch.float64).detach().reshape(-1).to(self.vals.device)
        if self.theta_sqnorms.numel() != self.G:
            raise ValueError(f"{self.G} groups need {self.G} squared norms, got {self.theta_sqnorms.numel()}")
        self.chunks = chunk_table(self.segments, self.chunk)
        self.group_ptr, self.group_idx = group_chunks(self.segments, self.chunks, self.G)
        self._dev = None
        if self.vals.is_cuda:
            self._bind()

    @property
    def terms_per_group(self) -> torch.Tensor:
        """(G,) int64: the number of eigenvalues every group owns"""
        n = torch.zeros(self.G, dtype=torch.int64)
        for s in self.segments:
            n[s.group] += s.terms
        return n

    def _bind(self):
        from . import _native as nv
        lib = nv.load()
        dev = self.vals.device
        segs = (nv.EvSeg * len(self.segments))(*[nv.EvSeg(s.kind, s.group, s.off, s.rows, s.cols, s.scale) for s in self.segments])
        chunks = (nv.EvChunk * len(self.chunks))(*[nv.EvChunk(start, k, 0) for k, start in self.chunks])
        need = C.c_int64(0)
        nv.check(lib.lip_evidence_terms_scratch(len(self.chunks), C.byref(need)), "lip_evidence_terms_scratch")
        self._dev = dict(
            segs_host=segs, segs=_upload(segs, dev), chunks=_upload(chunks, dev),
            ptr=torch.tensor(self.group_ptr, dtype=torch.int64, device=dev),
            idx=torch.tensor(self.group_idx, dtype=torch.int32, device=dev),
            scratch=torch.empty(need.value, dtype=torch.float64, device=dev))

    def terms(self, log_alphas, rescale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(L, T)``, each (G,) float64 on the pool's device, at alpha_g = exp(log_alphas[g]) and r = ``rescale``"""
        la = torch.as_tensor(log_alphas, dtype=torch.float64, device=self.vals.device).reshape(-1).contiguous()
        if la.numel() != self.G:
            raise ValueError(f"{self.G} groups need {self.G} log precisions, got {la.numel()}")
        if not self.vals.is_cuda:
            return terms_torch(self.vals, self.segments, la, float(rescale), self.G)
        from . import _native as nv
        d = self._dev
        out = torch.empty(self.G, 2, dtype=torch.float64, device=self.vals.device)
        nv.check(nv.load().lip_evidence_terms(
            self.vals.data_ptr(), self.vals.numel(), C.addressof(d["segs_host"]), d["segs"].data_ptr(), len(self.segments),
            d["chunks"].data_ptr(), len(self.chunks), self.chunk, d["ptr"].data_ptr(), d["idx"].data_ptr(), la.data_ptr(),
            self.G, float(rescale), out.data_ptr(), d["scratch"].data_ptr(), d["scratch"].numel(), nv.stream_ptr()),
            "lip_evidence_terms")
        return out[:, 0], out[:, 1]


def terms_torch(vals: torch.Tensor, segments: Sequence[Segment], log_alphas: torch.Tensor, rescale: float, G: int):
    """the definition of ``lip_evidence_terms`` in float64 torch on the device of ``vals``: ``(L (G,), T (G,))``"""
    alphas = torch.exp(log_alphas.double())
    L = torch.zeros(G, dtype=torch.float64, device=vals.device)
    T = torch.zeros_like(L)
    for s in segments:
        if s.kind == KRON:
            lam = vals[s.off:s.off + s.rows].clamp_min(0.0)
            mu = vals[s.off + s.rows:s.off + s.rows + s.cols].clamp_min(0.0)
            x = s.scale * torch.outer(lam, mu).reshape(-1)
        else:
            x = s.scale * vals[s.off:s.off + s.rows].clamp_min(0.0)
        x = rescale * x / alphas[s.group]
        L[s.group] += torch.log1p(x).sum()
        T[s.group] += (x / (1.0 + x)).sum()
    return L, T


def lml_structured(log_alphas, plan: EvidencePlan, rescale: float):
    """``(value, grad)``: the layer-wise evidence of the module docstring at the log precisions ``log_alphas`` (G,) and
    its exact gradient (G,) float64 in them, on the plan's device"""
    la = torch.as_tensor(log_alphas, dtype=torch.float64, device=plan.vals.device).reshape(-1)
    L, T = plan.terms(la, rescale)
    at2 = torch.exp(la) * plan.theta_sqnorms
    value = -0.5 * at2.sum() - 0.5 * L.sum()
    return float(value), -0.5 * at2 + 0.5 * T


def fit_log_alphas_structured(plan: EvidencePlan, rescale: float, log_alphas0, alpha_lr: float = 5e-2, steps: int = 200):
    """The Adam ascent of ``train_alpha.fit_log_alphas`` on the structured evidence: ``(log_alphas, history)`` with
    history = [(alphas (G,) float64 on the CPU, value)] before each step.  With G = 1 it walks the trajectory of
    ``train_alpha._fit_from_spectrum`` on the same spectrum."""
    la = torch.as_tensor(log_alphas0, dtype=torch.float64, device=plan.vals.device).reshape(-1).clone()
    opt = Adam(alpha_lr)
    st = dict(count=0, mu=torch.zeros_like(la), nu=torch.zeros_like(la))
    history = []
    for _ in range(steps):
        v, g = lml_structured(la, plan, rescale)
        history.append((torch.exp(la).cpu(), v))
        upd, st = _adam_update(opt, -g, st)
        la = la + upd
    return la, history


# ---- plans from the curvature of a fit (any device, CPU included) -----------------------------------------------------
def _block_name(b) -> str:
    return "/".join(str(k) for k in b.unit.kernel[:-1])


def block_groups(prior: GroupedPrior, blocks, D: int) -> List[int]:
    """the prior group of every layer block; ``ValueError`` naming the block and two of its groups when a block is not
    inside one group (the Kronecker eigenbasis of such a block would move with the precisions).  Pure Python."""
    check_dim(prior, D)
    probe = prior.with_values(torch.arange(1, prior.G + 1, dtype=torch.float64))     # the precision of a row names its group
    out = []
    for b in blocks:
        try:
            ids = torch.unique(_kfac.block_prior_rows(probe, b, D))
        except ValueError:
            ids = None
        if ids is None or ids.numel() != 1:
            end = b.off + b.Mt * b.N
            inside = [g for g in range(prior.G) if any(o < end and o + n > b.off for o, n in prior.segments(g))]
            raise ValueError(f"the ({b.Mt}, {b.N}) block of {_block_name(b)} at flat offset {b.off} lies in the prior groups "
                             f"{prior.names[inside[0]]!r} and {prior.names[inside[1]]!r}: the layer-wise evidence of a "
                             f"Kronecker-factored posterior needs one precision per block (groups='layer' gives that)")
        out.append(int(ids[0]) - 1)
    return out


def _group_ids(prior: GroupedPrior) -> torch.Tensor:
    gid = torch.empty(prior.D, dtype=torch.int64)
    for g, (_, segs) in enumerate(prior.table):
        for o, n in segs:
            gid[o:o + n] = g
    return gid


def _remainder_segments(prior: GroupedPrior, rem: torch.Tensor, off: int) -> List[Segment]:
    """``LIST`` segments over the remainder's diagonal stored at ``off`` in the order of ``rem``: one per contiguous run
    of one group"""
    if rem.numel() == 0:
        return []
    gids, counts = torch.unique_consecutive(_group_ids(prior)[rem], return_counts=True)
    segs = []
    for g, n in zip(gids.tolist(), counts.tolist()):
        segs.append(Segment(LIST, off, n, 1, 1.0, g))
        off += n
    return segs


def _finish(parts, segments, prior: GroupedPrior, flat: torch.Tensor) -> EvidencePlan:
    vals = torch.cat([p.reshape(-1).double() for p in parts]).contiguous()
    return EvidencePlan(vals, segments, prior.group_sqnorms(flat), prior.names)


def plan_from_diag(diag: torch.Tensor, prior: GroupedPrior, flat: torch.Tensor) -> EvidencePlan:
    """the plan of the diagonal posterior from its (D,) GGN diagonal built at N/M = 1: the prior's own segments"""
    check_dim(prior, diag.numel())
    segments = [Segment(LIST, o, n, 1, 1.0, g) for g, (_, segs) in enumerate(prior.table) for o, n in segs]
    return _finish([diag.detach()], segments, prior, flat)


def plan_from_kfac(blocks, As, Ss, M: int, classifier: bool, scale: float, prior: GroupedPrior, flat: torch.Tensor,
                   diag: Optional[torch.Tensor] = None, groups: Optional[List[int]] = None) -> EvidencePlan:
    """the plan of the KFAC posterior from its factors: per block two ``eigvalsh`` calls (the final classifier block
    centred, as ``kfac.kfac_spectrum`` does) and one ``KRON`` segment with scale = ``scale`` / (M T_l); ``diag``: the
    (D,) GGN diagonal at N/M = 1, read at the parameters outside every block (not needed when there is none)"""
    from .last_layer_kron import centre
    D = flat.numel()
    groups = block_groups(prior, blocks, D) if groups is None else groups
    parts, segments, off = [], [], 0
    for b, A, S, g in zip(blocks, As, Ss, groups):
        S = centre(S) if (classifier and b.final) else S
        parts += [torch.linalg.eigvalsh(0.5 * (A + A.T)), torch.linalg.eigvalsh(0.5 * (S + S.T))]
        segments.append(Segment(KRON, off, b.Mt, b.N, scale / (M * b.T), g))
        off += b.Mt + b.N
    return _with_remainder(parts, segments, off, blocks, prior, flat, diag)


def plan_from_ekfac(blocks, Lams, scale: float, prior: GroupedPrior, flat: torch.Tensor, diag: Optional[torch.Tensor] = None,
                    groups: Optional[List[int]] = None) -> EvidencePlan:
    """the plan of the EKFAC posterior from the second moments Lam_l (Mt, N) in the orthonormal Kronecker eigenbasis of
    every block (unscaled, summed over the examples): one ``LIST`` segment per block with scale ``scale``"""
    D = flat.numel()
    groups = block_groups(prior, blocks, D) if groups is None else groups
    parts, segments, off = [], [], 0
    for b, Lam, g in zip(blocks, Lams, groups):
        parts.append(Lam.detach())
        segments.append(Segment(LIST, off, b.Mt * b.N, 1, scale, g))
        off += b.Mt * b.N
    return _with_remainder(parts, segments, off, blocks, prior, flat, diag)


def _with_remainder(parts, segments, off, blocks, prior, flat, diag):
    rem = _kfac.remainder_indices(blocks, flat.numel())
    if rem.numel():
        if diag is None:
            raise ValueError(f"{rem.numel()} parameters lie outside every block: the plan needs the GGN diagonal")
        parts = parts + [diag.detach().double()[rem.to(diag.device)].to(parts[0].device)]
        segments = segments + _remainder_segments(prior, rem, off)
    return _finish(parts, segments, prior, flat)


# ---- plans of a bound network ---------------------------------------------------------------------------------------
def _scale(state, model_type) -> float:
    return math.exp(-_ggn._logvar(state)) if model_type == "regressor" else 1.0


def _flat(state) -> torch.Tensor:
    return flatten_nn_params(state.params)[0].detach()


def plan_diag(state, X, model_type, prior: GroupedPrior, curvature=None) -> EvidencePlan:
    """the plan of the diagonal posterior of (state, X): ``ggn.compute_ggn_diag`` at N/M = 1 (with the curvature spec
    ``curvature`` of ``fisher.py`` when one is given) under any grouping"""
    flat = _flat(state)
    check_dim(prior, flat.numel())
    return plan_from_diag(_ggn.compute_ggn_diag(state, X, model_type, curvature=curvature).double(), prior, flat)


def plan_kfac(state, X, model_type, prior: GroupedPrior, curvature=None) -> EvidencePlan:
    """the plan of the KFAC posterior of (state, X) from ``kfac.compute_kfac_factors``; a prior that is not constant over
    every block is refused before anything is bound or allocated"""
    flat = _flat(state)
    groups = block_groups(prior, _kfac.block_table(state), flat.numel())
    blocks, As, Ss, M = _kfac.compute_kfac_factors(state, X, model_type, curvature=curvature)
    diag = None
    if _kfac.remainder_indices(blocks, flat.numel()).numel():
        diag = _ggn.compute_ggn_diag(state, X, model_type, curvature=curvature)
    return plan_from_kfac(blocks, As, Ss, M, model_type != "regressor", _scale(state, model_type), prior, flat, diag, groups)


def plan_ekfac(state, X, model_type, prior: GroupedPrior, moments: Optional[str] = None, curvature=None) -> EvidencePlan:
    """the plan of the EKFAC posterior of (state, X): the second moments of ``ekfac.compute_ekfac_scales`` in the
    orthonormal bases of ``ekfac.orthonormal_bases``, exactly as ``ekfac._spectrum_ekfac`` builds them; refusals as
    :func:`plan_kfac`"""
    from . import ekfac as _ekfac
    flat = _flat(state)
    groups = block_groups(prior, _kfac.block_table(state), flat.numel())
    moments = _ekfac._route(moments, curvature)
    blocks, As, Ss, M = _kfac.compute_kfac_factors(state, X, model_type, curvature=curvature)
    bases = _ekfac.orthonormal_bases(blocks, As, Ss, model_type != "regressor")
    Lams = _ekfac.compute_ekfac_scales(state, X, model_type, bases, **_ekfac._route_kwargs(moments, curvature))
    diag = None
    if _kfac.remainder_indices(blocks, flat.numel()).numel():
        diag = _ggn.compute_ggn_diag(state, X, model_type, curvature=curvature)
    return plan_from_ekfac(blocks, Lams, _scale(state, model_type), prior, flat, diag, groups)
