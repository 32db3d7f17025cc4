"""GGN operators — same call surface as the reference's ``src/ggn.py``, computed by the HIP engine.

``compute_ggn_vp`` (``src/ggn.py:97``), ``compute_W_vps`` (``:9``), ``compute_ggn_dense`` (``:149``),
``build_WTW`` (``:198``), ``build_WTWz`` (``:233``), ``ensure_symmetry`` (``:277``).

The reference returns closures that callers ``vmap`` over probe vectors.  A ctypes call cannot be
vmapped, and every consumer is multi-vector anyway, so the closures here are *block operators*:
called on ``(D,)`` they return ``(D,)``; called on ``(P, D)`` (rows = probes, the reference's
``(S, D)`` / ``(P, D)`` layout, ``src/sample.py:151``, ``src/stochtrace.py:28``) they process the whole
block in one engine call; ``.cols(M)`` takes the ``(D, k)`` column layout the reference uses when it
calls an oracle on a matrix (``src/stochtrace.py:64,74,177``).  Inputs are never mutated; outputs are
fresh float32 device tensors.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .engine import LinearizedNet
from .utils import flatten_nn_params

_ENGINE_CACHE = {}
_ENGINE_CACHE_MAX = 4


def _leaves(tree):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k])
    else:
        yield tree


def engine_key(state, Z, model_type):
    """Cache key of a binding: the factories of the reference snapshot ``flat_params`` at factory time
    (``src/ggn.py:10,108``) — so does the key (data pointers + in-place version counters)."""
    return (model_type, id(state.net), tuple(Z.shape), Z.data_ptr(), Z._version,
            tuple((t.data_ptr(), t._version) for t in _leaves(state.params) if torch.is_tensor(t)),
            tuple((t.data_ptr(), t._version) for t in _leaves(state.batch_stats) if torch.is_tensor(t)))


_EVICTION_HOOKS = []          # callables(key) run when a binding leaves the cache (the sampler drops its parts)
_CLEAR_HOOKS = []             # callables() run by clear_engine_cache (caches whose entries may outlive their binding)


_SHARED_WORK = {}


def shared_workspace(device) -> torch.Tensor:
    """ONE probe workspace per device for the cached engines: the workspace is scratch inside a call and the calls of a
    process run one after the other on one stream, so the bindings need not own one each (four cached engines x 8 GB
    before, and 8 GB held the CIFAR net to 85 probes per pass — the 256-probe blocks of the Krylov loops ran as
    85 + 85 + 85 + 1).  An eighth of the card's memory, at most 32 GB (340 probes of the CIFAR config per pass);
    ``LIP_WORKSPACE_GB`` overrides."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    w = _SHARED_WORK.get(idx)
    if w is None:
        import os
        gb = os.environ.get("LIP_WORKSPACE_GB")
        total = torch.cuda.get_device_properties(idx).total_memory
        nbytes = int(float(gb) * (1 << 30)) if gb else min(32 << 30, total // 8)
        w = torch.empty(nbytes // 4, device=torch.device("cuda", idx), dtype=torch.float32)
        _SHARED_WORK[idx] = w
    return w


def get_engine(state, Z, model_type, workspace_bytes: Optional[int] = None) -> LinearizedNet:
    """One engine per (theta snapshot, Z snapshot, model_type).  The cache is LRU: a hit moves the binding to the
    fresh end, so the inducing-point engine an evaluation loop returns to every batch survives the per-batch
    prediction engines that pass through (``scale_experiments/evaluate.py:98-154``).  The bindings share one probe
    workspace (:func:`shared_workspace`) unless ``workspace_bytes`` asks for a private one."""
    key = engine_key(state, Z, model_type)
    eng = _ENGINE_CACHE.pop(key, None)
    if eng is None:
        if workspace_bytes is None:
            dev = torch.device("cuda")
            work = shared_workspace(dev)
            try:
                eng = LinearizedNet(state, Z, model_type, work=work)
            except ValueError as err:
                if "shared workspace" not in str(err):
                    raise
                eng = LinearizedNet(state, Z, model_type)     # one probe does not fit the pool: a private workspace
        else:
            eng = LinearizedNet(state, Z, model_type, workspace_bytes=workspace_bytes)
        eng._keepalive = (state.params, state.batch_stats, Z)   # keep the keyed storage alive
        eng.cache_key = key
        while len(_ENGINE_CACHE) >= _ENGINE_CACHE_MAX:
            old = next(iter(_ENGINE_CACHE))
            _ENGINE_CACHE.pop(old)
            for hook in _EVICTION_HOOKS:
                hook(old)
    _ENGINE_CACHE[key] = eng                                    # (re-)insert at the fresh end
    return eng


def clear_engine_cache():
    for key in list(_ENGINE_CACHE):
        _ENGINE_CACHE.pop(key)
        for hook in _EVICTION_HOOKS:
            hook(key)
    for hook in _CLEAR_HOOKS:
        hook()


class BlockOperator:
    """A linear map applied to one vector ``(n_in...)`` or to a block ``(P, n_in...)``."""

    def __init__(self, fn_block, in_shape, out_shape, engine=None, tag=""):
        self._fn, self.in_shape, self.out_shape = fn_block, tuple(in_shape), tuple(out_shape)
        self.engine, self.tag = engine, tag

    def __call__(self, v: torch.Tensor) -> torch.Tensor:
        nd = len(self.in_shape)
        if v.dim() == nd:
            return self._fn(v[None])[0]
        if v.dim() == nd + 1:
            return self._fn(v)
        raise ValueError(f"{self.tag}: expected shape {self.in_shape} or (P,)+{self.in_shape}, got {tuple(v.shape)}")

    def rows(self, Mrows: torch.Tensor) -> torch.Tensor:      # (P, n_in) -> (P, n_out)
        return self._fn(Mrows)

    def cols(self, Mcols: torch.Tensor) -> torch.Tensor:      # (n_in, k) -> (n_out, k)
        return self._fn(Mcols.T.contiguous()).T


def attach_quadratic_forms(op: "BlockOperator", eng, scale: float, alpha: float = 0.0) -> "BlockOperator":
    """``op.quadratic_forms(V) -> (P,) float64``: v^T (scale GGN + alpha I) v for every row of V WITHOUT the backward sweep:
    GGN = sum_i J_i^T L_i L_i^T J_i (``src/ggn.py:16-39``), so v^T GGN v = sum_i ||L_i^T J_i v||^2 — one tangent-forward
    sweep and the K-vector head (``lip_jvp``, ``LIP_HEAD_LT``), half the arithmetic of the product and no (P, D) output block.
    The estimators that only need eps^T X eps (Hutchinson ``src/stochtrace.py:30-34``, the two quadratic forms of Hutch++
    ``:75,109-111,133-134``) use it when the operator offers it; every other operator goes through its products."""
    from . import krylov
    c = math.sqrt(scale)

    def quadratic_forms(V):
        Vb = V.to(device=eng.device, dtype=torch.float32).contiguous()
        U = eng.jvp(Vb, "lt", c).double().reshape(Vb.shape[0], -1)
        q = (U * U).sum(1)
        if alpha != 0.0:
            q = q + float(alpha) * krylov.bdot(Vb, Vb).double()
        return q

    op.quadratic_forms = quadratic_forms
    return op


def attach_quadratic_forms_diag(op: "BlockOperator", eng, scale: float, a: torch.Tensor) -> "BlockOperator":
    """:func:`attach_quadratic_forms` for a vector prior precision: v^T (scale GGN + diag(a)) v.  The GGN term is the same
    tangent-forward sweep; the prior term sum_j a_j v_j^2 is one weighted dot (``lip_bdot_w``), no (P, D) temporary."""
    from . import krylov
    c = math.sqrt(scale)

    def quadratic_forms(V):
        Vb = V.to(device=eng.device, dtype=torch.float32).contiguous()
        U = eng.jvp(Vb, "lt", c).double().reshape(Vb.shape[0], -1)
        return (U * U).sum(1) + krylov.bdot_w(Vb, Vb, a).double()

    op.quadratic_forms = quadratic_forms
    return op


def _logvar(state):
    return float(torch.as_tensor(state.params["logvar"]["logvar"]).detach().cpu())


class ExampleChunkedGGN:
    """GGN block operator over a data set too large for one engine binding: the examples are split into chunks,
    each chunk gets its own engine (cached primal pass), and the per-chunk products are summed — the data sum of
    ``src/ggn.py:144`` is associative, so this is the single-GPU twin of the multi-GPU shard (``dist.py``).
    The chunks run one after the other on one stream and share ONE probe workspace (``workspace_bytes``); only the
    primal caches are per chunk."""

    def __init__(self, state, Z, model_type, full_set_size=None, example_chunk=64, workspace_bytes=8 << 30,
                 max_probes=1024):
        from .engine import compile_net
        n = Z.shape[0]
        if model_type is not None:
            state.net.model_type = model_type
        sizes = sorted({min(example_chunk, n - s) for s in range(0, n, example_chunk)})
        work_pp = max(compile_net(state.net, m, state.params).work_pp for m in sizes)
        probes = int(max(1, min(max_probes, workspace_bytes // (4 * work_pp))))
        dev = Z.device if Z.is_cuda else torch.device("cuda")
        self.work = torch.empty(work_pp * probes, device=dev, dtype=torch.float32)
        self.engines = [LinearizedNet(state, Z[s:s + example_chunk], model_type, device=dev, work=self.work, max_chunk=probes)
                        for s in range(0, n, example_chunk)]
        N = full_set_size or n
        self.scale = N / n * (math.exp(-_logvar(state)) if model_type == "regressor" else 1.0)
        self.D = self.engines[0].D
        self.engine = self.engines[0]
        self.n = n

    def __call__(self, V, alpha: float = 0.0, out: Optional[torch.Tensor] = None):
        single = V.dim() == 1
        Vb = V[None] if single else V
        Vb = Vb.to(device=self.engines[0].device, dtype=torch.float32).contiguous()
        Y = self.engines[0].ggn_vp(Vb, self.scale, alpha, out=out)
        if len(self.engines) > 1:
            if getattr(self, "_tmp", None) is None or self._tmp.shape != Y.shape:
                self._tmp = torch.empty_like(Y)          # one scratch block for the chunks' partial products, kept
            for eng in self.engines[1:]:
                Y += eng.ggn_vp(Vb, self.scale, 0.0, out=self._tmp)
        return Y[0] if single else Y

    rows = __call__


def materialize_factor(eng: LinearizedNet, c: float = 1.0, block: Optional[int] = None,
                       per_example: bool = True) -> torch.Tensor:
    """Wm (d, D) with rows c * J_i^T L_i e_k — the square-root factor W^T of the GGN (``src/ggn.py:9-93``)
    written out, d = M K.  Row (i, k) depends on example i only: K probes that each hold e_k on EVERY example go
    through one per-example backward sweep (``lip_vjp_rows``) and yield all M K rows — M times less arithmetic than
    pushing the d one-hot cotangents through the summed ``vjp`` (kept as ``per_example=False``; measured at the
    CIFAR config, d = 500: 184 ms -> see DESIGN §4)."""
    d = eng.n * eng.K
    if per_example:
        E = torch.eye(eng.K, device=eng.device, dtype=torch.float32)[:, None, :].expand(eng.K, eng.n, eng.K)
        rows = eng.vjp_rows(E.contiguous(), "l", c)                       # (K, n, D)
        return rows.permute(1, 0, 2).reshape(d, eng.D)
    bs = block or max(1, min(d, (2 << 30) // (4 * eng.D)))
    Wm = torch.empty(d, eng.D, device=eng.device, dtype=torch.float32)
    for s in range(0, d, bs):
        e = min(d, s + bs)
        E = torch.zeros(e - s, d, device=eng.device, dtype=torch.float32)
        E[torch.arange(e - s), torch.arange(s, e)] = 1.0
        Wm[s:e] = eng.vjp(E.reshape(e - s, eng.n, eng.K), "l", c)
    return Wm


def compute_ggn_diag(state, Z, model_type, full_set_size=None, example_chunk: Optional[int] = None, *,
                     curvature=None) -> torch.Tensor:
    """diag((N/M) sum_i J_i^T H_i J_i) (x exp(-logvar) for the regressor) -> (D,) float32 on the device.

    Not a reference function (the reference has no diagonal): the exact GGN diagonal, the curvature of a diagonal
    Laplace posterior and the Jacobi preconditioner of the D-space solves.  K one-hot probes (e_k on every example)
    go through ONE square-accumulating backward sweep (:meth:`LinearizedNet.vjp_sqsum`): diag = recal * sum_k sum_i
    (J_i^T L_i e_k)^2 with the same N/M (x exp(-logvar)) factor as :func:`compute_ggn_vp`, and without the (M K, D)
    factor rows ``(materialize_factor(eng) ** 2).sum(0)`` would write.  ``example_chunk`` binds the examples in chunks
    as :class:`ExampleChunkedGGN` does; the chunks' sums add up in one output vector.  ``curvature`` (a spec of
    ``fisher.py``: ``MCFisher``, ``EmpiricalFisher``, ``Cotangents``) replaces the K one-hot probes by that spec's raw
    cotangents (:func:`fisher.compute_ggn_diag`); ``None`` / ``"ggn"`` is the exact diagonal."""
    if curvature is not None:
        from . import fisher
        spec = fisher.checked(curvature, state, Z, model_type)
        if spec is not None:
            return fisher.compute_ggn_diag(state, Z, model_type, spec, full_set_size=full_set_size, example_chunk=example_chunk)
    M = Z.shape[0]
    N = full_set_size or M
    recal = N / M
    if model_type == "regressor":
        recal *= math.exp(-_logvar(state))
    if example_chunk is None or example_chunk >= M:
        engines = [get_engine(state, Z, model_type)]
    else:
        engines = ExampleChunkedGGN(state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk).engines
    Y = torch.zeros(engines[0].D, device=engines[0].device, dtype=torch.float32)
    for eng in engines:
        E = torch.eye(eng.K, device=eng.device, dtype=torch.float32)[:, None, :].expand(eng.K, eng.n, eng.K)
        eng.vjp_sqsum(E.contiguous(), "l", 1.0, out=Y)
    return Y.mul_(recal)


def compute_ggn_last_layer(state, Z, model_type, full_set_size=None, example_chunk: Optional[int] = None) -> torch.Tensor:
    """The dense GGN block of the final Dense layer, (DL, DL) float64 with DL = (F + 1) K, scaled like
    :func:`compute_ggn_vp` and chunked like :func:`compute_ggn_diag` (:func:`last_layer.compute_ggn_last_layer`)."""
    from . import last_layer
    return last_layer.compute_ggn_last_layer(state, Z, model_type, full_set_size=full_set_size, example_chunk=example_chunk)


def compute_kron_factors_last_layer(state, Z, model_type, example_chunk: Optional[int] = None):
    """``(A (F + 1, F + 1), Bf (K, K), M)``: the Kronecker factors of the last-layer curvature, float64, unscaled
    (:func:`last_layer_kron.compute_kron_factors_last_layer`)."""
    from . import last_layer_kron
    return last_layer_kron.compute_kron_factors_last_layer(state, Z, model_type, example_chunk=example_chunk)


def compute_kfac_factors(state, Z, model_type, example_chunk: Optional[int] = None, *, curvature=None):
    """``(blocks, As, Ss, M)``: the layer blocks of the Kronecker-factored posterior over all layers and their two
    factors per block, float64, unscaled (:func:`kfac.compute_kfac_factors`)."""
    from . import kfac
    return kfac.compute_kfac_factors(state, Z, model_type, example_chunk=example_chunk, curvature=curvature)


def compute_ekfac_scales(state, Z, model_type, bases, example_chunk: Optional[int] = None,
                         class_chunk: Optional[int] = None, *, moments: str = "rows", curvature=None):
    """``[Lam_l (Mt, N)]``: the second moments of the per-example factor rows in the Kronecker eigenbasis
    ``bases[l] = (V_l, Ub_l)`` of every layer block, float64, unscaled (:func:`ekfac.compute_ekfac_scales`);
    ``moments="sweep"`` forms them inside backward sweeps without factor rows and takes a ``curvature`` spec."""
    from . import ekfac
    return ekfac.compute_ekfac_scales(state, Z, model_type, bases, example_chunk=example_chunk, class_chunk=class_chunk,
                                      moments=moments, curvature=curvature)


def compute_ggn_lowrank(state, Z, model_type, rank, prior=None, example_chunk: Optional[int] = None, **solver):
    """``(lam (r,), U (r, D), info)``: the ``rank`` leading eigenpairs of the (prior-whitened) GGN summed over the examples
    of Z at N/M = 1, by randomized block subspace iteration on the GGN-vector product (:func:`lowrank.compute_ggn_lowrank`)."""
    from . import lowrank
    return lowrank.compute_ggn_lowrank(state, Z, model_type, rank, prior=prior, example_chunk=example_chunk, **solver)


def compute_ggn_subnetwork(state, Z, model_type, indices, full_set_size=None, example_chunk: Optional[int] = None) -> torch.Tensor:
    """The dense GGN block over the flat-parameter indices ``indices``, (S, S) float64, scaled like
    :func:`compute_ggn_vp` and chunked like :func:`compute_ggn_diag` (:func:`subnetwork.compute_ggn_subnetwork`)."""
    from . import subnetwork
    return subnetwork.compute_ggn_subnetwork(state, Z, model_type, indices, full_set_size=full_set_size,
                                             example_chunk=example_chunk)


def subnetwork_indices(state, select, size=None, **kw) -> torch.Tensor:
    """The sorted index set of a subnetwork posterior (:func:`subnetwork.subnetwork_indices`)."""
    from . import subnetwork
    return subnetwork.subnetwork_indices(state, select, size, **kw)


FACTOR_BYTES_LIMIT = 64 << 30


def gram_from_factor(Wm: torch.Tensor) -> torch.Tensor:
    """Wm Wm^T (d, d) accumulated in float64: an fp32 Gram of a (d, 1e6) factor carries ~1e-4 * max|G| of rounding
    noise, enough to push the (numerically zero) eigenvalues of W^T W negative.  The long axis is cut into slabs
    that go through ONE batched float64 GEMM each (a single (d, d) product has only (d/128)^2 output tiles — 16 at
    d = 500 — and leaves the chip idle: 176 ms measured; batched: the slab products fill it), then summed."""
    d, D = Wm.shape
    G = torch.zeros(d, d, device=Wm.device, dtype=torch.float64)
    slab = 8192                                              # columns per batch entry
    per_call = max(1, (1 << 30) // (8 * d * slab))           # batch entries per call: <= 1 GiB of float64 operands
    body = (D // slab) * slab
    for c in range(0, body, per_call * slab):
        e = min(body, c + per_call * slab)
        blk = Wm[:, c:e].reshape(d, (e - c) // slab, slab).permute(1, 0, 2).double()      # (B, d, slab)
        G += torch.bmm(blk, blk.transpose(1, 2)).sum(0)
    if body < D:
        tail = Wm[:, body:].double()
        G += tail @ tail.T
    return G


def grouped_grams(Wm: torch.Tensor, prior) -> torch.Tensor:
    """(G, d, d) float64: G_g = Wm[:, S_g] Wm[:, S_g]^T, the Gram of the factor restricted to the columns of group g of a
    :class:`prior.GroupedPrior`.  They do not depend on the precisions: det(A + beta W W^T) = prod_g alpha_g^{D_g} *
    det(I_d + beta sum_g G_g / alpha_g), so the layer-wise evidence and its gradient are d x d algebra after this one
    pass.  One float64-accumulated product per segment on the column slice (``lip_dot_nt_f64`` takes the row stride D);
    the segments partition the columns, so the factor is read once in total; ``.sum(0)`` is :func:`gram_from_factor`."""
    from . import krylov
    d, D = Wm.shape
    if prior.D != D:
        raise ValueError(f"the prior covers {prior.D} parameters, the factor has {D} columns")
    out = torch.zeros(prior.G, d, d, device=Wm.device, dtype=torch.float64)
    for g in range(prior.G):
        for o, n in prior.segments(g):
            blk = Wm[:, o:o + n]
            out[g] += krylov.dot_nt(blk, blk)
    return 0.5 * (out + out.transpose(1, 2))


def compute_ggn_vp(state, Z, model_type, full_set_size=None, mode: str = "matfree"):
    """``src/ggn.py:97-146``: v -> (N/M) sum_i J_i^T H_i J_i v (x exp(-logvar) for the regressor,
    ``:111-113``).

    ``mode="matfree"`` (default, the reference's algorithm): one fused tangent-forward -> output-Hessian ->
    backward sweep per probe block, 8 MACs_fwd FLOP per (example, probe), nothing of size M x D stored.
    ``mode="factor"``: when the factor Wm (d = M K rows of D floats) fits in HBM — the inducing-point regime
    M << N — the GGN is Wm^T Wm and a block matvec is two plain GEMMs, 4 d D FLOP per probe (30x fewer
    than matrix-free at the CIFAR config: d = 500, D = 1.08 M) after a one-off d-row backward sweep.
    ``mode="auto"`` picks "factor" when d * D * 4 B <= 64 GiB."""
    eng = get_engine(state, Z, model_type)
    M = Z.shape[0]
    N = full_set_size or M
    recal_term = N / M
    if model_type == "regressor":
        recal_term *= math.exp(-_logvar(state))
    if mode == "auto":
        mode = "factor" if eng.n * eng.K * eng.D * 4 <= FACTOR_BYTES_LIMIT else "matfree"
    if mode == "matfree":
        return attach_quadratic_forms(BlockOperator(lambda V: eng.ggn_vp(V, recal_term, 0.0), (eng.D,), (eng.D,), eng, "ggn_vp"),
                                      eng, recal_term)
    if mode != "factor":
        raise ValueError("mode must be 'matfree', 'factor' or 'auto'")
    Wm = materialize_factor(eng, math.sqrt(recal_term))

    def apply(V):
        Vb = V.to(device=eng.device, dtype=torch.float32)
        from . import krylov
        Vb = Vb.contiguous()
        U = krylov.gemm_nt(Vb, Wm) if Vb.shape[0] >= 32 else Vb @ Wm.T      # both operands run along D: lip_gemm_nt
        # (P, d)(d, D): the library GEMM (hipBLASLt ~145 TFLOP/s on this shape; the build's own lip_gemm_nn_axpy reaches 86
        # — scripts/sampler_gemm_bench.py — and is kept as an ABI primitive, not on this path)
        return U @ Wm

    op = BlockOperator(apply, (eng.D,), (eng.D,), eng, "ggn_vp[factor]")
    op.factor = Wm
    return op


def compute_W_vps(state, Z, model_type, full_set_size=None, blockwise=False):
    """``src/ggn.py:9-93``: square-root factors  W^T v = sqrt(N/M) [L_i^T J_i v]_i  (M, K)
    and  W U = sqrt(N/M) sum_i J_i^T L_i U_i  (D,);  regressor: L = exp(-logvar/2), outputs squeezed
    to (M,) as the reference does (``:58``)."""
    eng = get_engine(state, Z, model_type)
    M = Z.shape[0]
    N = full_set_size or M
    c = math.sqrt(N / M)
    if model_type == "regressor":
        c *= math.exp(-0.5 * _logvar(state))
    K = eng.K
    inner = (M,) if (model_type == "regressor" and K == 1) else (M, K)

    def WT_block(V):
        return eng.jvp(V, "lt", c).reshape((V.shape[0],) + inner)

    def W_block(U):
        return eng.vjp(U.reshape(U.shape[0], M, K), "l", c)

    WTfun = BlockOperator(WT_block, (eng.D,), inner, eng, "WTfun")
    Wfun = BlockOperator(W_block, inner, (eng.D,), eng, "Wfun")
    Wfun.factor_scale = WTfun.factor_scale = c          # lets build_WTW form factor columns per example (lip_vjp_rows)
    if not blockwise:
        return Wfun, WTfun

    kshape = () if inner == (M,) else (K,)

    def WT_point(i, v):                      # (D,) -> (K,)     src/ggn.py:55-62
        return WTfun(v)[..., i] if inner == (M,) else WTfun(v)[..., i, :]

    def W_point(i, U_i):                     # (K,) -> (D,)     src/ggn.py:64-76
        U_i = torch.as_tensor(U_i, device=eng.device, dtype=torch.float32)
        batch = U_i.shape[:U_i.dim() - len(kshape)]
        U = torch.zeros(tuple(batch) + inner, device=eng.device, dtype=torch.float32)
        if inner == (M,):
            U[..., i] = U_i
        else:
            U[..., i, :] = U_i
        return Wfun(U)

    return W_point, WT_point


def compute_ggn_dense(state, Z, model_type, full_set_size=None, block: int = 256):
    """``src/ggn.py:149-193``: the dense GGN, returned as ``(GGN, flat_params, unravel_fn)``.  Built by
    applying the matrix-free operator to identity blocks (toy sizes only: D^2 floats)."""
    flat_params, unravel_fn = flatten_nn_params(state.params)
    vp = compute_ggn_vp(state, Z, model_type, full_set_size=full_set_size)
    eng = vp.engine
    D = eng.D
    GGN = torch.empty(D, D, device=eng.device, dtype=torch.float32)
    for s in range(0, D, block):
        e = min(D, s + block)
        I = torch.zeros(e - s, D, device=eng.device, dtype=torch.float32)
        I[torch.arange(e - s), torch.arange(s, e)] = 1.0
        GGN[s:e] = vp(I)                       # rows of a symmetric matrix
    return GGN, flat_params.to(eng.device), unravel_fn


def _apply_block(fun, E):
    return fun.rows(E) if isinstance(fun, BlockOperator) else torch.stack([fun(e) for e in E])


def build_WTW(W, WT, inner_shape, d, *, dtype=torch.float32, block=64, factor_bytes_limit=8 << 30):
    """``src/ggn.py:198-227``: dense W^T W (d, d), symmetrised through its upper triangle (``:227``).

    ``block`` only bounds peak memory in the reference (column blocks under ``jax.remat``); here it is a
    lower bound on the batch handed to the engine — the result does not depend on it.  When W and W^T
    come from one engine the Gram is formed as  Wm Wm^T  from the materialised factor Wm = W(I_d)
    (d engine rows + one plain GEMM) instead of d x (W then W^T) network sweeps."""
    inner_shape = tuple(inner_shape)
    if isinstance(W, BlockOperator) and W.engine is not None:
        dev = W.engine.device
        D = W.engine.D
        bs = max(int(block), min(d, max(1, (4 << 30) // (4 * D))))
        c, M, K = getattr(W, "factor_scale", None), W.engine.n, W.engine.K
        if d * D * 4 <= factor_bytes_limit:
            Wm = torch.empty(d, D, device=dev, dtype=torch.float32)
            for s in range(0, d, bs):
                e = min(d, s + bs)
                E = torch.zeros(e - s, d, device=dev, dtype=torch.float32)
                E[torch.arange(e - s), torch.arange(s, e)] = 1.0
                Wm[s:e] = W.rows(E.reshape((e - s,) + inner_shape))
            WTW = gram_from_factor(Wm)
        elif c is not None and d == M * K and M > 1:
            # the factor does not fit: stream column blocks, W then W^T.  Column (i, k) of W depends on example i only, so
            # a probe holding e_k on EVERY example yields its M columns in one per-example backward sweep
            # (lip_vjp_rows) — the summed vjp of d one-hot cotangents pushes M - 1 zero cotangents per row through the
            # network (ResNet-50, 2 inducing images, d = 2000: 2.08 -> 1.78 s; the saving grows with M)
            WTW = torch.empty(d, d, device=dev, dtype=torch.float32)
            pb = max(1, bs // M)
            eyeK = torch.eye(K, device=dev, dtype=torch.float32)
            for k0 in range(0, K, pb):
                k1 = min(K, k0 + pb)
                U = eyeK[k0:k1, None, :].expand(k1 - k0, M, K).contiguous()
                cols = W.engine.vjp_rows(U, "l", c).reshape((k1 - k0) * M, D)           # row (j, i) = column (i, k0 + j) of W
                G = WT.rows(cols).reshape(k1 - k0, M, d)
                WTW.view(d, M, K)[:, :, k0:k1] = G.permute(2, 1, 0)
        else:
            WTW = torch.empty(d, d, device=dev, dtype=torch.float32)
            for s in range(0, d, bs):
                e = min(d, s + bs)
                E = torch.zeros(e - s, d, device=dev, dtype=torch.float32)
                E[torch.arange(e - s), torch.arange(s, e)] = 1.0
                WTW[:, s:e] = WT.rows(W.rows(E.reshape((e - s,) + inner_shape))).reshape(e - s, d).T
    else:
        cols = []
        for j in range(d):
            e = torch.zeros(d, dtype=dtype)
            e[j] = 1.0
            cols.append(WT(W(e.reshape(inner_shape))).reshape(-1))
        WTW = torch.stack(cols, dim=1)
    WTW = torch.triu(WTW) + torch.triu(WTW, 1).T
    return WTW.to(dtype)


def build_WTWz(WT, W_z, inner_shape_z, *, d, dtype=torch.float32, block=64):
    """``src/ggn.py:233-272``: cross-Gram W^T W_z (d, d_z)."""
    inner_shape_z = tuple(inner_shape_z)
    d_z = math.prod(inner_shape_z)
    if isinstance(W_z, BlockOperator) and W_z.engine is not None:
        dev = W_z.engine.device
        D = W_z.engine.D
        bs = max(int(block), min(d_z, max(1, (1 << 30) // (4 * D))))
        G = torch.empty(d, d_z, device=dev, dtype=torch.float32)
        for s in range(0, d_z, bs):
            e = min(d_z, s + bs)
            E = torch.zeros(e - s, d_z, device=dev, dtype=torch.float32)
            E[torch.arange(e - s), torch.arange(s, e)] = 1.0
            G[:, s:e] = _apply_block(WT, W_z.rows(E.reshape((e - s,) + inner_shape_z))).reshape(e - s, d).T
        return G.to(dtype)
    cols = []
    for j in range(d_z):
        e = torch.zeros(d_z, dtype=dtype)
        e[j] = 1.0
        cols.append(WT(W_z(e.reshape(inner_shape_z))).reshape(-1))
    return torch.stack(cols, dim=1).to(dtype)


def ensure_symmetry(M, jitter=1e-8):
    """``src/ggn.py:277-278``."""
    return 0.5 * (M + M.T) + jitter * torch.eye(M.shape[0], dtype=M.dtype, device=M.device)
