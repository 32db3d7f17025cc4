"""Minimal stand-in for ``tfp.distributions.MultivariateNormalFullCovariance`` — the object
``posterior_lla_dense`` / ``predict_lla_dense`` return in the reference
(``src/lla.py:42-45,79-82``).  Only the members its callers use exist:
``.mean() .covariance() .stddev() .sample(seed=, sample_shape=)``
(``tests/test_lla.py:21,24``, ``tests/test_sample.py:478-479``).
Supports a batch of distributions: loc (..., k), covariance (..., k, k).

``MultivariateNormalDiag`` (not in the reference) is the diagonal-covariance twin that ``posterior_lla_diag`` returns:
``.mean() .variance() .stddev() .sample(sample_shape, seed)`` and no (k, k) ``covariance()``, which would not fit at
the sizes a diagonal posterior is used for.

``KroneckerNormal`` (not in the reference) is the factored Gaussian that ``posterior_lla_last_layer_kron`` returns.

``KFACNormal`` (not in the reference) is the Gaussian over the whole flat vector that ``posterior_lla_kfac`` returns: one
``KroneckerNormal`` per layer block and independent variances for the parameters outside every block.

``LowRankNormal`` (not in the reference) is the Gaussian over the whole flat vector that ``posterior_lla_lowrank``
returns: the prior plus the leading eigenpairs of the whitened GGN in the precision, every other direction at the prior
variance.
"""
from __future__ import annotations

import torch


class MultivariateNormalFullCovariance:
    def __init__(self, loc: torch.Tensor, covariance_matrix: torch.Tensor):
        self.loc = loc
        self.covariance_matrix = covariance_matrix

    def mean(self) -> torch.Tensor:
        return self.loc

    def covariance(self) -> torch.Tensor:
        return self.covariance_matrix

    def variance(self) -> torch.Tensor:
        return torch.diagonal(self.covariance_matrix, dim1=-2, dim2=-1)

    def stddev(self) -> torch.Tensor:
        return torch.sqrt(self.variance())

    def sample(self, sample_shape=(), seed=None) -> torch.Tensor:
        if isinstance(sample_shape, int):
            sample_shape = (sample_shape,)
        g = None
        if seed is not None:
            g = torch.Generator(device=self.loc.device).manual_seed(int(seed))
        cov = self.covariance_matrix
        L = torch.linalg.cholesky(0.5 * (cov + cov.transpose(-1, -2)))
        eps = torch.randn(tuple(sample_shape) + tuple(self.loc.shape), dtype=self.loc.dtype,
                          device=self.loc.device, generator=g)
        return self.loc + (L @ eps.unsqueeze(-1)).squeeze(-1)


class MultivariateNormalDiag:
    """N(loc, diag(variance)); give ``variance`` or ``scale_diag`` (its square root), shapes (..., k) like loc."""

    def __init__(self, loc: torch.Tensor, scale_diag: torch.Tensor = None, variance: torch.Tensor = None):
        if (scale_diag is None) == (variance is None):
            raise ValueError("give exactly one of scale_diag and variance")
        self.loc = loc
        self._var = variance if variance is not None else scale_diag * scale_diag
        if self._var.shape[-1] != loc.shape[-1]:
            raise ValueError(f"variance {tuple(self._var.shape)} does not match loc {tuple(loc.shape)}")

    def mean(self) -> torch.Tensor:
        return self.loc

    def variance(self) -> torch.Tensor:
        return self._var

    def stddev(self) -> torch.Tensor:
        return torch.sqrt(self._var)

    def sample(self, sample_shape=(), seed=None) -> torch.Tensor:
        if isinstance(sample_shape, int):
            sample_shape = (sample_shape,)
        g = None
        if seed is not None:
            g = torch.Generator(device=self.loc.device).manual_seed(int(seed))
        shape = tuple(sample_shape) + tuple(torch.broadcast_shapes(self.loc.shape, self._var.shape))
        eps = torch.randn(shape, dtype=self.loc.dtype, device=self.loc.device, generator=g)
        return self.loc + self.stddev() * eps


class KroneckerNormal:
    """N(loc, S) over a (Ft, K) block flattened row-major (index f K + k), with the covariance in factored form
    S[(f,k)][(g,m)] = sum_{j,l} V[f][j] V[g][j] Ub[k][l] Ub[m][l] R[j][l]; V (Ft, Ft), R (Ft, K) positive, Ub (K, K),
    loc (Ft K,).  ``spectrum`` = (lam (Ft,), mu (K,), c) with R = 1 / (c lam mu^T + 1), when known, keeps the
    log-determinant free of the cancellation in log R."""
    def __init__(self, loc: torch.Tensor, V: torch.Tensor, R: torch.Tensor, Ub: torch.Tensor, spectrum=None):
        Ft, K = R.shape
        if tuple(V.shape) != (Ft, Ft) or tuple(Ub.shape) != (K, K) or loc.shape[-1] != Ft * K:
            raise ValueError(f"V {tuple(V.shape)}, R {tuple(R.shape)}, Ub {tuple(Ub.shape)} and loc {tuple(loc.shape)} do "
                             f"not describe one ({Ft}, {K}) block")
        self.loc, self.V, self.R, self.Ub, self.spectrum = loc, V, R, Ub, spectrum

    def mean(self) -> torch.Tensor:
        return self.loc

    def variance(self) -> torch.Tensor:
        return ((self.V * self.V) @ self.R @ (self.Ub * self.Ub).T).reshape(-1)

    def stddev(self) -> torch.Tensor:
        return torch.sqrt(self.variance())

    def covariance(self) -> torch.Tensor:
        from .last_layer import LAST_LAYER_MAX_DIM
        Ft, K = self.R.shape
        if Ft * K > LAST_LAYER_MAX_DIM:
            raise ValueError(f"a dense {Ft * K} x {Ft * K} covariance is not built (more than LAST_LAYER_MAX_DIM = "
                             f"{LAST_LAYER_MAX_DIM} parameters): use variance(), sample() or the factors V, R, Ub")
        W = torch.kron(self.V, self.Ub)
        return (W * self.R.reshape(-1)[None, :]) @ W.T

    def log_det_precision_ratio(self) -> torch.Tensor:
        """log det(prior^-1 posterior precision) = -sum log R = sum log1p(c lam mu)"""
        if self.spectrum is not None:
            lam, mu, c = self.spectrum
            return torch.log1p(c * lam[:, None] * mu[None, :]).sum()
        return -torch.log(self.R).sum()

    def sample(self, sample_shape=(), seed=None) -> torch.Tensor:
        """loc + vec(V (E o sqrt(R)) Ub^T), E standard normal of shape sample_shape + (Ft, K)"""
        if isinstance(sample_shape, int):
            sample_shape = (sample_shape,)
        g = None
        if seed is not None:
            g = torch.Generator(device=self.loc.device).manual_seed(int(seed))
        Ft, K = self.R.shape
        E = torch.randn(tuple(sample_shape) + (Ft, K), dtype=self.loc.dtype, device=self.loc.device, generator=g)
        dW = self.V @ (E * torch.sqrt(self.R)) @ self.Ub.T
        return self.loc + dW.reshape(tuple(sample_shape) + (Ft * K,))


class KFACNormal:
    """N(loc, S) over the whole flat parameter vector (D,), S block-diagonal: ``blocks`` is a list of
    ``(offset, KroneckerNormal)`` whose (Mt, N) blocks are the contiguous slices loc[offset : offset + Mt N], and
    ``remainder`` = ``(indices, variance)`` gives every other parameter an independent variance.  Blocks and remainder
    must cover [0, D) exactly once.  ``remainder_prior`` (the prior precisions of the remainder, or one number), when
    given, lets :meth:`log_det_precision_ratio` include the remainder's term."""

    def __init__(self, loc: torch.Tensor, blocks, remainder, remainder_prior=None):
        idx, var = remainder
        idx = torch.as_tensor(idx, dtype=torch.int64, device=loc.device).reshape(-1)
        var = torch.as_tensor(var, device=loc.device).reshape(-1)
        if idx.numel() != var.numel():
            raise ValueError(f"the remainder has {idx.numel()} indices and {var.numel()} variances")
        seen = torch.zeros(loc.shape[-1], dtype=torch.int64)
        for off, kn in blocks:
            Mt, N = kn.R.shape
            if off < 0 or off + Mt * N > loc.shape[-1]:
                raise ValueError(f"the ({Mt}, {N}) block at offset {off} does not lie in [0, {loc.shape[-1]})")
            seen[off:off + Mt * N] += 1
        seen.index_add_(0, idx.cpu(), torch.ones(idx.numel(), dtype=torch.int64))       # counts a repeated index twice
        if not bool((seen == 1).all()):
            raise ValueError("the blocks and the remainder must cover every parameter exactly once")
        self.loc, self.blocks, self.remainder, self.remainder_prior = loc, list(blocks), (idx, var), remainder_prior

    def mean(self) -> torch.Tensor:
        return self.loc

    def variance(self) -> torch.Tensor:
        idx, var = self.remainder
        out = torch.empty_like(self.loc)
        for off, kn in self.blocks:
            v = kn.variance()
            out[off:off + v.numel()] = v.to(out.dtype)
        out[idx] = var.to(out.dtype)
        return out

    def stddev(self) -> torch.Tensor:
        return torch.sqrt(self.variance())

    def log_det_precision_ratio(self) -> torch.Tensor:
        """log det(prior^-1 posterior precision): the blocks' sums and -sum log(a_d var_d) over the remainder"""
        idx, var = self.remainder
        total = sum((kn.log_det_precision_ratio() for _, kn in self.blocks), torch.zeros((), dtype=torch.float64, device=self.loc.device))
        if idx.numel():
            if self.remainder_prior is None:
                raise ValueError("the remainder's prior precisions are not known (remainder_prior)")
            a = torch.as_tensor(self.remainder_prior, dtype=torch.float64, device=var.device)
            total = total - torch.log(a * var.double()).sum()
        return total

    def sample(self, sample_shape=(), seed=None, dtype=torch.float32) -> torch.Tensor:
        """draws (sample_shape + (D,)) of ``dtype``: every block through :meth:`KroneckerNormal.sample` (block l seeded
        ``seed + l``), the remainder loc + sqrt(var) E (seeded ``seed + number of blocks``)"""
        if isinstance(sample_shape, int):
            sample_shape = (sample_shape,)
        shape = tuple(sample_shape)
        out = torch.empty(shape + (self.loc.shape[-1],), dtype=dtype, device=self.loc.device)
        for l, (off, kn) in enumerate(self.blocks):
            x = kn.sample(shape, seed=None if seed is None else int(seed) + l)
            out[..., off:off + x.shape[-1]] = x.to(dtype)
        idx, var = self.remainder
        if idx.numel():
            g = None
            if seed is not None:
                g = torch.Generator(device=self.loc.device).manual_seed(int(seed) + len(self.blocks))
            E = torch.randn(shape + (idx.numel(),), dtype=var.dtype, device=var.device, generator=g)
            out[..., idx] = (self.loc[idx].to(var.dtype) + torch.sqrt(var) * E).to(dtype)
        return out


class LowRankNormal:
    """N(loc, S) over the whole flat parameter vector (D,) with a diagonal-plus-low-rank precision: with the prior
    A0 = alpha I or diag(a), orthonormal rows ``Ut`` (r, D) and whitened eigenvalues ``lam_t`` (r,) >= 0 (the leading
    eigenpairs of A0^(-1/2) G A0^(-1/2); for a scalar prior recal lam / alpha with the eigenvectors of G itself),

        S^-1 = A0^(1/2) (I + Ut^T diag(lam_t) Ut) A0^(1/2),
        S    = A0^(-1/2) (I - Ut^T diag(s) Ut) A0^(-1/2),    s_j = lam_t_j / (1 + lam_t_j).

    Every direction outside span(Ut) keeps the prior variance, so truncating the spectrum over-states the variance: it
    never under-states it relative to the posterior that more of the same Ritz pairs would give, because every further
    pair only subtracts a positive semi-definite term.

    ``prior`` is a number (alpha) or a (D,) vector of precisions.  On CUDA ``Ut`` is float32 and the (r, D) passes are the
    HIP primitives of ``krylov.py``: ``cols_wsqsum`` for the marginal variance, ``dot_nt`` / ``gemm_nt`` and
    ``gemm_nn_axpy`` / ``rows_combine`` for the draws and the covariance products.  CPU tensors (float64 in the tests)
    run the same algebra in plain torch."""

    STIFF = 250.0          # sqrt(1 + lam_t) above which a draw's coefficient is accumulated in float64 (``sample.py``)

    def __init__(self, loc: torch.Tensor, Ut: torch.Tensor, lam_t: torch.Tensor, prior):
        D = loc.shape[-1]
        if Ut.dim() != 2 or Ut.shape[1] != D or lam_t.shape != (Ut.shape[0],):
            raise ValueError(f"Ut {tuple(Ut.shape)}, lam_t {tuple(lam_t.shape)} and loc {tuple(loc.shape)} do not describe "
                             f"r eigenpairs over {D} parameters")
        self.loc, self.Ut = loc, Ut
        self.lam_t = lam_t.to(device=loc.device, dtype=torch.float64).clamp_min(0.0)
        if torch.is_tensor(prior) and prior.dim() > 0:
            if prior.numel() != D:
                raise ValueError(f"the prior holds {prior.numel()} precisions for {D} parameters")
            self.a = prior.to(device=loc.device, dtype=torch.float64).reshape(-1)
            if not bool((self.a > 0).all()):
                raise ValueError("the prior precisions must be positive")
            self.isq = self.a.rsqrt().to(Ut.dtype)
        else:
            self.a = float(prior)
            if not self.a > 0:
                raise ValueError("the prior precision must be positive")
            self.isq = self.a ** -0.5
        self.s = self.lam_t / (1.0 + self.lam_t)
        root = torch.sqrt(1.0 + self.lam_t)
        self.g = -self.lam_t / (root * (1.0 + root))        # (1 + lam_t)^(-1/2) - 1 without the cancellation
        self.n_stiff = int(min(96, int((root > self.STIFF).sum())))      # lam_t descends: the stiff rows come first

    def _hip(self) -> bool:
        return self.Ut.is_cuda and self.Ut.dtype == torch.float32

    def mean(self) -> torch.Tensor:
        return self.loc

    def spectrum(self) -> torch.Tensor:
        """the whitened eigenvalues lam_t (r,), float64: the posterior precision is A0^(1/2) (I + Ut^T diag(lam_t) Ut) A0^(1/2)"""
        return self.lam_t

    def log_det_precision_ratio(self) -> torch.Tensor:
        """log det(prior^-1 posterior precision) = sum_j log1p(lam_t_j)"""
        return torch.log1p(self.lam_t).sum()

    def variance(self) -> torch.Tensor:
        """diag(S)_d = (1 - sum_j s_j Ut[j, d]^2) / a_d, (D,) float64 (``lip_cols_wsqsum`` on float32 device rows: one read
        of Ut, no (r, D) temporary)"""
        if self.Ut.shape[0] == 0:
            q = torch.zeros_like(self.loc, dtype=torch.float64)
        elif self._hip():
            from . import krylov
            q = krylov.cols_wsqsum(self.Ut, self.s)
        else:
            q = (self.s[:, None] * self.Ut.double() ** 2).sum(0)
        return (1.0 - q) / self.a

    def stddev(self) -> torch.Tensor:
        return torch.sqrt(self.variance())

    def _combine(self, X: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
        """X + (C o coef) Ut with C = X Ut^T, for rows X (P, D) of Ut's dtype; X is overwritten where the kernels allow"""
        if self.Ut.shape[0] == 0:
            return X
        if not self._hip():
            return X + ((X @ self.Ut.T) * coef.to(X.dtype)) @ self.Ut
        from . import krylov
        X = X.contiguous()
        if X.shape[0] < 32:
            C = krylov.dot_nt(X, self.Ut)
        else:
            C = krylov.gemm_nt(X, self.Ut).double()
            if self.n_stiff:
                C[:, :self.n_stiff] = krylov.dot_nt(X, self.Ut[:self.n_stiff])
        return krylov.gemm_nn_axpy((C * coef).float().contiguous(), self.Ut, X, 1.0, out=X)

    def cov_vp(self, V: torch.Tensor) -> torch.Tensor:
        """S V for a vector (D,) or the rows of a block (P, D), in Ut's dtype"""
        single = V.dim() == 1
        X = (V[None] if single else V).to(device=self.Ut.device, dtype=self.Ut.dtype) * self.isq
        out = self._combine(X, -self.s) * self.isq
        return out[0] if single else out

    def sample_map(self, eps: torch.Tensor) -> torch.Tensor:
        """the exact linear map of the draws, rows eps (S, D) -> A0^(-1/2) (eps + Ut^T (g o (Ut eps))), whose covariance
        under standard-normal eps is S: (I + Ut^T diag(g) Ut)^2 = I - Ut^T diag(s) Ut.  ``eps`` may be overwritten."""
        return self._combine(eps, self.g) * self.isq

    def sample(self, sample_shape=(), seed=None, dtype=None) -> torch.Tensor:
        """draws (sample_shape + (D,)): loc + A0^(-1/2) (eps + Ut^T (g o (Ut eps))), g_j = -lam_t_j / (sqrt(1 + lam_t_j)
        (1 + sqrt(1 + lam_t_j))); two passes over Ut per block of draws.  On the device eps is ``fill_normal(seed)`` and
        the draws are float32 unless ``dtype`` says otherwise; on the CPU a seeded torch generator in Ut's dtype."""
        if isinstance(sample_shape, int):
            sample_shape = (sample_shape,)
        shape = tuple(sample_shape)
        S = 1
        for n in shape:
            S *= int(n)
        D = self.loc.shape[-1]
        if self._hip():
            from . import krylov
            eps = krylov.fill_normal(S, D, 0 if seed is None else int(seed), device=self.Ut.device)
        else:
            g = None
            if seed is not None:
                g = torch.Generator(device=self.Ut.device).manual_seed(int(seed))
            eps = torch.randn(S, D, dtype=self.Ut.dtype, device=self.Ut.device, generator=g)
        dtype = dtype or eps.dtype
        return (self.loc.to(dtype) + self.sample_map(eps).to(dtype)).reshape(shape + (D,))
