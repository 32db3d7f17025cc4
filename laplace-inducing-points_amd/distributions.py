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
