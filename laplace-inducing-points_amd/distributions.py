"""Minimal stand-in for ``tfp.distributions.MultivariateNormalFullCovariance`` — the object
``posterior_lla_dense`` / ``predict_lla_dense`` return in the reference
(``src/lla.py:42-45,79-82``).  Only the members its callers use exist:
``.mean() .covariance() .stddev() .sample(seed=, sample_shape=)``
(``tests/test_lla.py:21,24``, ``tests/test_sample.py:478-479``).
Supports a batch of distributions: loc (..., k), covariance (..., k, k).

``MultivariateNormalDiag`` (not in the reference) is the diagonal-covariance twin that ``posterior_lla_diag`` returns:
``.mean() .variance() .stddev() .sample(sample_shape, seed)`` and no (k, k) ``covariance()``, which would not fit at
the sizes a diagonal posterior is used for.
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
