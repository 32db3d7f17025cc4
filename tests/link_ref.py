"""Float64 replay of the Monte-Carlo softmax link (``lip_link_mc``) and of the semidefinite Cholesky factor
(``lip_link_chol``), written from their definitions in include/lip.h; numpy only, no product code on its path.

* :func:`normals` — Philox4x32-10 (``krylov_harness.philox4x32``) at the counter words (g, s, k >> 2, 0x4C4E4B31), keyed by
  the two words of the seed; word pairs (0, 1) and (2, 3) give (rad cos, rad sin) with u = ((w >> 8) + 0.5) / 2^24 formed in
  float32 as the kernel forms it and the angle 2 pi u2 rounded to float32 as well (both as ``krylov_harness.ref_normal``);
  logarithm, square root, sine and cosine in float64.
* :func:`cholesky_semidefinite` — the column rule: tol = 2^-20 max_i C_ii, d_j = C_jj - sum_{k<j} L_jk^2, a column with
  d_j > tol is scaled by 1 / sqrt(d_j), any other is zero; dead on a non-finite lower-triangle entry or a C_ii < -tol.
* :func:`replay` — z = mean + sd eps or mean + L eps, float64 softmax, averages over the draws, entropies.
* :func:`sigmoid_expectation` — E[sigmoid(z)], z ~ N(mu, s2), by Gauss-Hermite quadrature (96 nodes).
"""
import numpy as np

import krylov_harness as kh

LINK_TAG = 0x4C4E4B31
HEAD_TAG = 0xBB67AE85              # lip_head_sample's fourth counter word


def first_words(g, s, seed, c2=0, tag=LINK_TAG):
    """Philox words (4 arrays) at the counter (g, s, c2, tag)"""
    seed = int(seed) & (2 ** 64 - 1)
    return kh.philox4x32([g, s, c2, tag], [seed & 0xFFFFFFFF, seed >> 32])


def normals(n, K, S, seed, example_offset=0):
    """eps (n, S, K) float64: the standard normals of the link"""
    Q = (K + 3) // 4
    g = (example_offset + np.arange(n, dtype=np.uint64)).reshape(n, 1, 1)
    s = np.arange(S, dtype=np.uint64).reshape(1, S, 1)
    q = np.arange(Q, dtype=np.uint64).reshape(1, 1, Q)
    g, s, q = (np.broadcast_to(x, (n, S, Q)).reshape(-1) for x in (g, s, q))
    w = first_words(g, s, seed, c2=q)
    f32 = np.float32
    u = [((x >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0) for x in w]
    out = np.empty((n * S * Q, 4))
    for hh in range(2):
        r = np.sqrt(-2.0 * np.log(u[2 * hh].astype(np.float64)))
        ang = (f32(6.283185307179586) * u[2 * hh + 1]).astype(np.float64)
        out[:, 2 * hh], out[:, 2 * hh + 1] = r * np.cos(ang), r * np.sin(ang)
    return out.reshape(n, S, 4 * Q)[:, :, :K]


def cholesky_semidefinite(C):
    """one (K, K) float64 matrix -> (L (K, K) float64, dead flag)"""
    C = np.asarray(C, dtype=np.float64)
    K = C.shape[0]
    L = np.zeros((K, K))
    low = C[np.tril_indices(K)]
    if not np.isfinite(low).all():
        return L, 1
    tol = 2.0 ** -20 * np.max(np.diag(C))
    if (np.diag(C) < -tol).any():
        return L, 1
    for j in range(K):
        d = C[j, j] - np.sum(L[j, :j] ** 2)
        if d > tol:
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, K):
                L[i, j] = (C[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return L, 0


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(-1)


def draws(mean, var=None, L=None, S=1, seed=0, example_offset=0):
    """per-draw probabilities (n, S, K) float64"""
    mean = np.asarray(mean, dtype=np.float64)
    n, K = mean.shape
    eps = normals(n, K, S, seed, example_offset)
    if L is None:
        z = mean[:, None, :] + np.sqrt(np.asarray(var, dtype=np.float64))[:, None, :] * eps
    else:
        z = mean[:, None, :] + np.einsum("nkj,nsj->nsk", np.tril(np.asarray(L, dtype=np.float64)), eps)
    return softmax(z)


def replay(mean, var=None, L=None, S=1, seed=0, example_offset=0, return_draws=False):
    """(probs (n, K), mean_entropy (n,)) float64 [, the per-draw probabilities]"""
    p = draws(mean, var, L, S, seed, example_offset)
    out = (p.mean(1), entropy(p).mean(1))
    return out + (p,) if return_draws else out


def sigmoid_expectation(mu, s2, nodes=96):
    """E[1 / (1 + exp(-z))], z ~ N(mu, s2): Gauss-Hermite (physicists') quadrature"""
    x, w = np.polynomial.hermite.hermgauss(nodes)
    z = mu + np.sqrt(2.0 * s2) * x
    return float(np.sum(w / (1.0 + np.exp(-z))) / np.sqrt(np.pi))
