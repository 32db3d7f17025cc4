"""Float64 / integer yardstick of the Fisher fits (``lip_amd.fisher``) — TEST INFRASTRUCTURE (a plain helper module):
CPU torch and numpy only, no product code on its path.

* :func:`replay_labels` / :func:`replay` — the definition of ``lip_head_sample`` in Python integers: q_k =
  floor(p_k 2^40), prefix sums, Philox4x32-10 at counter (s << 32) | g keyed by the seed, t = mulhi64(w1:w0, Q), the first
  class whose prefix exceeds t; U = float32(onehot) - p in one float32 subtraction.
* :func:`diag_ref`, :func:`kfac_output_factors_ref` — the curvature of given raw cotangents:
  diag = recal / divisor sum_p sum_i (J_i^T u_pi)^2, S_l = 1 / divisor sum_p sum_i sum_t g g^T.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from krylov_harness import _lib_words

SHIFT = 40


def quantise(p_row) -> list:
    """[q_k] Python integers: floor(float64(p_k) 2^40); all 0 for a row with an entry outside [0, 1] (NaN included)"""
    row = np.asarray(p_row, dtype=np.float32).astype(np.float64).tolist()
    if not all(0.0 <= v <= 1.0 for v in row):
        return [0] * len(row)
    return [int(math.floor(v * 2.0 ** SHIFT)) for v in row]


def replay_labels(probs, S: int, seed: int, example_offset: int = 0) -> np.ndarray:
    """(S, n) int32 labels of the definition; -1 on a row whose quantised sum is 0"""
    probs = np.asarray(probs, dtype=np.float32)
    n, K = probs.shape
    labels = np.empty((S, n), dtype=np.int32)
    s_idx = np.arange(S, dtype=np.uint64)
    for i in range(n):
        q = quantise(probs[i])
        pre, acc = [], 0
        for v in q:
            acc += v
            pre.append(acc)
        Q = acc
        if Q == 0:
            labels[:, i] = -1
            continue
        g = int(example_offset) + i
        assert 0 <= g < 2 ** 32
        w = _lib_words((s_idx << np.uint64(32)) | np.uint64(g), seed)
        pre_arr = np.array(pre, dtype=object)
        for s in range(S):
            r = (int(w[1][s]) << 32) | int(w[0][s])
            t = (r * Q) >> 64
            lo, hi = 0, K - 1                       # min{k : pre_k > t}
            while lo < hi:
                mid = (lo + hi) // 2
                if pre_arr[mid] > t:
                    hi = mid
                else:
                    lo = mid + 1
            labels[s, i] = lo
    return labels


def cotangents_from_labels(probs, labels) -> np.ndarray:
    """(S, n, K) float32: onehot(label) - p, one float32 subtraction per entry (label -1: -p)"""
    probs = np.asarray(probs, dtype=np.float32)
    S, n = labels.shape
    K = probs.shape[1]
    hot = (np.arange(K, dtype=np.int64)[None, None, :] == labels[:, :, None]).astype(np.float32)
    return hot - probs[None]


def replay(probs, S: int, seed: int, example_offset: int = 0):
    labels = replay_labels(probs, S, seed, example_offset)
    return cotangents_from_labels(probs, labels), labels


# ------------------------------------------------------------------------------------------------ curvature
def diag_ref(state, Z, model_type, U, divisor, N, J=None) -> torch.Tensor:
    """(D,) float64: recal / divisor sum_p sum_i (J_i^T u_pi)^2 for raw cotangents U (P, M, K); J (M, K, D) is the
    autograd Jacobian of ``last_layer_ref.jac64`` (pass it to share one among several calls)"""
    import last_layer_ref as ref
    if J is None:
        _, J = ref.jac64(state, Z, model_type)
    U = torch.as_tensor(np.asarray(U), dtype=torch.float64).reshape(-1, J.shape[0], J.shape[1])
    rows = torch.einsum("pik,ikd->pid", U, J)
    return ref.recal(state, Z.shape[0], model_type, N) / float(divisor) * (rows * rows).sum((0, 1))


def kfac_output_factors_ref(state, Z, U, divisor, Gs=None):
    """[S_l (N, N)] float64, uncentred and unscaled: 1 / divisor sum_p sum_i sum_t (G_it u_pi)(G_it u_pi)^T with
    G_it[:, k] = dF_k / dz_{i,t} of ``kfac_ref.patches_and_cotangents`` (pass its third result as ``Gs`` to share it)"""
    import kfac_ref
    if Gs is None:
        _, _, Gs = kfac_ref.patches_and_cotangents(state, Z)
    U = torch.as_tensor(np.asarray(U), dtype=torch.float64)
    out = []
    for G in Gs:                                              # (n, K, T, N)
        g = torch.einsum("pik,iktn->pitn", U.reshape(-1, G.shape[0], G.shape[1]), G)
        out.append(torch.einsum("pitn,pitm->nm", g, g) / float(divisor))
    return out


def exact_expectation_cotangents(p) -> torch.Tensor:
    """(K, n, K) float64: U[k, i] = sqrt(p_ik) (e_k - p_i), whose outer products sum to diag(p_i) - p_i p_i^T"""
    p = torch.as_tensor(p, dtype=torch.float64)
    n, K = p.shape
    E = torch.eye(K, dtype=torch.float64)[:, None, :] - p[None]
    return p.T.sqrt()[:, :, None] * E
