"""CPU: the definition of the head sampler pinned by known answers of its integer replay (``fisher_ref``), the band of
its frequencies, the unbiasedness of the Monte-Carlo Fisher for the head Hessian, and the validation of the curvature
specs of ``lip_amd.fisher`` (no GPU work)."""
import math

import numpy as np
import pytest
import torch

import fisher_ref as fr
from lip_amd import fisher

ROWS = np.array([[0.5, 0.25, 0.0, 0.125, 0.125], [0.0, 0.0, 1.0, 0.0, 0.0], [0.0625] * 4 + [0.75]], dtype=np.float32)
S, OFFSET = 4096, 5
KNOWN = {1234: [[2060, 1036, 0, 495, 505], [0, 0, 4096, 0, 0], [245, 267, 250, 281, 3053]],
         7: [[2064, 1019, 0, 521, 492], [0, 0, 4096, 0, 0], [248, 243, 230, 255, 3120]]}
_LABELS = {}


def _labels(seed):
    if seed not in _LABELS:
        _LABELS[seed] = fr.replay_labels(ROWS, S, seed, OFFSET)
    return _LABELS[seed]


def _counts(seed):
    lab = _labels(seed)
    return [np.bincount(lab[:, i], minlength=ROWS.shape[1]).tolist() for i in range(ROWS.shape[0])]


@pytest.mark.parametrize("seed", sorted(KNOWN))
def test_replay_known_answers(seed):
    assert _counts(seed) == KNOWN[seed]


@pytest.mark.parametrize("seed", sorted(KNOWN))
def test_frequency_band_and_zero_classes(seed):
    worst = 0.0
    for row, counts in zip(ROWS.astype(np.float64), _counts(seed)):
        for p, c in zip(row, counts):
            sd = math.sqrt(S * p * (1.0 - p))
            if p == 0.0:
                assert c == 0                                   # a zero-probability class is never drawn
            if sd == 0.0:
                assert c == S * p
                continue
            worst = max(worst, abs(c - S * p) / sd)
            assert abs(c - S * p) <= 4.0 * sd, (seed, p, c)
    print(f"seed {seed}: worst |count - S p| / sqrt(S p (1 - p)) = {worst:.2f}")


def test_replay_depends_on_sample_and_global_example_only():
    """rows [a, b) replayed at example_offset + a equal the slice of the whole replay; labels -1 on a dead row"""
    whole = fr.replay_labels(ROWS, 64, 9, 3)
    part = fr.replay_labels(ROWS[1:], 64, 9, 4)
    assert np.array_equal(whole[:, 1:], part)
    dead = np.array([[0.0, 0.0, 0.0], [float("nan"), 0.5, 0.5]], dtype=np.float32)
    U, lab = fr.replay(dead, 3, 1)
    assert (lab[:, 0] == -1).all() and np.array_equal(U[:, 0], np.broadcast_to(-dead[0], (3, 3)))
    assert (lab[:, 1] == -1).all()                               # a row with a NaN is no distribution


def test_mc_definition_is_unbiased_for_the_head_hessian():
    g = torch.Generator().manual_seed(0)
    p = torch.softmax(3.0 * torch.randn(4, 7, dtype=torch.float64, generator=g), dim=-1)
    E = torch.eye(7, dtype=torch.float64)[None, :, :] - p[:, None, :]                 # (n, k, K): e_k - p
    mean = torch.einsum("nk,nka,nkb->nab", p, E, E)
    H = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    assert (mean - H).abs().max().item() <= 1e-15
    U = fr.exact_expectation_cotangents(p)                                            # (K, n, K)
    assert (torch.einsum("kna,knb->nab", U, U) - H).abs().max().item() <= 1e-15


def test_spec_validation():
    with pytest.raises(ValueError):
        fisher.MCFisher(0)
    with pytest.raises(ValueError):
        fisher.MCFisher(2.5)
    with pytest.raises(ValueError):
        fisher.MCFisher(2, seed="a")
    with pytest.raises(ValueError):
        fisher.Cotangents(torch.zeros(1, 4, 3), divisor=0.0)
    with pytest.raises(ValueError):
        fisher.resolve("fisher")
    assert fisher.resolve(None) is None and fisher.resolve("ggn") is None and fisher.spec_key("ggn") is None

    M, K = 4, 3
    fisher.EmpiricalFisher(torch.tensor([0, 2, 1, 1])).check(M, K, "classifier")
    for bad in (torch.tensor([0, 2, 1]), torch.tensor([0.0, 2.0, 1.0, 1.0]), torch.tensor([0, 3, 1, 1]),
                torch.tensor([0, -1, 1, 1]), torch.zeros(4, 3, dtype=torch.int64), torch.tensor([True, False, True, True])):
        with pytest.raises(ValueError):
            fisher.EmpiricalFisher(bad).check(M, K, "classifier")
    fisher.EmpiricalFisher(torch.zeros(M, K)).check(M, K, "regressor")
    for bad in (torch.zeros(M), torch.zeros(M + 1, K), torch.zeros(M, K, dtype=torch.int64)):
        with pytest.raises(ValueError):
            fisher.EmpiricalFisher(bad).check(M, K, "regressor")
    fisher.Cotangents(torch.zeros(2, M, K)).check(M, K, "classifier")
    for bad in (torch.zeros(2, M + 1, K), torch.zeros(M, K), torch.zeros(2, M, K, dtype=torch.int32), torch.zeros(0, M, K)):
        with pytest.raises(ValueError):
            fisher.Cotangents(bad).check(M, K, "classifier")
    with pytest.raises(ValueError):
        fisher.MCFisher(2).check(M, fisher.MAX_CLASSES + 1, "classifier")
    fisher.MCFisher(2).check(M, fisher.MAX_CLASSES + 1, "regressor")


def test_keys_distinguish_seeds_sample_counts_and_targets():
    keys = [fisher.MCFisher(3, 1).key(), fisher.MCFisher(3, 2).key(), fisher.MCFisher(4, 1).key(),
            fisher.EmpiricalFisher(torch.tensor([0, 1, 1])).key(), fisher.EmpiricalFisher(torch.tensor([0, 1, 0])).key(),
            fisher.EmpiricalFisher(torch.tensor([[0.5], [1.0], [0.0]])).key()]
    U = torch.zeros(2, 3, 2)
    keys += [fisher.Cotangents(U).key(), fisher.Cotangents(U, 2.0).key(), fisher.Cotangents(U.clone()).key()]
    assert len(set(keys)) == len(keys)
    for k in keys:
        hash(k)
    assert fisher.MCFisher(3, 1).key() == fisher.MCFisher(3, 1).key()
    assert fisher.EmpiricalFisher(torch.tensor([0, 1, 1])).key() == fisher.EmpiricalFisher([0, 1, 1]).key()
    assert fisher.MCFisher(3, -1).seed == 2 ** 64 - 1
    U.add_(1.0)                                                  # an in-place edit of the block is another fit
    assert fisher.Cotangents(U).key() != keys[6]


def test_reexports():
    from lip_amd import lla
    assert lla.MCFisher is fisher.MCFisher and lla.EmpiricalFisher is fisher.EmpiricalFisher
    assert lla.Cotangents is fisher.Cotangents and lla.sample_head_cotangents is fisher.sample_head_cotangents
