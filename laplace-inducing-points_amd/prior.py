"""Layer-wise prior precisions: the Gaussian prior N(0, A^-1) with A = diag(a), a_j = alpha_{g(j)}, g(j) the group of
flat parameter j.  Not a reference structure: the reference has one scalar ``alpha`` (``src/lla.py:21-22``); every
function of this package that takes ``alpha`` takes a :class:`GroupedPrior` in its place where INTEGRATION.md says so.

The group table is derived from the flat-parameter layout (``utils.param_layout``: sorted-key traversal, C-order
leaves), so it is valid for exactly the vectors ``flatten_nn_params`` produces.
"""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple, Union

import torch

from .utils import param_layout

Segment = Tuple[int, int]                                   # (offset, length) in the flat vector


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _name(key) -> str:
    if isinstance(key, tuple):
        return "/".join(str(k) for k in key)
    return str(key)


def _check_table(table, D: int) -> None:
    """the segments of all groups cover [0, D) exactly once"""
    segs = sorted((int(o), int(n)) for _, ss in table for o, n in ss)
    pos = 0
    for o, n in segs:
        if n <= 0:
            raise ValueError(f"group table: empty or negative segment ({o}, {n})")
        if o != pos:
            raise ValueError(f"group table: {'overlap' if o < pos else 'gap'} at flat offset {min(o, pos)} "
                             f"(the segments must cover [0, {D}) exactly once)")
        pos = o + n
    if pos != D:
        raise ValueError(f"group table covers [0, {pos}), the parameter vector has {D} entries")
    if any(not ss for _, ss in table):
        raise ValueError("group table: a group without segments")


def _check_values(values, G: int) -> torch.Tensor:
    v = torch.as_tensor(values, dtype=torch.float64).detach().cpu().reshape(-1).clone()
    if v.numel() == 1 and G > 1:
        v = v.repeat(G)
    if v.numel() != G:
        raise ValueError(f"{G} groups need {G} precisions (or one shared value), got {v.numel()}")
    if not bool(torch.isfinite(v).all()) or not bool((v > 0).all()):
        raise ValueError("prior precisions must be finite and positive")
    return v


class GroupedPrior:
    """One prior precision per parameter group.

    ``groups``: ``"tensor"`` (one group per leaf), ``"layer"`` (leaves sharing ``path[:-1]``: a kernel and its bias, a
    BN scale and its bias), a callable ``path -> hashable key`` (equal keys form a group; the group need not be
    contiguous in the flat vector), or a list with one group index per leaf (indices 0 .. G-1, each used).
    Groups are numbered in the order of their first flat offset, except with an explicit index list, whose indices are
    the group numbers (group ``i`` is named ``group<i>``).  ``values``: (G,) precisions or one shared number.
    """

    def __init__(self, params, values, groups: Union[str, Callable, Sequence[int]] = "layer"):
        layout = param_layout(params)
        if isinstance(groups, str) and groups == "tensor":
            keys = [path for path, _, _ in layout]
        elif isinstance(groups, str) and groups == "layer":
            keys = [path[:-1] for path, _, _ in layout]
        elif isinstance(groups, str):
            raise ValueError("groups must be 'tensor', 'layer', a callable or a list of group indices")
        elif callable(groups):
            keys = [groups(path) for path, _, _ in layout]
        else:
            keys = [int(g) for g in groups]
            if len(keys) != len(layout):
                raise ValueError(f"{len(layout)} leaves need {len(layout)} group indices, got {len(keys)}")
            if sorted(set(keys)) != list(range(len(set(keys)))):
                raise ValueError("group indices must be 0 .. G-1 with every index used")
        explicit = not isinstance(groups, str) and not callable(groups)
        order: List = sorted(set(keys)) if explicit else list(dict.fromkeys(keys))
        index = {k: i for i, k in enumerate(order)}
        table: List[Tuple[str, List[Segment]]] = [(f"group{k}" if explicit else _name(k), []) for k in order]
        for (path, off, shape), k in zip(layout, keys):
            n = _numel(shape)
            if n == 0:
                continue
            segs = table[index[k]][1]
            if segs and segs[-1][0] + segs[-1][1] == off:
                segs[-1] = (segs[-1][0], segs[-1][1] + n)    # adjacent leaves of one group: one segment
            else:
                segs.append((off, n))
        D = sum(_numel(shape) for _, _, shape in layout)
        self._init(table, values, D)

    def _init(self, table, values, D: int):
        table = [(str(name), [(int(o), int(n)) for o, n in segs]) for name, segs in table]
        _check_table(table, int(D))
        self.table, self.D = table, int(D)
        self.values = _check_values(values, len(table))
        self._vec = {}
        return self

    @classmethod
    def from_table(cls, table, values, D: int) -> "GroupedPrior":
        """a prior on an explicit ``[(name, [(offset, length), ...]), ...]`` table over [0, D)"""
        return cls.__new__(cls)._init(table, values, D)

    # ------------------------------------------------------------------------------------------ the table
    @property
    def G(self) -> int:
        return len(self.table)

    @property
    def names(self) -> List[str]:
        return [name for name, _ in self.table]

    @property
    def sizes(self) -> torch.Tensor:
        """(G,) int64: D_g"""
        return torch.tensor([sum(n for _, n in segs) for _, segs in self.table], dtype=torch.int64)

    def segments(self, g: int) -> List[Segment]:
        return list(self.table[g][1])

    def key(self):
        """hashable identity of the prior (values and group table): what caches key on in place of ``float(alpha)``"""
        return (tuple(self.values.tolist()), tuple((name, tuple(segs)) for name, segs in self.table))

    def with_values(self, values) -> "GroupedPrior":
        return GroupedPrior.from_table(self.table, values, self.D)

    # ------------------------------------------------------------------------------------------ vectors
    def vector(self, device="cpu", dtype=torch.float32) -> torch.Tensor:
        """(D,) expanded precisions a_j = alpha_{g(j)}, cached per (device, dtype); do not write to it"""
        k = (str(torch.device(device)), dtype)
        v = self._vec.get(k)
        if v is None:
            a = torch.empty(self.D, dtype=torch.float64)
            for g, (_, segs) in enumerate(self.table):
                for o, n in segs:
                    a[o:o + n] = self.values[g]
            v = a.to(device=device, dtype=dtype)
            self._vec[k] = v
        return v

    def group_sqnorms(self, flat: torch.Tensor) -> torch.Tensor:
        """(G,) float64 ||theta_g||^2 of a flat parameter vector (on its device)"""
        flat = flat.detach().reshape(-1)
        if flat.numel() != self.D:
            raise ValueError(f"expected {self.D} parameters, got {flat.numel()}")
        f2 = flat.double() ** 2
        return torch.stack([sum(f2[o:o + n].sum() for o, n in segs) for _, segs in self.table])

    def __repr__(self):
        lo, hi = float(self.values.min()), float(self.values.max())
        return f"GroupedPrior(G={self.G}, D={self.D}, precisions in [{lo:.3g}, {hi:.3g}])"


def is_grouped(alpha) -> bool:
    return isinstance(alpha, GroupedPrior)


def check_dim(prior: GroupedPrior, D: int) -> GroupedPrior:
    if prior.D != int(D):
        raise ValueError(f"the prior covers {prior.D} parameters, the network has {D}")
    return prior
