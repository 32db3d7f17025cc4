"""Timing of the layer-wise evidence terms at the ResNet-50 block table (D = 25.6 M, one prior group per layer): one fit
is ``--evals`` evaluations of ``EvidencePlan.terms`` (``lip_evidence_terms``: two launches), timed next to the float64
torch expression it replaces, which per block forms outer(lam_l, mu_l) (KFAC) or reads Lam_l (EKFAC), scales it by
c_l r / alpha_g and takes log1p(.).sum() and (x / (1 + x)).sum(): the form ``kfac.kfac_spectrum`` +
``train_alpha._lml_from_spectrum`` would take group by group.  The spectra are synthetic (no network is bound): the
cost depends on the table alone.

Prints one JSON line per case:
  * kfac_kernel / kfac_torch      KRON segments: Mt + N numbers per block stand for its Mt N eigenvalues
  * ekfac_kernel / ekfac_torch    LIST segments: the 25.6 M second moments are resident either way
each with the time of ``--evals`` evaluations (CUDA events on the current stream around the whole loop, which ends in
a synchronise; warm-up loops first; median, min and max over ``--reps`` loops), the bytes the plan keeps resident, the
peak of ``torch.cuda.max_memory_allocated`` above the resident operands during a loop, and the largest relative
difference between the two routes' (L, T).

    python scripts/evidence_bench.py [--evals 200] [--reps 5] [--warmup 1] [--dry-run]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lip_amd  # noqa: E402,F401
from kfac_bench import emit, timed  # noqa: E402
from lip_amd import evidence as ev  # noqa: E402
from lip_amd import kfac  # noqa: E402
from lip_amd.prior import GroupedPrior  # noqa: E402
from lip_amd.scalemodels import ResNet50  # noqa: E402
from lip_amd.toymodels import create_state  # noqa: E402
from lip_amd.utils import flatten_nn_params  # noqa: E402

F64 = torch.float64


def spectrum(n, g):
    """n synthetic eigenvalues, log-uniform over twelve decades"""
    return 10.0 ** (12.0 * torch.rand(n, dtype=F64, generator=g) - 8.0)


def tables(state, M=1000):
    """(prior, blocks, groups, remainder indices) of the net, and the per-block scale c_l = 1 / (M T_l)"""
    prior = GroupedPrior(state.params, 1.0, "layer")
    blocks = kfac.block_table(state)
    D = flatten_nn_params(state.params)[0].numel()
    return prior, blocks, ev.block_groups(prior, blocks, D), kfac.remainder_indices(blocks, D), [1.0 / (M * b.T) for b in blocks]


def build(kind, prior, blocks, groups, rem, scales, dev):
    """the plan of plan_from_kfac / plan_from_ekfac on synthetic numbers, and the per-block operands of the torch route"""
    g = torch.Generator().manual_seed(5)
    parts, segs, ops, off = [], [], [], 0
    for b, grp, c in zip(blocks, groups, scales):
        if kind == "kfac":
            lam, mu = spectrum(b.Mt, g), spectrum(b.N, g)
            parts += [lam, mu]
            segs.append(ev.Segment(ev.KRON, off, b.Mt, b.N, c, grp))
            ops.append((grp, c, lam.to(dev), mu.to(dev)))
            off += b.Mt + b.N
        else:
            Lam = spectrum(b.Mt * b.N, g)
            parts.append(Lam)
            segs.append(ev.Segment(ev.LIST, off, b.Mt * b.N, 1, c, grp))
            ops.append((grp, c, Lam.to(dev), None))
            off += b.Mt * b.N
    diag = spectrum(rem.numel(), g)
    parts.append(diag)
    for s in ev._remainder_segments(prior, rem, off):
        segs.append(s)
        ops.append((s.group, 1.0, diag[s.off - off:s.off - off + s.rows].to(dev), None))
    plan = ev.EvidencePlan(torch.cat(parts).to(dev), segs, torch.ones(prior.G, dtype=F64), prior.names)
    return plan, ops


def terms_torch_blocks(ops, la, r, G):
    """the torch route: per block outer / log1p / sum, added per group; log alpha stays on the device"""
    s = r / torch.exp(la)
    L = [[] for _ in range(G)]
    T = [[] for _ in range(G)]
    for grp, c, lam, mu in ops:
        x = (c * s[grp]) * (torch.outer(lam, mu) if mu is not None else lam)
        L[grp].append(torch.log1p(x).sum())
        T[grp].append((x / (1.0 + x)).sum())
    return torch.stack([torch.stack(p).sum() for p in L]), torch.stack([torch.stack(p).sum() for p in T])


def peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true", help="build the tables on the CPU, print their sizes and stop")
    args = ap.parse_args()
    state = create_state(ResNet50(1000), seed=0, dtype=torch.float32)
    prior, blocks, groups, rem, scales = tables(state)
    D = prior.D
    del state
    if args.dry_run:
        for kind in ("kfac", "ekfac"):
            plan, _ = build(kind, prior, blocks, groups, rem, scales, "cpu")
            print(dict(kind=kind, D=D, G=plan.G, blocks=len(blocks), segments=len(plan.segments), chunks=len(plan.chunks),
                       pool=plan.vals.numel(), terms=int(plan.terms_per_group.sum())))
        return
    if not torch.cuda.is_available():
        raise SystemExit("evidence_bench.py times the device kernel: no GPU found")
    dev = torch.device("cuda")
    r = 1281167 / 1000
    la = torch.linspace(-3.0, 3.0, prior.G, dtype=F64, device=dev)
    for kind in ("kfac", "ekfac"):
        plan, ops = build(kind, prior, blocks, groups, rem, scales, dev)
        shape = dict(D=D, G=plan.G, segments=len(plan.segments), chunks=len(plan.chunks), evals=args.evals)

        def kernel_loop():
            for _ in range(args.evals):
                out = plan.terms(la, r)
            return out

        def torch_loop():
            for _ in range(args.evals):
                out = terms_torch_blocks(ops, la, r, plan.G)
            return out

        Lk, Tk = plan.terms(la, r)
        Lt, Tt = terms_torch_blocks(ops, la, r, plan.G)
        diff = max(float(((Lk - Lt).abs() / Lt).max()), float(((Tk - Tt).abs() / Tt).max()))
        resident_k = 8 * plan.vals.numel() + sum(t.numel() * t.element_size() for t in plan._dev.values() if torch.is_tensor(t))
        resident_t = sum(8 * (lam.numel() + (0 if mu is None else mu.numel())) for _, _, lam, mu in ops)
        emit(f"{kind}_kernel", timed(kernel_loop, args.reps, args.warmup), resident_bytes=resident_k,
             peak_extra_bytes=peak_over(kernel_loop), max_rel_diff=diff, **shape)
        emit(f"{kind}_torch", timed(torch_loop, args.reps, args.warmup), resident_bytes=resident_t,
             peak_extra_bytes=peak_over(torch_loop), max_rel_diff=diff, **shape)
        del plan, ops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
