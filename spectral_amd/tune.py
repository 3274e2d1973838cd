"""Weight tuning against a_cost, the score find_traj returns: multi-start projected Adam on the solve's weights, with
gradients through diff.solve + diff.traj_cost.  Every start is a parameter set of one batched launch."""
import numpy as np
import torch

from . import diff, layout as L

BOX = (1e-3, 50.0)   # the reference sweep's U(0, 50) box, kept off 0


def shared_of(w, header, delta, variant):
    """weights.txt order (Params) + a corridor file's header -> layout.Shared."""
    w = [float(v) for v in w]
    return L.Shared(w_s=(w[4], w[5], w[0], w[1]), w_l=(w[6], w[7], w[2], w[3]), weight_end_s=w[8], weight_end_l=w[9],
                    ds_ref=header["ds_ref"], dl_ref=header["dl_ref"], dds=tuple(header["dds"]), ddds=tuple(header["ddds"]),
                    ddl=tuple(header["ddl"]), dddl=tuple(header["dddl"]), delta=delta, variant=variant)


def replicated_record(solver, kb, variant, n):
    """The device corridor stage's record of candidate 0 of a knots.KnotBatch, n copies side by side (seg_stride 64)."""
    rec = solver.corridor_batch(kb, variant, seg_stride=64)
    return dict(B=n, seg_stride=64, seg=rec["seg"][:, :1].repeat(1, n, 1).contiguous(),
                seg_count=rec["seg_count"][:1].repeat(n).contiguous(), init=rec["init"][:1].repeat(n, 1).contiguous(),
                ref_end=rec["ref_end"][:1].repeat(n, 1).contiguous(), dl_bounds=rec["dl_bounds"][:1].repeat(n, 1).contiguous())


def descend(solver, kb, variant, weights, starts=16, steps=30, seed=0, lr=1.0, score_weights=None, spread=0.3):
    """Adam on candidate 0 of the knots.KnotBatch kb from `starts` starts at +-spread perturbed copies of `weights` (ten
    values, weights.txt / Params order), projected on the box BOX.  The trapezoid's a_cost is degenerate over the weights
    the solve uses (every term carries one of them), so trapezoid runs are scored with FIXED weights (score_weights,
    default `weights`); the cuboid's a_cost has none.  Returns the mean a_cost of the starts at the first and after the
    last step, the best a_cost seen, the per-step means, the solve count and the final weights."""
    d = solver.device
    W = np.asarray(weights, dtype=np.float64)
    rec = replicated_record(solver, kb, variant, starts)
    rng = np.random.default_rng(seed)
    w0 = W[None, :10] * (1 + spread * rng.uniform(-1, 1, (starts, 10)))
    rows = np.stack([diff.params_from_shared(shared_of(w, kb.header, kb.delta, variant)) for w in w0])
    P = torch.tensor(rows, dtype=torch.float64, device=d, requires_grad=True)
    score = torch.tensor(diff.params_from_shared(shared_of(score_weights if score_weights is not None else W, kb.header,
                                                           kb.delta, variant)), dtype=torch.float64, device=d)
    idx = torch.arange(starts, dtype=torch.int32, device=d)
    s_ref = torch.tensor(kb.s_ref[0], dtype=torch.float64, device=d)
    l_ref = torch.tensor(kb.l_ref[0], dtype=torch.float64, device=d)
    # the ten weights move; ds_ref, dl_ref and the limits stay
    mask = torch.zeros(20, dtype=torch.float64, device=d); mask[:10] = 1.0
    opt = torch.optim.Adam([P], lr=lr)
    means, best = [], np.inf

    def evaluate():
        ctrl, _, st = diff.solve(solver, rec["seg"], rec["init"], rec["ref_end"], rec["dl_bounds"], P,
                                 seg_count=rec["seg_count"], set_index=idx, variant=variant, delta=kb.delta)
        a = diff.traj_cost(ctrl, rec["seg"], rec["init"], s_ref, l_ref, score, solver, seg_count=rec["seg_count"],
                           status=st, variant=variant, delta=kb.delta)
        return a

    for _ in range(steps):
        opt.zero_grad()
        a = evaluate()
        fin = torch.isfinite(a)
        means.append(float(a.detach()[fin].mean()))
        best = min(best, float(a.detach()[fin].min()))
        a[fin].sum().backward()
        P.grad *= mask
        opt.step()
        with torch.no_grad():
            P[:, :10].clamp_(*BOX)
    with torch.no_grad():
        a = evaluate()
    fin = torch.isfinite(a)
    means.append(float(a[fin].mean()))
    best = min(best, float(a[fin].min()))
    return dict(start_mean=means[0], final_mean=means[-1], best=best, means=means, solves=starts * (steps + 1),
                weights=P.detach()[:, :10].cpu().numpy())
