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


ROW_OF_WEIGHT = (2, 3, 6, 7, 0, 1, 4, 5, 8, 9)   # weights.txt / Params position -> position in the parameter row (shared_of)


def fit_trajectory(solver, kb, variant, target, weights, starts=16, steps=100, seed=0, lr=0.05, spread=float(np.log(1.3)),
                   columns=(0, 1, 2, 3, 4, 5)):
    """Which weights reproduce a recorded trajectory?  Multi-start projected Adam on the ten weights of candidate 0 of the
    knots.KnotBatch kb, organised as `descend`: every start is a parameter set of one batched launch, the gradient runs
    through diff.solve + diff.sample.  Minimised per start: the mean squared difference between the sampled trajectory
    and target [6, n] (rows s, ds, dds, l, dl, ddl every kb.delta seconds, as find_traj writes them) over `columns` (a
    subset of the six) and the samples both have.  The starts are `weights` (ten values, weights.txt / Params order) with
    every log-weight moved by +-spread (random signs from `seed`); Adam steps on the
    log-weights, projected on the box BOX.  A start whose solve fails (status outside {1, 2}) is left out of the means.

    Returns what `descend` returns with the loss in place of a_cost -- the mean loss of the starts at the first and after
    the last step, the best loss seen, the per-step means, the solve count -- plus "losses" (per start, after the last
    step), "max_dev" ([6] largest |difference| per column of the best start, over the compared samples) and "weights"
    [starts, 10] in weights.txt order.

    What the Nelder-Mead fit of tests/golden/fit_weights.py established holds here too: the solve's optimum is invariant
    under a common factor on one axis' weights, so weights are recoverable only up to one scale per axis; the loss, not
    the distance to some known weights, is the measure of a fit."""
    d = solver.device
    W = np.clip(np.asarray(weights, dtype=np.float64)[:10], *BOX)
    rec = replicated_record(solver, kb, variant, starts)
    rng = np.random.default_rng(seed)
    w0 = W[None, :] * np.exp(spread * rng.choice([-1.0, 1.0], (starts, 10)))
    rows = np.stack([diff.params_from_shared(shared_of(w, kb.header, kb.delta, variant)) for w in np.clip(w0, *BOX)])
    U = torch.tensor(np.log(rows[:, :10]), dtype=torch.float64, device=d, requires_grad=True)
    rest = torch.tensor(rows[:, 10:], dtype=torch.float64, device=d)
    idx = torch.arange(starts, dtype=torch.int32, device=d)
    tgt = torch.as_tensor(np.asarray(target, dtype=np.float64), device=d)
    cols = torch.tensor(sorted(int(c) for c in columns), dtype=torch.long, device=d)
    lo, hi = float(np.log(BOX[0])), float(np.log(BOX[1]))
    opt = torch.optim.Adam([U], lr=lr)
    means, best, state = [], np.inf, {}

    def evaluate():
        P = torch.cat([torch.exp(U), rest], dim=1)
        ctrl, _, st = diff.solve(solver, rec["seg"], rec["init"], rec["ref_end"], rec["dl_bounds"], P,
                                 seg_count=rec["seg_count"], set_index=idx, variant=variant, delta=kb.delta)
        traj, npts = diff.sample(ctrl, rec["seg"], rec["init"], solver, seg_count=rec["seg_count"], delta=kb.delta)
        if "n" not in state:
            state["n"] = min(int(tgt.shape[1]), int(traj.shape[2]), int(npts.min().item()))
        n = state["n"]
        dev = traj[:, :, :n] - tgt[None, :, :n]
        loss = (dev[:, cols] ** 2).mean(dim=(1, 2))
        ok = (st == 1) | (st == 2)
        return loss, ok, dev

    def record(loss, ok):
        nonlocal best
        l = loss.detach()[ok]
        means.append(float(l.mean()) if l.numel() else float("nan"))
        if l.numel():
            best = min(best, float(l.min()))

    for _ in range(steps):
        opt.zero_grad()
        loss, ok, _ = evaluate()
        record(loss, ok)
        loss[ok].sum().backward()
        opt.step()
        with torch.no_grad():
            U.clamp_(lo, hi)
    with torch.no_grad():
        loss, ok, dev = evaluate()
    record(loss, ok)
    final = torch.where(ok, loss, torch.full_like(loss, float("inf")))
    b = int(torch.argmin(final).item())
    w_rows = torch.exp(U.detach()).cpu().numpy()
    return dict(start_mean=means[0], final_mean=means[-1], best=best, means=means, solves=starts * (steps + 1),
                losses=final.cpu().numpy(), max_dev=dev[b].abs().amax(dim=1).cpu().numpy(), samples=state["n"],
                weights=w_rows[:, list(ROW_OF_WEIGHT)])


def fit_trajectory_lm(solver, kb, variant, target, weights, starts=16, steps=25, seed=0, spread=float(np.log(1.3)),
                      columns=(0, 1, 2, 3, 4, 5), damping=1e-2, damping_range=(1e-7, 1e7)):
    """fit_trajectory's problem -- the same starts (weights, seed, spread), the same loss -- by Levenberg-Marquardt on the
    ten log-weights: it is a least-squares problem with ten unknowns, and forward mode gives its Jacobian from ONE
    factorisation per axis problem.  Every start is a parameter set of one batched launch.  Per step: the Jacobian of the
    control points with respect to the ten log-weights at the current weights (diff.solve_jacobian, log=True, on the solve
    the previous step accepted), through the sampling (diff.sample_jvp) to the residuals' J [m, 10] per start; the damped
    normal equations (J'J + damping mean(diag J'J) I) step = -J'r per start (torch, 10 x 10); a trial solve of every
    start at its stepped weights, projected on BOX; per start, accept when the loss fell (damping / 3) or keep the old
    point (damping x 4).  The weights are determined only up to one factor per axis (fit_trajectory), so J'J has a
    two-dimensional null space: the damping is kept inside damping_range and never reaches 0.

    Returns fit_trajectory's dict.  "solves" counts every candidate solved, trial solves included: starts (steps + 1);
    "jvp_launches" is the number of JVP launches (steps), each over the `starts` candidates; "accepted" the accepted
    steps per start."""
    d = solver.device
    W = np.clip(np.asarray(weights, dtype=np.float64)[:10], *BOX)
    rec = replicated_record(solver, kb, variant, starts)
    rng = np.random.default_rng(seed)
    w0 = W[None, :] * np.exp(spread * rng.choice([-1.0, 1.0], (starts, 10)))
    rows = np.stack([diff.params_from_shared(shared_of(w, kb.header, kb.delta, variant)) for w in np.clip(w0, *BOX)])
    U = torch.tensor(np.log(rows[:, :10]), dtype=torch.float64, device=d)
    rest = torch.tensor(rows[:, 10:], dtype=torch.float64, device=d)
    idx = torch.arange(starts, dtype=torch.int32, device=d)
    tgt = torch.as_tensor(np.asarray(target, dtype=np.float64), device=d)
    cols = torch.tensor(sorted(int(c) for c in columns), dtype=torch.long, device=d)
    lo, hi = float(np.log(BOX[0])), float(np.log(BOX[1]))
    args = (rec["seg"], rec["init"], rec["ref_end"], rec["dl_bounds"])
    kw = dict(seg_count=rec["seg_count"], set_index=idx, variant=variant, delta=kb.delta)
    state = {}

    def solve_at(Uc):
        o = diff.solve_kept(solver, *args, torch.cat([torch.exp(Uc), rest], dim=1), **kw)
        traj, npts = diff.sample(o["ctrl"], rec["seg"], rec["init"], solver, seg_count=rec["seg_count"], delta=kb.delta)
        if "n" not in state:
            state["n"] = min(int(tgt.shape[1]), int(traj.shape[2]), int(npts.min().item()))
        dev = traj[:, :, :state["n"]] - tgt[None, :, :state["n"]]
        ok = (o["status"] == 1) | (o["status"] == 2)
        loss = torch.where(ok, (dev[:, cols] ** 2).mean(dim=(1, 2)), torch.full((starts,), float("inf"), dtype=torch.float64, device=d))
        return o, dev, loss

    def mean_of(loss):
        l = loss[torch.isfinite(loss)]
        return float(l.mean()) if l.numel() else float("nan")

    out, dev, loss = solve_at(U)
    lam = torch.full((starts,), float(damping), dtype=torch.float64, device=d)
    accepted = torch.zeros(starts, dtype=torch.int64, device=d)
    means = [mean_of(loss)]
    eye = torch.eye(10, dtype=torch.float64, device=d)
    for _ in range(steps):
        jac = diff.solve_jacobian(solver, *args, torch.cat([torch.exp(U), rest], dim=1), range(10), log=True, out=out, **kw)
        dtraj = diff.sample_jvp(solver, jac["dctrl"], rec["seg"], seg_count=rec["seg_count"], delta=kb.delta)
        n = state["n"]
        J = dtraj[:, :, cols, :n].permute(1, 2, 3, 0).reshape(starts, -1, 10)      # [starts, m, 10]
        r = dev[:, cols].reshape(starts, -1)                                       # [starts, m]
        live = torch.isfinite(loss)
        J = torch.where(live[:, None, None], J, torch.zeros_like(J))
        r = torch.where(live[:, None], r, torch.zeros_like(r))
        A = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])[:, :, 0]
        scale = A.diagonal(dim1=1, dim2=2).mean(dim=1)
        usable = live & (scale > 0) & torch.isfinite(scale)
        # (a start without a solve, or whose Jacobian vanishes, gets the identity system: step 0, never a singular member)
        Ad = torch.where(usable[:, None, None], A + (lam * scale)[:, None, None] * eye, eye.expand(starts, 10, 10))
        g = torch.where(usable[:, None], g, torch.zeros_like(g))
        step = -torch.linalg.solve(Ad, g[:, :, None])[:, :, 0]
        U_try = (U + step).clamp(lo, hi)
        o_t, dev_t, loss_t = solve_at(U_try)
        acc = live & torch.isfinite(loss_t) & (loss_t < loss)
        U = torch.where(acc[:, None], U_try, U)
        dev = torch.where(acc[:, None, None], dev_t, dev)
        loss = torch.where(acc, loss_t, loss)
        out = dict(out)
        out["ctrl"] = torch.where(acc[:, None], o_t["ctrl"], out["ctrl"])
        out["lam"] = torch.where(acc[None, None, :, None], o_t["lam"], out["lam"])
        out["status"] = torch.where(acc, o_t["status"], out["status"])
        out["cost"] = torch.where(acc, o_t["cost"], out["cost"])
        lam = torch.where(acc, lam / 3.0, lam * 4.0).clamp(*damping_range)
        accepted += acc.long()
        means.append(mean_of(loss))
    b = int(torch.argmin(loss).item())   # (every start failed: start 0, loss inf)
    w_rows = torch.exp(U).cpu().numpy()
    return dict(start_mean=means[0], final_mean=means[-1], best=float(loss.min()), means=means, solves=starts * (steps + 1),
                jvp_launches=steps, accepted=accepted.cpu().numpy(), losses=loss.cpu().numpy(),
                max_dev=dev[b].abs().amax(dim=1).cpu().numpy(), samples=state["n"], weights=w_rows[:, list(ROW_OF_WEIGHT)])
