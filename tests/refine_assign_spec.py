"""NumPy statement of okp_refine_assignments, written from the specification in include/okp.h on top of the two specifications it extends:
the hypotheses and the rigid fit of the pose stage (tests/object_pose_spec.py: hypotheses, fit_kabsch, degenerate) and the Gauss-Newton
refinement of one object (tests/refine_spec.py: refine_object).  Every hypothesis is refined from its own rigid fit; among those that end
with status 0 the least final cost wins, the lowest index on exactly equal cost.  The device finds the fit by Horn's closed form and sums in
a butterfly, so the two are compared by tolerance (tests/test_gpu_refine_assign.py)."""
import numpy as np

import object_pose_spec as pose_spec
import refine_spec

NONE = 16
MAX_HYPOTHESES = 24
SKIPPED, SINGULAR, BEHIND, REJECTED = refine_spec.SKIPPED, refine_spec.SINGULAR, refine_spec.BEHIND, refine_spec.REJECTED


def count_hypotheses(type_count):
    """prod c_k!: what the entry point refuses above MAX_HYPOTHESES."""
    out = 1
    for c in type_count:
        for i in range(2, c + 1):
            out *= i
    return out


def refine_object(tab_o, pose_o, assignment_o, model, type_count, fx, fy, sigma_px, sigma_z, iters, damping, fit=pose_spec.fit_kabsch, diag=None):
    """One live object -> dict(pose [12], fit [4], information [36], status, assignment [S], hypothesis [2], cost [2]).  diag (a dict) receives
    "hypotheses": per hypothesis a dict of its rows, its status, its start pose, refine_spec.refine_object's diag and the second-eigenvalue
    ratio of its matched model points."""
    nan = np.nan
    S = model.shape[0]

    def refused(status):
        return dict(pose=pose_o.copy(), fit=np.full(4, nan), information=np.full(36, nan), status=status, assignment=np.array(assignment_o, dtype=np.int32),
                    hypothesis=np.full(2, -1, dtype=np.int32), cost=np.full(2, nan))

    filled = np.isfinite(tab_o).all(axis=1)
    rows = tab_o[filled]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = rows[:, 0] / rows[:, 2], rows[:, 1] / rows[:, 2]
    if not np.isfinite(pose_o).all() or int(filled.sum()) < 3 or (rows[:, 2] == 0.0).any() or not np.isfinite(u).all() or not np.isfinite(v).all():
        return refused(SKIPPED)
    hyps = pose_spec.hypotheses(filled, type_count)
    assert 1 <= len(hyps) <= MAX_HYPOTHESES
    results, records = [], []
    for h, matched in enumerate(hyps):
        asg = np.full(S, -1, dtype=np.int32)
        asg[np.flatnonzero(filled)] = matched
        rec = dict(rows=list(matched), ratio=pose_spec.second_eigenvalue_ratio(model[matched]))
        if pose_spec.degenerate(model[matched]):
            rec.update(status=SINGULAR, degenerate=True)
            results.append(None)
            records.append(rec)
            continue
        R, t, _, _ = fit(model[matched], rows[:, :3])
        start = np.concatenate([R, t[:, None]], axis=1).reshape(12)
        d = {}
        pose, fit4, info, status = refine_spec.refine_object(tab_o, start, asg, model, fx, fy, sigma_px, sigma_z, iters, damping, diag=d)
        rec.update(status=status, degenerate=False, start=start, diag=d)
        records.append(rec)
        results.append((d["J_final"], h, pose, fit4, info, asg) if status == 0 else None)
    if diag is not None:
        diag["hypotheses"] = records
    ranked = sorted((r for r in results if r is not None), key=lambda r: (r[0], r[1]))
    if not ranked:
        return refused(NONE)
    J, h, pose, fit4, info, asg = ranked[0]
    second = ranked[1] if len(ranked) > 1 else None
    return dict(pose=pose, fit=fit4, information=info, status=0, assignment=asg,
                hypothesis=np.array([h, second[1] if second else -1], dtype=np.int32), cost=np.array([J, second[0] if second else nan]))


def refine_assignments(tab, pose, assignment, n_obj, model, type_count, fx, fy, sigma_px=0.25, sigma_z=0.05, iters=6, damping=1e-9, fit=pose_spec.fit_kabsch,
                       diags=None):
    """Whole tensors -> {"pose" [B,max_obj,12], "fit" [..,4], "information" [..,36], "status" [B,max_obj] int32, "assignment" [..,S] int32,
    "hypothesis" [..,2] int32, "cost" [..,2]}.  diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj, S = tab.shape[:3]
    assert model.shape == (S, 3) and S == 1 + sum(type_count)
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 4), np.nan), "information": np.full((B, max_obj, 36), np.nan),
           "status": np.full((B, max_obj), SKIPPED, dtype=np.int32), "assignment": np.full((B, max_obj, S), -1, dtype=np.int32),
           "hypothesis": np.full((B, max_obj, 2), -1, dtype=np.int32), "cost": np.full((B, max_obj, 2), np.nan)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            got = refine_object(tab[b, o], pose[b, o], assignment[b, o], model, type_count, fx, fy, sigma_px, sigma_z, iters, damping, fit=fit, diag=d)
            for key, value in got.items():
                out[key][b, o] = value
            if diags is not None:
                diags[(b, o)] = d
    return out
