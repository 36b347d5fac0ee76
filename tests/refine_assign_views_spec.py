"""NumPy statement of okp_refine_assignments_views, written from the specification in include/okp.h on top of the two specifications it
combines: the hypotheses and the rigid fit of the pose stage (tests/object_pose_spec.py: hypotheses, fit_kabsch, degenerate) and the refinement
of one object against a table of views (tests/refine_views_spec.py: refine_object).  Every hypothesis on the filled mask of the table is
refined from its own rigid fit to the table's points against the bearings of the filled slots; among those that end with status 0 the least
final cost wins, the lowest index on exactly equal cost.  The device finds the fit by Horn's closed form and sums in butterflies, so the two
are compared by tolerance (tests/test_gpu_refine_assign_views.py)."""
import numpy as np

import object_pose_spec as pose_spec
import refine_views_spec as views_spec

NONE = 16
MAX_HYPOTHESES = 24
SKIPPED, SINGULAR, BEHIND, REJECTED = views_spec.SKIPPED, views_spec.SINGULAR, views_spec.BEHIND, views_spec.REJECTED


def observations(obs_o, filled):
    """The number of observations: the filled entries (s, v) of the filled slots."""
    return int(sum(np.isfinite(obs_o[s, v]).all() for s in np.flatnonzero(filled) for v in range(obs_o.shape[1])))


def refine_object(obs_o, views, tab_o, pose_o, assignment_o, model, type_count, sigma_px, iters, damping, fit=pose_spec.fit_kabsch, diag=None):
    """One live object -> dict(pose [12], fit [2], n_obs, information [36], status, assignment [S], hypothesis [2], cost [2]).  diag (a dict)
    receives "hypotheses": per hypothesis a dict of its rows, its status, its start pose, refine_views_spec.refine_object's diag and the
    second-eigenvalue ratio of its matched model points."""
    nan = np.nan
    S = model.shape[0]
    filled = np.isfinite(tab_o).all(axis=1)
    n_obs = observations(obs_o, filled)

    def refused(status):
        return dict(pose=pose_o.copy(), fit=np.full(2, nan), n_obs=n_obs, information=np.full(36, nan), status=status, assignment=np.array(assignment_o, dtype=np.int32),
                    hypothesis=np.full(2, -1, dtype=np.int32), cost=np.full(2, nan))

    halves = np.isnan(obs_o)
    malformed = bool((halves[..., 0] != halves[..., 1]).any() or np.isinf(obs_o).any())
    seen = sum(1 for s in np.flatnonzero(filled) if np.isfinite(obs_o[s]).all(axis=1).any())
    if not np.isfinite(pose_o).all() or malformed or seen < 3:
        return refused(SKIPPED)
    rows = tab_o[filled]
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
        pose, fit2, n, info, status = views_spec.refine_object(obs_o, views, start, asg, model, sigma_px, iters, damping, diag=d)
        assert n == n_obs                                               # the same number under every hypothesis
        rec.update(status=status, degenerate=False, start=start, diag=d)
        records.append(rec)
        results.append((d["J_final"], h, pose, fit2, info, asg) if status == 0 else None)
    if diag is not None:
        diag["hypotheses"] = records
    ranked = sorted((r for r in results if r is not None), key=lambda r: (r[0], r[1]))
    if not ranked:
        return refused(NONE)
    J, h, pose, fit2, info, asg = ranked[0]
    second = ranked[1] if len(ranked) > 1 else None
    return dict(pose=pose, fit=fit2, n_obs=n_obs, information=info, status=0, assignment=asg,
                hypothesis=np.array([h, second[1] if second else -1], dtype=np.int32), cost=np.array([J, second[0] if second else nan]))


def refine_assignments_views(obs, views, tab, pose, assignment, n_obj, model, type_count, sigma_px=0.25, iters=6, damping=1e-9, fit=pose_spec.fit_kabsch, diags=None):
    """Whole tensors -> {"pose" [B,max_obj,12], "fit" [..,2], "n_obs" [B,max_obj] int32, "information" [..,36], "status" [B,max_obj] int32,
    "assignment" [..,S] int32, "hypothesis" [..,2] int32, "cost" [..,2]}.  diags (a dict) receives {(b, o): diag} for the live objects."""
    B, max_obj, S = tab.shape[:3]
    assert model.shape == (S, 3) and S == 1 + sum(type_count) and obs.shape[:3] == (B, max_obj, S)
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 2), np.nan), "n_obs": np.zeros((B, max_obj), dtype=np.int32),
           "information": np.full((B, max_obj, 36), np.nan), "status": np.full((B, max_obj), SKIPPED, dtype=np.int32),
           "assignment": np.full((B, max_obj, S), -1, dtype=np.int32), "hypothesis": np.full((B, max_obj, 2), -1, dtype=np.int32), "cost": np.full((B, max_obj, 2), np.nan)}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            d = {} if diags is not None else None
            got = refine_object(obs[b, o], views, tab[b, o], pose[b, o], assignment[b, o], model, type_count, sigma_px, iters, damping, fit=fit, diag=d)
            for key, value in got.items():
                out[key][b, o] = value
            if diags is not None:
                diags[(b, o)] = d
    return out
