"""NumPy statement of the object pose stage (okp_object_points, okp_rig_object_points, okp_object_pose), written from the specification in
include/okp.h - not from the kernels: the table builders as plain loops, the hypotheses by itertools.permutations, the fit by Kabsch
(np.linalg.svd with the determinant correction), the rmse from the residuals, the status rules.  fit_horn() is a second, independent
formulation of the same fit (Horn's 4 x 4 matrix, np.linalg.eigh); tests/test_object_pose_args.py holds the two together."""
import itertools

import numpy as np

MAX_POINTS, MAX_HYPOTHESES, DEGENERACY = 16, 1024, 1e-12
FEW, DEGENERATE, POOR = 1, 2, 4


def slots(type_count):
    """[(type k, index j)] of the S = 1 + sum(type_count) slots / model rows: the centre, then c_k per type."""
    return [(0, 0)] + [(k + 1, j) for k, c in enumerate(type_count) for j in range(c)]


def model_of(points_3d, type_count):
    """Rows 1.. the key points in type order, row 0 their mean."""
    pts = np.asarray(points_3d, dtype=np.float64)
    assert pts.shape == (sum(type_count), 3)
    return np.concatenate([pts.mean(axis=0)[None], pts])


# ---- the table builders ------------------------------------------------------------------------------------------------------------------

def object_points(points, sel, n_obj, n_votes, reduced, type_count, lift=None):
    """points [n,K,cap,4], sel [n,max_obj,K-1,max_sel], n_obj [n], n_votes [n,max_obj,K-1], reduced [n,max_obj,K-1,max_sel,2] or None ->
    tab [n,max_obj,S,4].  lift(f, k, xy [c,2] float32) -> [c,3]: the lifting of okp_lift_peaks through depth map (f, k), for reduced types."""
    n, K, cap, _ = points.shape
    max_obj = sel.shape[1]
    sl = slots(type_count)
    tab = np.full((n, max_obj, len(sl), 4), np.nan)
    for f in range(n):
        for o in range(min(int(n_obj[f]), max_obj)):
            for s, (k, j) in enumerate(sl):
                if k == 0:
                    peak = o
                else:
                    c = type_count[k - 1]
                    if reduced is not None and c > 1 and n_votes[f, o, k - 1] > c:
                        xy = reduced[f, o, k - 1, j]
                        if not np.isnan(xy).any():
                            tab[f, o, s, :3] = lift(f, k, xy[None].astype(np.float32))[0]
                            tab[f, o, s, 3] = 1.0
                        continue
                    peak = int(sel[f, o, k - 1, j])
                if 0 <= peak < cap:
                    tab[f, o, s] = points[f, k, peak]
    return tab


def rig_object_points(fused, n_fused, obj, type_count):
    """fused [K,cap_f,4], n_fused [K], object [K,cap_f] (okp_rig_fuse) -> tab [1,cap_f,S,4]."""
    K, cap_f, _ = fused.shape
    sl = slots(type_count)
    tab = np.full((1, cap_f, len(sl), 4), np.nan)
    for o in range(min(int(n_fused[0]), cap_f)):
        for s, (k, j) in enumerate(sl):
            if k == 0:
                tab[0, o, s] = fused[0, o]
                continue
            mine = [c for c in range(min(int(n_fused[k]), cap_f)) if obj[k, c] == o]
            if j < len(mine):
                tab[0, o, s] = fused[k, mine[j]]
    return tab


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------

def second_eigenvalue_ratio(pts):
    """Second-largest eigenvalue of the scatter of the centred points over its trace (0 for coincident points)."""
    p = np.asarray(pts, dtype=np.float64)
    p = p - p.mean(axis=0)
    trace = float((p * p).sum())
    e = np.linalg.eigvalsh(p.T @ p)
    return (float(e[1]) / trace) if trace > 0.0 else 0.0


def degenerate(pts):
    p = np.asarray(pts, dtype=np.float64)
    p = p - p.mean(axis=0)
    return not np.linalg.eigvalsh(p.T @ p)[1] > DEGENERACY * float((p * p).sum())


def fit_kabsch(m, p):
    """min over proper rotations of sum |R (m - m_bar) - (p - p_bar)|^2 -> (R, t, rmse, cost); rmse and cost from the residuals."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    mb, pb = m.mean(axis=0), p.mean(axis=0)
    U, _, Vt = np.linalg.svd((p - pb).T @ (m - mb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    t = pb - R @ mb
    res = m @ R.T + t - p
    cost = float((res * res).sum())
    return R, t, float(np.sqrt(cost / len(m))), cost


def fit_horn(m, p):
    """The same minimum by Horn's closed form: the unit quaternion is the eigenvector of the largest eigenvalue of the 4 x 4 matrix of the
    correlation M = sum (m - m_bar)(p - p_bar)^T."""
    m, p = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    mb, pb = m.mean(axis=0), p.mean(axis=0)
    M = (m - mb).T @ (p - pb)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (y * x + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (z * x - w * y), 2 * (z * y + w * x), w * w - x * x - y * y + z * z]])
    t = pb - R @ mb
    res = m @ R.T + t - p
    cost = float((res * res).sum())
    return R, t, float(np.sqrt(cost / len(m))), cost


def hypotheses(filled, type_count):
    """filled: bool [S].  The hypotheses in index order: each a list of model rows, one per filled slot in slot order.  Per type the injective
    maps of its filled slots onto its instances in lexicographic order; mixed radix, type 1 the slowest digit (itertools.product varies the
    last factor fastest; itertools.permutations(range(c), n) is lexicographic)."""
    per_type = [[(0,)] if filled[0] else [()]]
    base = 1
    for c in type_count:
        n_k = int(np.count_nonzero(filled[base:base + c]))
        per_type.append([tuple(base + a for a in perm) for perm in itertools.permutations(range(c), n_k)])
        base += c
    return [[row for part in combo for row in part] for combo in itertools.product(*per_type)]


def object_pose(tab, n_obj, model, type_count, max_rmse=np.inf, fit=fit_kabsch):
    """-> dict of pose [B,max_obj,12], fit [B,max_obj,2], assignment [B,max_obj,S] int32, used, status [B,max_obj] int32, and (for the tests'
    own conditions, not an output of the entry point) costs: {(b, o): sorted costs of all hypotheses}."""
    tab, model = np.asarray(tab, dtype=np.float64), np.asarray(model, dtype=np.float64)
    B, max_obj, S, _ = tab.shape
    assert model.shape == (S, 3) and S == 1 + sum(type_count)
    out = {"pose": np.full((B, max_obj, 12), np.nan), "fit": np.full((B, max_obj, 2), np.nan),
           "assignment": np.full((B, max_obj, S), -1, dtype=np.int32), "used": np.zeros((B, max_obj), dtype=np.int32),
           "status": np.zeros((B, max_obj), dtype=np.int32), "costs": {}}
    for b in range(B):
        for o in range(min(int(np.reshape(n_obj, -1)[b]), max_obj)):
            rows = tab[b, o]
            filled = np.isfinite(rows).all(axis=1)
            used = int(filled.sum())
            out["used"][b, o] = used
            if used < 3:
                out["status"][b, o] = FEW
                continue
            p = rows[filled, :3]
            if degenerate(p):
                out["status"][b, o] = DEGENERATE
                continue
            hyps = hypotheses(filled, type_count)
            assert 1 <= len(hyps) <= MAX_HYPOTHESES
            fits = [fit(model[h], p) for h in hyps]
            order = sorted(range(len(hyps)), key=lambda i: (fits[i][3], i))
            out["costs"][(b, o)] = [fits[i][3] for i in order]
            win = order[0]
            out["assignment"][b, o, np.flatnonzero(filled)] = hyps[win]
            if degenerate(model[hyps[win]]):
                out["status"][b, o] = DEGENERATE
                continue
            R, t, rmse, _ = fits[win]
            out["pose"][b, o] = np.concatenate([R, t[:, None]], axis=1).reshape(12)
            out["fit"][b, o, 0] = rmse
            if len(order) > 1:
                out["fit"][b, o, 1] = fits[order[1]][2]
            out["status"][b, o] = POOR if rmse > max_rmse else 0
    return out
