"""okp_score_objects in NumPy, written from the comment in include/okp.h: one statement per sentence of the specification, explicit
associations (every product and sum is one fp64 operation in the order written), the log's order and its overflow rule.  The view test
projects with the host cameras' formulae; the device compiles the same formulae with contraction, which is why the GPU cases keep every
projection away from a border (score_cases.input_margins)."""
import numpy as np

MAX_POSES = 4
OVERFLOW = 1
(CALLS, FRAMES, DETECTIONS, NO_CENTRE, UNMATCHED, OUT_OF_VIEW, POINTS, MISSING, ABSENT, TRUTH_HIDDEN, TRUTH_VISIBLE, TRUTH_DETECTED, KP_WRITTEN,
 POSE_WRITTEN, OVERFLOW_WORD) = range(15)


def new_log(cap_kp, cap_pose):
    """All zeros is a valid empty log."""
    return {"kp_err": np.zeros((cap_kp, 2)), "kp_id": np.zeros((cap_kp, 4), np.int32), "pose_err": np.zeros((cap_pose, MAX_POSES, 3)),
            "pose_id": np.zeros((cap_pose, 4), np.int32), "counts": np.zeros(16, np.int64)}


def project(cam, p):
    """cam = (fx, fy, cx, cy, d0..d3, model): a camera-frame point -> raw pixels (u, v); the division by Z is unguarded, as in the reference."""
    fx, fy, cx, cy, d0, d1, d2, d3, model = cam
    with np.errstate(all="ignore"):
        a, b = p[0] / p[2], p[1] / p[2]
        if int(model) == 1:
            r2 = a * a + b * b
            radial = 1 + d0 * r2 + d1 * r2 * r2
            u = a * radial + 2 * d2 * a * b + d3 * (r2 + 2 * a * a)
            v = b * radial + d2 * (r2 + 2 * b * b) + 2 * d3 * a * b
        else:
            r = np.sqrt(a * a + b * b)
            theta = np.arctan(r)
            t2 = theta * theta
            theta_d = theta * (1 + d0 * t2 + d1 * t2 * t2 + d2 * t2 * t2 * t2 + d3 * t2 * t2 * t2 * t2)
            sc = theta_d / r if r > 1e-8 else 1.0
            u, v = a * sc, b * sc
        return fx * u + cx, fy * v + cy


def in_view(cam, size, p):
    """Step 3's test of one truth row; without a camera every row is in view."""
    if cam is None:
        return True
    u, v = project(cam, p)
    return bool(p[2] > 0.0 and 0.0 < u < size[0] and 0.0 < v < size[1])


def pose_errors(E, T, model):
    """Step 5: (rotation in degrees, centre error, model rmse) of the pose row E [12] against the truth's T [12]; all NaN where either is not finite."""
    if not (np.isfinite(E).all() and np.isfinite(T).all()):
        return np.full(3, np.nan)
    R, t, Rg, tg = E.reshape(3, 4)[:, :3], E.reshape(3, 4)[:, 3], T.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, 3]
    Q = np.array([[(Rg[0, a] * R[0, c] + Rg[1, a] * R[1, c]) + Rg[2, a] * R[2, c] for c in range(3)] for a in range(3)])
    w = (Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1])
    s = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    theta = np.arctan2(s * 0.5, (((Q[0, 0] + Q[1, 1]) + Q[2, 2]) - 1.0) * 0.5)
    total = centre = None
    for i, m in enumerate(model):
        d = [(((R[r, 0] * m[0] + R[r, 1] * m[1]) + R[r, 2] * m[2]) + t[r]) - (((Rg[r, 0] * m[0] + Rg[r, 1] * m[1]) + Rg[r, 2] * m[2]) + tg[r]) for r in range(3)]
        e = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        if i == 0:
            centre, total = np.sqrt(e), e
        else:
            total = total + e
    return np.array([theta * 57.29577951308232, centre, np.sqrt(total / float(len(model)))])


def score(log, tab, n_obj, truth, n_truth, match_radius=np.inf, max_range=2.0, cam=None, size=None, sets=(), truth_pose=None, model=None):
    """One call: appends to `log` in place and returns (match [B,max_obj], nearest [B,max_obj,S]).  sets: [(pose [B,rows,12], index [B,max_obj] or None)]."""
    B, max_obj, S = tab.shape[:3]
    G = truth.shape[1]
    counts = log["counts"]
    cap_kp, cap_pose = len(log["kp_err"]), len(log["pose_err"])
    step = int(counts[CALLS])
    radius2 = float(match_radius) * float(match_radius)          # formed once
    match = np.full((B, max_obj), -4, np.int32)
    nearest = np.full((B, max_obj, S), -1, np.int32)
    kp_records, pose_records = [], []                            # in (b, o, s) order
    P = len(sets)
    with np.errstate(all="ignore"):
        for b in range(B):
            n = min(max(int(n_obj[b]), 0), max_obj)
            nt = min(max(int(n_truth[b]), 0), G)
            seen = [in_view(cam, size, truth[b, g, 0, :3]) for g in range(nt)]
            detected = [False] * nt
            for o in range(n):
                centre = tab[b, o, 0]
                if not np.isfinite(centre).all():                                       # 1
                    counts[NO_CENTRE] += 1
                    match[b, o] = -1
                    continue
                best, gs = np.inf, -1                                                   # 2
                for g in range(nt):
                    dx, dy = centre[0] - truth[b, g, 0, 0], centre[1] - truth[b, g, 0, 1]
                    d2 = dx * dx + dy * dy
                    if d2 < best:
                        best, gs = d2, g
                if gs < 0 or best > radius2:
                    counts[UNMATCHED] += 1
                    match[b, o] = -2
                    continue
                if not seen[gs]:                                                        # 3
                    counts[OUT_OF_VIEW] += 1
                    match[b, o] = -3
                    continue
                match[b, o] = gs
                counts[DETECTIONS] += 1
                detected[gs] = True
                for s in range(S):                                                      # 4
                    x, y, z, conf = tab[b, o, s]
                    if not np.isfinite(conf):
                        counts[ABSENT] += 1
                        continue
                    if not (np.isfinite([x, y, z]).all() and x < max_range and y < max_range and z < max_range):
                        counts[POINTS] += 1
                        counts[MISSING] += 1
                        continue
                    best, best_xy, js = np.inf, 0.0, -1
                    for j in range(S):
                        dx, dy, dz = x - truth[b, gs, j, 0], y - truth[b, gs, j, 1], z - truth[b, gs, j, 2]
                        dxy = dx * dx + dy * dy
                        d2 = dxy + dz * dz
                        if d2 < best:
                            best, best_xy, js = d2, dxy, j
                    nearest[b, o, s] = js
                    if js < 0 or not in_view(cam, size, truth[b, gs, js, :3]):
                        counts[TRUTH_HIDDEN] += 1
                        continue
                    counts[POINTS] += 1
                    kp_records.append(((np.sqrt(best), np.sqrt(best_xy)), (step, b, o, s)))
                if P > 0:                                                               # 5
                    triples = np.full((MAX_POSES, 3), np.nan)
                    for p, (pose, index) in enumerate(sets):
                        row = int(index[b, o]) if index is not None else o
                        if 0 <= row < pose.shape[1]:
                            triples[p] = pose_errors(pose[b, row], truth_pose[b, gs], model)
                    pose_records.append((triples, (step, b, o, gs)))
            counts[TRUTH_VISIBLE] += sum(seen)                                          # 6
            counts[TRUTH_DETECTED] += sum(1 for g in range(nt) if seen[g] and detected[g])
    for records, err, ids, cursor, cap in ((kp_records, log["kp_err"], log["kp_id"], KP_WRITTEN, cap_kp),
                                           (pose_records, log["pose_err"], log["pose_id"], POSE_WRITTEN, cap_pose)):
        pos = int(counts[cursor])
        for value, ident in records:
            if pos < cap:
                err[pos], ids[pos] = value, ident
            pos += 1                                     # a record that does not fit is dropped, and so are all after it
        if pos > cap:
            counts[OVERFLOW_WORD] |= OVERFLOW
        counts[cursor] = min(pos, cap)
    counts[CALLS] += 1
    counts[FRAMES] += B
    return match, nearest


def summary_keypoints(log):
    """Results.summary() (perception/evaluation.py) from a log: the same keys from the same NumPy calls."""
    c = log["counts"]
    n, written = int(c[POINTS]), int(c[KP_WRITTEN])
    if n == 0 or written == 0:
        return {"points": n, "missing": 100.0 if n else 0.0}
    err, err_xy = np.asarray(log["kp_err"])[:written, 0], np.asarray(log["kp_err"])[:written, 1]
    cm, cm_xy = np.array(err) * 100.0, np.array(err_xy) * 100.0
    q25, q75 = np.percentile(cm, [25, 75])
    return {"mean": float(cm.mean()), "mean xy": float(cm_xy.mean()), "std": float(cm.std()), "< 3cm": float((np.array(err) < 0.03).sum()) / n,
            "25th percentile": float(q25), "75th percentile": float(q75), "missing": 100.0 * int(c[MISSING]) / n, "points": n}
