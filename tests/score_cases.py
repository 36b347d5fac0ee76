"""Inputs for okp_score_objects: seeded scenes at the three shapes that reach both edges of every lane loop, and built edge cases whose
decisions are exact (ties from exactly representable coordinates, a coordinate equal to max_range, a log filled to the last record).
A case is a dict of NumPy arrays and host scalars; score_spec.score takes it through run_spec.  No GPU and no product code here."""
import numpy as np

import score_spec

FISHEYE = (60.0, 60.0, 32.0, 32.0, -0.02, 0.01, -0.003, 0.0004, 0.0)
FISHEYE_SIZE = (64.0, 64.0)
RADTAN = (420.0, 415.0, 320.0, 240.0, -0.28, 0.07, 0.0006, -0.0002, 1.0)
RADTAN_SIZE = (480.0, 640.0)                                        # image_size as the camera holds it: (height, width)
SHAPES = {"tiny": (1, 1, 1, 2, 0), "small": (3, 3, 4, 4, 1), "wide": (2, 64, 64, 16, 4)}     # (B, G, max_obj, S, P)


def _rotation(rng, max_angle):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.0, max_angle)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _pose_row(R, t):
    return np.concatenate([R, np.asarray(t, dtype=np.float64)[:, None]], axis=1).reshape(12)


def seeded(shape, seed, cam=None, size=None, no_centre=True):
    """A random scene: labelled objects on a jittered grid in front of the camera, detections near them with dropped, unlifted and
    out-of-range slots, and P pose sets (0, 1: row o; 2, 3: through an index with -1 and out-of-range entries, and a NaN row)."""
    B, G, max_obj, S, P = shape
    rng = np.random.default_rng(seed)
    model = rng.uniform(-0.03, 0.03, (S, 3))
    model[0] = 0.0
    side = int(np.ceil(np.sqrt(G)))
    pitch = min(0.09, 0.6 / side)
    truth = np.full((B, G, S, 4), -5.0)                             # (the fourth value is never read)
    truth_pose = np.zeros((B, G, 12))
    tab = np.full((B, max_obj, S, 4), np.nan)
    est = np.full((B, max_obj, 12), np.nan)
    n_obj, n_truth = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n_truth[b] = G if b % 2 == 0 else max(G - 1, 1)
        n_obj[b] = max_obj if b == 0 else int(rng.integers(1, max_obj + 1))
        for g in range(G):
            c = np.array([(g % side - (side - 1) / 2.0) * pitch, (g // side - (side - 1) / 2.0) * pitch, 0.0]) + rng.uniform(-0.01, 0.01, 3)
            c[2] = rng.uniform(0.9, 1.4)
            Rg = _rotation(rng, np.pi)
            truth_pose[b, g] = _pose_row(Rg, c)
            truth[b, g, :, :3] = model @ Rg.T + c
        order = rng.permutation(int(n_truth[b]))
        for o in range(max_obj):
            if o >= n_obj[b]:
                tab[b, o] = 0.5                                     # rows past n_obj are never read, whatever they hold
                est[b, o] = 0.25
                continue
            g = int(order[o % len(order)])
            Rg, c = truth_pose[b, g].reshape(3, 4)[:, :3], truth_pose[b, g].reshape(3, 4)[:, 3]
            Re, te = Rg @ _rotation(rng, 0.2), c + rng.normal(0.0, 0.004, 3)
            est[b, o] = _pose_row(Re, te)
            tab[b, o, :, :3] = model @ Re.T + te + rng.normal(0.0, 0.002, (S, 3))
            tab[b, o, :, 3] = rng.uniform(0.5, 1.0, S)
            for s in range(1, S):
                u = rng.uniform()
                if u < 0.1:
                    tab[b, o, s] = np.nan                           # absent
                elif u < 0.2:
                    tab[b, o, s, :3] = np.nan                       # detected, not lifted
                elif u < 0.25:
                    tab[b, o, s, 2] = 2.5                           # beyond range
            if no_centre and rng.uniform() < 0.05:
                tab[b, o, 0] = np.nan
    sets = []
    for p in range(P):
        if p < 2:
            pose = est.copy() if p == 0 else est + rng.normal(0.0, 0.003, est.shape)
            sets.append((pose, None))
            continue
        rows = max(2, max_obj // 2) if p == 2 else max_obj + 3
        pose = np.zeros((B, rows, 12))
        for b in range(B):
            for r in range(rows):
                tp = truth_pose[b, r % G].reshape(3, 4)
                pose[b, r] = _pose_row(tp[:, :3] @ _rotation(rng, 0.1), tp[:, 3] + rng.normal(0.0, 0.003, 3))
        pose[0, 1, 5] = np.nan
        index = rng.integers(-1, rows + (2 if p == 3 else 0), (B, max_obj)).astype(np.int32)
        sets.append((pose, index))
    return {"tab": tab, "n_obj": n_obj, "truth": truth, "n_truth": n_truth, "cam": cam, "size": size, "sets": sets, "truth_pose": truth_pose if P else None,
            "model": model if P else None, "match_radius": np.inf, "max_range": 2.0, "cap_kp": B * max_obj * S + 8, "cap_pose": B * max_obj + 8}


def _blank(B, G, max_obj, S):
    return np.full((B, max_obj, S, 4), np.nan), np.zeros((B, G, S, 4)), np.zeros((B, G, 12))


def _object(truth, truth_pose, b, g, rows, R=np.eye(3)):
    truth[b, g, :, :3] = rows
    truth_pose[b, g] = _pose_row(R, rows[0])


def edges_match():
    """(3, 3, 4, 4, 1), fisheye, match_radius 0.5.  Frame 0: an empty centre slot; an exact tie in the match (lowest g) and in the nearest
    row (lowest j); a coordinate equal to max_range, a finite confidence with NaN X, Y, Z, an absent slot; a detection the radius excludes.
    Frame 1: n_obj = 0.  Frame 2: n_truth = 0."""
    tab, truth, truth_pose = _blank(3, 3, 4, 4)
    for b in range(3):
        _object(truth, truth_pose, b, 0, np.array([[-0.25, 0.0, 1.0], [-0.5, 0.125, 1.0], [-0.5, -0.125, 1.0], [-0.25, 0.25, 1.0]]))
        _object(truth, truth_pose, b, 1, np.array([[0.25, 0.0, 1.0], [0.25, 0.125, 1.0], [0.375, 0.0, 1.0], [0.25, -0.125, 1.0]]))
        _object(truth, truth_pose, b, 2, np.array([[0.0, -0.5, 1.5], [0.0625, -0.5, 1.5], [0.0, -0.4375, 1.5], [0.0, -0.5, 1.5625]]))
    tab[0, 0, 1:] = [[0.25, 0.125, 1.0, 1.0]] * 3                                       # centre slot empty, the others full
    tab[0, 1] = [[0.0, 0.125, 1.0, 1.0], [-0.5, 0.0, 1.0, 1.0], [-0.25, 0.25, 1.0078125, 1.0], [-0.25, 0.0, 1.0, 0.5]]    # ties: g 0 == g 1; rows 1 == 2
    tab[0, 2] = [[0.0, -0.5, 1.5, 1.0], [0.0625, -0.5, 2.0, 1.0], [np.nan, np.nan, np.nan, 0.75], [np.nan, np.nan, np.nan, np.nan]]
    tab[0, 3] = [[0.0, 0.375, 1.0, 1.0]] * 4                                            # 0.4507 from g 0 and g 1: inside; see below
    tab[0, 3, :, 1] = 0.75                                                              # sqrt(0.0625 + 0.5625) = 0.79 > 0.5: excluded
    tab[2, 0] = [[0.25, 0.0, 1.0, 1.0]] * 4
    tab[2, 1] = [[-0.25, 0.0, 1.0, 1.0]] * 4
    pose = np.zeros((3, 4, 12))
    pose[:] = _pose_row(np.eye(3), [0.0, 0.0, 1.0])
    return {"tab": tab, "n_obj": np.array([4, 0, 2], np.int32), "truth": truth, "n_truth": np.array([3, 3, 0], np.int32), "cam": FISHEYE,
            "size": FISHEYE_SIZE, "sets": [(pose, None)], "truth_pose": truth_pose, "model": np.array(truth[0, 0, :, :3] - truth[0, 0, 0, :3]),
            "match_radius": 0.5, "max_range": 2.0, "cap_kp": 64, "cap_pose": 16}


def edges_view(cam=FISHEYE, size=FISHEYE_SIZE):
    """(3, 3, 4, 4, 1).  Frame 0: a truth centre out of view, a truth row out of view, a truth centre behind the camera.  Frame 1: an index of
    -1, an index >= rows, a NaN pose, R_est == R_gt (0 degrees).  Frame 2: a half turn (180 degrees)."""
    tab, truth, truth_pose = _blank(3, 3, 4, 4)
    far = 1.25 if cam is FISHEYE else 1.0                                               # x / z of a point beyond the right border
    edge, out = (0.5, 0.75) if cam is FISHEYE else (0.3125, 0.5)                        # a centre inside, a row of it outside
    model = np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0], [0.0, 0.0, 0.0625]])
    for b in range(3):
        _object(truth, truth_pose, b, 0, model + [far, 0.0, 1.0])
        rows = model + [edge, 0.0, 1.0]
        rows[2] = [out, 0.0, 1.0]
        _object(truth, truth_pose, b, 1, rows)
        _object(truth, truth_pose, b, 2, model + [0.0, 0.25, 1.0])
    truth[0, 2, :, 2] = -1.0                                                            # frame 0: object 2 is behind the camera
    tab[0, 0] = np.concatenate([model + [far, 0.0, 1.0], np.ones((4, 1))], axis=1)      # -> out_of_view
    tab[0, 1] = np.concatenate([truth[0, 1, :, :3] + [0.0, 0.0, 0.0078125], np.ones((4, 1))], axis=1)       # slot 2 -> truth_hidden
    tab[0, 2] = np.concatenate([model + [0.0, 0.25, -1.0], np.ones((4, 1))], axis=1)    # -> out_of_view by z <= 0
    half = np.diag([1.0, -1.0, -1.0])
    for o in range(4):
        tab[1, o] = np.concatenate([model + [0.0, 0.25, 1.0] + [0.0, 0.0, 0.015625 * o], np.ones((4, 1))], axis=1)
    tab[2, 0] = tab[1, 0]
    pose = np.zeros((3, 3, 12))
    pose[:, 0] = _pose_row(np.eye(3), [0.0, 0.25, 1.0])                                 # == the truth's pose of object 2
    pose[:, 1] = np.nan
    pose[:, 2] = _pose_row(half, [0.0, 0.25, 1.0])
    index = np.array([[0, 0, 0, 0], [-1, 3, 1, 0], [2, 0, 0, 0]], np.int32)
    return {"tab": tab, "n_obj": np.array([3, 4, 1], np.int32), "truth": truth, "n_truth": np.array([3, 3, 3], np.int32), "cam": cam, "size": size,
            "sets": [(pose, index)], "truth_pose": truth_pose, "model": model, "match_radius": np.inf, "max_range": 2.0, "cap_kp": 64, "cap_pose": 16}


def run_spec(case, log=None, calls=1):
    """The case through the specification `calls` times -> (log, match, nearest)."""
    log = score_spec.new_log(case["cap_kp"], case["cap_pose"]) if log is None else log
    for _ in range(calls):
        match, nearest = score_spec.score(log, case["tab"], case["n_obj"], case["truth"], case["n_truth"], case["match_radius"], case["max_range"], case["cam"],
                                          case["size"], case["sets"], case["truth_pose"], case["model"])
    return log, match, nearest


def with_capacity(case, slack_kp, slack_pose, calls=1):
    """The case with logs that hold exactly its records of `calls` calls plus the given slack (negative: that many records do not fit)."""
    log, _, _ = run_spec(dict(case, cap_kp=1 << 20, cap_pose=1 << 20), calls=calls)
    return dict(case, cap_kp=int(log["counts"][score_spec.KP_WRITTEN]) + slack_kp, cap_pose=int(log["counts"][score_spec.POSE_WRITTEN]) + slack_pose)


def all_cases():
    cases = {
        "tiny_no_camera": seeded(SHAPES["tiny"], 11),
        "small_fisheye": seeded(SHAPES["small"], 12, FISHEYE, FISHEYE_SIZE),
        "small_no_camera": seeded(SHAPES["small"], 13),
        "wide_radtan": seeded(SHAPES["wide"], 14, RADTAN, RADTAN_SIZE),
        "wide_no_camera": seeded(SHAPES["wide"], 15),
        "edges_match": edges_match(),
        "edges_view_fisheye": edges_view(),
        "edges_view_radtan": edges_view(RADTAN, RADTAN_SIZE),
    }
    cases["small_radius"] = dict(seeded(SHAPES["small"], 16, FISHEYE, FISHEYE_SIZE), match_radius=0.003)
    cases["small_exactly_full"] = with_capacity(cases["small_fisheye"], 0, 0)
    cases["small_one_over"] = with_capacity(cases["small_fisheye"], -1, 0)
    cases["small_pose_one_over"] = with_capacity(cases["small_fisheye"], 0, -1)
    return cases


RESULTS_CASES = ("tiny", "small", "wide")          # seeded scenes with every centre present, for the comparison with evaluation.Results


def results_case(name):
    cam, size = (RADTAN, RADTAN_SIZE) if name == "wide" else (FISHEYE, FISHEYE_SIZE)
    return seeded(SHAPES[name], 21 + len(name), cam, size, no_centre=False)


def input_margins(case):
    """What the device's rounding could decide instead of the specification's, as the least margin of each kind over the case:
    "border_px": distance of a truth projection from a frame border (inf without camera); "z": |z| of a truth row; "decision_m2": the gap
    in squared distance behind a match or a nearest row that is not an exact tie, and between a match and match_radius^2."""
    out = {"border_px": np.inf, "z": np.inf, "decision_m2": np.inf}
    B, max_obj, S = case["tab"].shape[:3]
    r2 = case["match_radius"] ** 2
    with np.errstate(all="ignore"):
        for b in range(B):
            nt = min(max(int(case["n_truth"][b]), 0), case["truth"].shape[1])
            rows = case["truth"][b, :nt, :, :3].reshape(-1, 3)
            for p in rows:
                out["z"] = min(out["z"], abs(p[2]))
                if case["cam"] is not None:
                    u, v = score_spec.project(case["cam"], p)
                    out["border_px"] = min(out["border_px"], abs(u), abs(v), abs(u - case["size"][0]), abs(v - case["size"][1]))
            for o in range(min(max(int(case["n_obj"][b]), 0), max_obj)):
                c = case["tab"][b, o, 0]
                if not np.isfinite(c).all() or nt == 0:
                    continue
                d2 = np.sort((case["truth"][b, :nt, 0, 0] - c[0]) ** 2 + (case["truth"][b, :nt, 0, 1] - c[1]) ** 2)
                gaps = [d2[1] - d2[0]] if nt > 1 else []
                if np.isfinite(r2):
                    gaps.append(abs(d2[0] - r2))
                g = int(np.argmin((case["truth"][b, :nt, 0, 0] - c[0]) ** 2 + (case["truth"][b, :nt, 0, 1] - c[1]) ** 2))
                for s in range(S):
                    p = case["tab"][b, o, s]
                    if np.isfinite(p).all() and S > 1:
                        e2 = np.sort(((case["truth"][b, g, :, :3] - p[:3]) ** 2).sum(axis=1))
                        gaps.append(e2[1] - e2[0])
                for gap in gaps:
                    if gap != 0.0:                       # an exact tie is decided by the order, on the device as in the specification
                        out["decision_m2"] = min(out["decision_m2"], gap)
    return out
