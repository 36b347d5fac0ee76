"""The fabricated cases of the tests of okp_rig_bearings and okp_refine_pose_views, as plain arrays.  The CPU tests
(tests/test_refine_views_args.py) assert on the inputs, through the NumPy specification (tests/refine_views_spec.py), that every case is away
from every decision of the stage; the GPU tests (tests/test_gpu_refine_views.py) compare the device with the specification on the same cases.

Refinement cases: V cameras of a rig around the origin of the table's frame, objects of a random model at 0.6 .. 1.4 m in front of them, every
model point seen by every camera along its exact bearing plus 0.1 map pixels of noise, then views (and whole slots) taken away at random; the
start is the true pose moved by 0.05 rad and 2 cm.  The "crafted" case is built directly, one object per status.
Bearings cases: random peaks, matches, members and clusters that keep the rules of okp_rig_fuse's outputs where the contract relies on them
(one member of a cluster per pair, members are matched) and break them where it says what happens (more clusters of an object than its type
has instances, clusters past n_fused, slots past the count)."""
import numpy as np

import object_pose_cases as pc
import refine_cases as rc
import refine_views_spec as spec

F = 62.0                  # a 64 x 64 map of a camera with a 55 degree field of view
DEFAULTS = dict(sigma_px=0.25, iters=6, damping=1e-9)


def _yaw(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def rig(P, baseline=0.1, spread=np.radians(30.0), jitter=None):
    """P stereo pairs whose left cameras stand on a 0.4 m arc, yawed -spread .. +spread towards the scene, each right camera `baseline` to the
    right of its left one -> (T_BL [P,4,4], T_RL [P,4,4]).  jitter (a Generator): a centimetre and a degree of individual calibration."""
    T_BL, T_RL = np.stack([np.eye(4)] * P), np.stack([np.eye(4)] * P)
    for p in range(P):
        a = 0.0 if P == 1 else -spread + 2.0 * spread * p / (P - 1)
        T_BL[p, :3, :3] = _yaw(-a)
        T_BL[p, :3, 3] = [0.4 * np.sin(a) * 0.5, 0.02 * (p % 3 - 1), 0.0]
        T_RL[p, :3, 3] = [-baseline, 0.0, 0.0]
        if jitter is not None:
            dR, dt = rc.perturbation(jitter, np.radians(1.0), 0.01)
            T_RL[p, :3, :3], T_RL[p, :3, 3] = dR, T_RL[p, :3, 3] + dt
    return T_BL, T_RL


def views_of(V, seed=0):
    """The first V rows of the views table of a jittered rig of ceil(V / 2) pairs."""
    P = (V + 1) // 2
    T_BL, T_RL = rig(P, jitter=np.random.default_rng(1000 + seed))
    return spec.rig_views(T_BL, T_RL, np.full((2 * P, 2), F) * np.array([1.0, 1.02]))[:V]


def bearing(view, X):
    """The exact bearing of the table-frame point X in one view."""
    q = view[:12].reshape(3, 4)[:, :3] @ X + view[:12].reshape(3, 4)[:, 3]
    return q[0] / q[2], q[1] / q[2]


def scene(model, views, B, max_obj, seed, noise_px=0.1, miss=0.0, miss_slot=0.0, unassigned=0.0):
    """-> obs [B,max_obj,S,V,2], start pose [B,max_obj,12], assignment [B,max_obj,S], truth {(b, o): (R, t)}: every object of the table drawn."""
    rng = np.random.default_rng(seed)
    S, V = model.shape[0], views.shape[0]
    obs = np.full((B, max_obj, S, V, 2), np.nan)
    pose = np.full((B, max_obj, 12), np.nan)
    assignment = np.full((B, max_obj, S), -1, dtype=np.int32)
    truth = {}
    for b in range(B):
        for o in range(max_obj):
            R, t = pc.rotation(rng), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)])
            truth[(b, o)] = (R, t)
            for s in range(S):
                X = R @ model[s] + t
                gone = rng.random() < miss_slot
                for v in range(V):
                    u, w = bearing(views[v], X)
                    if not gone and not rng.random() < miss:
                        obs[b, o, s, v] = u + rng.normal() * noise_px / views[v, 12], w + rng.normal() * noise_px / views[v, 13]
            assignment[b, o] = np.where(rng.random(S) < unassigned, -1, np.arange(S))
            dR, dt = rc.perturbation(rng, 0.05, 0.02)
            pose[b, o] = np.concatenate([dR @ R, (t + dt)[:, None]], axis=1).reshape(12)
    return obs, pose, assignment, truth


def _case(name, obs, views, pose, assignment, n_obj, model, kind="scene", **params):
    return dict(name=name, obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.asarray(n_obj, dtype=np.int32), model=model, kind=kind,
                params=dict(DEFAULTS, **params))


def _scene_case(name, S, V, B, max_obj, n_obj, seed, model_seed=1, scale=0.1, **kw):
    params = {k: kw.pop(k) for k in list(kw) if k in DEFAULTS}
    model = pc.generic_model([1] * (S - 1), model_seed, scale=scale)
    views = views_of(V, seed)
    obs, pose, assignment, _ = scene(model, views, B, max_obj, seed, **kw)
    return _case(name, obs, views, pose, assignment, n_obj, model, **params)


# a seed of a search over far starts (`python tests/refine_views_cases.py --search`) whose single undamped step raises the cost in the
# specification - J goes from 4.4e4 to 5.5e4 - with every point at least 0.65 m in front of every camera before and after it (the first such
# seed, 1010, comes within 0.16 m of a camera plane)
REJECTED_SEED = 1014
CRAFTED_WANT = [0, 1, 1, 1, 1, 2, 4, 8, 1]


def _crafted_truth():
    return pc.rotation(np.random.default_rng(40)), np.array([0.05, -0.1, 1.0])


def crafted_case():
    """One object per status, built directly: B = 1, max_obj = 9, S = 4, V = 4, n_obj = 8; one undamped step."""
    rng = np.random.default_rng(41)
    model, S, V = rc.CRAFTED_MODEL, 4, 4
    views = views_of(V, seed=7)
    obs = np.full((1, 9, S, V, 2), np.nan)
    pose = np.full((1, 9, 12), np.nan)
    assignment = np.full((1, 9, S), -1, dtype=np.int32)

    def place(o, R, t, start_R=None, start_t=None):
        for s in range(S):
            for v in range(V):
                obs[0, o, s, v] = bearing(views[v], R @ model[s] + t)
        assignment[0, o] = np.arange(S)
        dR, dt = rc.perturbation(rng, 0.05, 0.02)
        pose[0, o] = np.concatenate([dR @ R if start_R is None else start_R, (t + dt if start_t is None else start_t)[:, None]], axis=1).reshape(12)

    R, t = _crafted_truth()
    place(0, R, t)                                                     # good: status 0
    place(1, R, t)
    pose[0, 1, 7] = np.inf                                             # a non-finite value in the pose: SKIPPED
    place(2, R, t)
    obs[0, 2, 1, 2, 1] = np.nan                                        # an entry with exactly one NaN half: SKIPPED
    place(3, R, t)
    obs[0, 3, 3, 0, 0] = np.inf                                        # an entry with an infinite half (in a slot without a model row, too): SKIPPED
    assignment[0, 3, 3] = -1
    place(4, R, t)
    assignment[0, 4, 0] = -1                                           # three rows, of which one has no observation left: two: SKIPPED
    obs[0, 4, 2] = np.nan
    # three model points on the x axis under R = I: a rotation about the axis moves nothing and H[0][0] is exactly 0: SINGULAR
    place(5, np.eye(3), np.array([0.0, 0.0, 1.0]), start_R=np.eye(3), start_t=np.array([0.0, 0.0, 1.0]))
    assignment[0, 5, 3] = -1
    place(6, R, t, start_R=R, start_t=np.array([0.05, -0.1, -0.5]))    # the start puts the object behind the cameras: BEHIND
    Rs, ts = rc.far_start(REJECTED_SEED, R)                            # a start far off, one undamped step: the cost goes up: REJECTED
    place(7, R, t, start_R=Rs, start_t=ts)
    pose[0, 8] = np.arange(12.0)                                       # beyond n_obj: finite garbage that is not read
    obs[0, 8] = 0.01
    assignment[0, 8] = np.arange(S)
    return dict(name="crafted_statuses", obs=obs, views=views, pose=pose, assignment=assignment, n_obj=np.array([8], dtype=np.int32), model=model, kind="crafted",
                params=dict(DEFAULTS, iters=1, damping=0.0), want=CRAFTED_WANT)


def cases():
    out = [_scene_case("v2_s4_one_object", 4, 2, 1, 1, [1], seed=70)]
    out.append(_scene_case("s5_v6", 5, 6, 1, 3, [3], seed=71))                      # 30 observations: below one wave of them
    out.append(_scene_case("s5_v14", 5, 14, 1, 3, [2], seed=72))                    # 70: just above
    out.append(_scene_case("s16_v64_full_iters16", 16, 64, 1, 2, [2], seed=73, model_seed=3, scale=0.2, iters=16))
    # more objects than one launch's first wave, a stream with none, finite objects past n_obj, views and whole slots missing, rows unassigned
    out.append(_scene_case("b3_obj64_n_0_5_64", 5, 8, 3, 64, [0, 5, 64], seed=74, miss=0.3, miss_slot=0.15, unassigned=0.1))
    out.append(_scene_case("iters1_mu0", 5, 8, 2, 4, [4, 3], seed=75, miss=0.2, iters=1, damping=0.0))
    return out


# ---- okp_rig_bearings ---------------------------------------------------------------------------------------------------------------------------

FISHEYE_D = (-0.02, 0.01, -0.004, 0.001)
RADTAN_D = (-0.28, 0.07, 0.0006, -0.0002)


def table_of(P, model=spec.EQUIDISTANT, d=FISHEYE_D, same=False):
    """P calibrations (the same one P times with same=True), each camera a little different from the next."""
    return [{"left": spec.camera(F + (0 if same else p), F * 1.01, 32.0 + (0 if same else 0.1 * p), 31.5, d, model),
             "right": spec.camera(F * 0.99, F - (0 if same else 0.5 * p), 31.0, 32.5, tuple(0.5 * v for v in d), model)} for p in range(P)]


def bearings_case(name, P, type_count, cap, cap_f, seed, table, fill=0.7, least=0):
    rng = np.random.default_rng(seed)
    K = 1 + len(type_count)
    count = rng.integers(least, cap + 3, size=(2 * P, K)).astype(np.int32)          # some maps hold more peaks than cap
    xyc = np.concatenate([rng.uniform(4.0, 60.0, size=(2 * P, K, cap, 2)), rng.uniform(0.3, 1.0, size=(2 * P, K, cap, 1))], axis=3).astype(np.float32)
    n_fused = rng.integers(1, cap_f + 1, size=K).astype(np.int32)
    n_fused[K - 1] = cap_f                                                          # one type fills its capacity
    n_obj = int(n_fused[0])
    obj = rng.integers(-1, n_obj, size=(K, cap_f)).astype(np.int32)                 # (also past n_fused[k]: rows that must not be read as clusters)
    obj[0] = np.where(np.arange(cap_f) < n_obj, np.arange(cap_f), -1)
    member = rng.integers(0, cap_f, size=(P, K, cap)).astype(np.int32)              # (past the count: garbage that must not be read as members)
    match = rng.integers(-1, cap, size=(P, K, cap)).astype(np.int32)
    for p in range(P):
        for k in range(K):
            nl, nr = min(int(count[2 * p, k]), cap), min(int(count[2 * p + 1, k]), cap)
            joined = rng.permutation(int(n_fused[k]))                               # a cluster holds at most one member per pair
            rights = rng.permutation(nr)
            at = 0
            for i in range(nl):
                if at < len(joined) and at < nr and rng.random() < fill:
                    member[p, k, i], match[p, k, i] = joined[at], rights[at]         # a member is a matched slot
                    at += 1
                else:
                    member[p, k, i] = -1
                    match[p, k, i] = -1 if rng.random() < 0.5 else (rights[at % nr] if nr else -1)          # unmatched, or matched and dropped at cap_f
    return dict(name=name, count=count, xyc=xyc, match=match, member=member, object=obj, n_fused=n_fused, table=table, type_count=list(type_count),
                shape=(P, K, cap, cap_f))


def bearings_cases():
    out = [bearings_case("p1_cap1", 1, [1], 1, 1, 80, table_of(1), fill=1.0, least=1)]
    out.append(bearings_case("p4_k3_cap8", 4, [1, 3], 8, 12, 81, table_of(4)))
    out.append(bearings_case("p32_cap32_capf64", 32, [2, 1], 32, 64, 82, table_of(32)))
    out.append(bearings_case("one_entry_table", 4, [1, 3], 8, 12, 83, table_of(1)))
    out.append(bearings_case("radtan_pair", 2, [1, 1, 1], 6, 8, 84, table_of(2, spec.RADTAN, RADTAN_D)))
    return out


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        c = crafted_case()
        R, _ = _crafted_truth()
        for seed in range(1000, 1030):
            Rs, ts = rc.far_start(seed, R)
            d = {}
            status = spec.refine_object(c["obs"][0, 0], c["views"], np.concatenate([Rs, ts[:, None]], axis=1).reshape(12), np.arange(4), c["model"], 0.25, 1, 0.0, diag=d)[4]
            print(seed, status, d.get("J_initial"), d.get("J_final"), d.get("min_qz"), d.get("pivot"))


# ---- the accuracy scene: a noisy rig tick through the repository's own specifications ----------------------------------------------------------

def triangulate(view_l, view_r, bl, br):
    """Linear two-view triangulation of one pair of bearings (no Hartley-Sturm correction) -> the point in the table's frame."""
    rows = []
    for view, (u, v) in ((view_l, bl), (view_r, br)):
        M = view[:12].reshape(3, 4)
        rows += [u * M[2] - M[0], v * M[2] - M[1]]
    X = np.linalg.svd(np.stack(rows))[2][-1]
    return X[:3] / X[3]


def noisy_rig_object(rng, model, type_count, T_BL, T_RL, table, noise_px):
    """One object in front of a rig, one tick of its own (so the correspondence is not in question): every key point seen by every camera at
    its projected pixel plus noise_px of Gaussian noise (stored as fp32 peaks) -> the tick's arrays (count, xyc, match, points) and (R, t)."""
    P, K = len(T_BL), 1 + len(type_count)
    R, t = pc.rotation(rng), np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.6, 1.4)])
    table = table * P if len(table) == 1 else table
    views = spec.rig_views(T_BL, T_RL, np.array([[c["fx"], c["fy"]] for e in table for c in (e["left"], e["right"])]))
    count = np.ones((2 * P, K), dtype=np.int32)
    xyc = np.zeros((2 * P, K, 1, 3), dtype=np.float32)
    for k in range(K):                                                            # (every type has one instance: slot = type)
        X = R @ model[k] + t
        for v in range(2 * P):
            cam = table[v // 2]["right" if v % 2 else "left"]
            M = views[v, :12].reshape(3, 4)
            px = spec.project(cam, M[:, :3] @ X + M[:, 3])
            xyc[v, k, 0] = px[0] + rng.normal() * noise_px, px[1] + rng.normal() * noise_px, 0.9
    match = np.zeros((P, K, 1), dtype=np.int32)
    points = np.zeros((P, K, 1, 4))
    for p in range(P):
        pair_views = spec.rig_views(np.eye(4)[None], T_RL[p][None], views[2 * p:2 * p + 2, 12:])      # the pair alone: its left camera is the frame
        for k in range(K):
            b = []
            for side, v in (("left", 2 * p), ("right", 2 * p + 1)):
                cam = table[p][side]
                xu, yu = spec.undistort(cam, float(xyc[v, k, 0, 0]), float(xyc[v, k, 0, 1]))
                b.append(((xu - cam["cx"]) / cam["fx"], (yu - cam["cy"]) / cam["fy"]))
            points[p, k, 0] = np.append(triangulate(pair_views[0], pair_views[1], b[0], b[1]), 0.9)
    return dict(count=count, xyc=xyc, match=match, points=points, views=views), (R, t)
