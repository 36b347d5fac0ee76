"""The fabricated cases of the object pose tests: each a point table, a model and the conditions it was built to meet.  The CPU tests
(tests/test_object_pose_args.py) assert those conditions on the inputs; the GPU tests (tests/test_gpu_object_pose.py) compare the device
with the specification (tests/object_pose_spec.py) on the same cases.

    python tests/object_pose_cases.py --write      # records the disagreement of the two NumPy formulations in tests/golden/object_pose_cases.json
"""
import itertools
import json
import os

import numpy as np

import object_pose_spec as spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "object_pose_cases.json")
MIN_RATIO = 1e-2          # conditioned cases: second scatter eigenvalue / trace, on both sides
MIN_GAP = 1e-6            # m^2: the runner-up's cost above the winner's, where H > 1

VALVE = [1, 3]            # config/valve.json
CUPS = [1, 1, 1]          # config/cups.json


def rotation(rng, max_deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-max_deg, max_deg))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def generic_model(type_count, seed, scale=0.1, min_sep=0.03):
    """Key points drawn in a cube of +-scale metres, no two closer than min_sep: no symmetry, so a wrong assignment costs."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < sum(type_count):
        x = rng.uniform(-scale, scale, size=3)
        if all(np.linalg.norm(x - y) >= min_sep for y in pts):
            pts.append(x)
    return spec.model_of(np.stack(pts), type_count)


def conditioned(model, type_count, rows):
    """The conditions of a conditioned object (see the module docstring of test_object_pose_args): both scatters well away from collinear,
    and with several hypotheses a clear winner."""
    filled = np.isfinite(rows).all(axis=1)
    if filled.sum() < 3 or spec.second_eigenvalue_ratio(rows[filled, :3]) < MIN_RATIO:
        return False
    hyps = spec.hypotheses(filled, type_count)
    fits = sorted((spec.fit_kabsch(model[h], rows[filled, :3])[3], i) for i, h in enumerate(hyps))
    win = hyps[fits[0][1]]
    if spec.second_eigenvalue_ratio(model[win]) < MIN_RATIO:
        return False
    return len(hyps) == 1 or fits[1][0] - fits[0][0] >= MIN_GAP


def scene(type_count, model, B, max_obj, n_obj, seed, noise=2e-3, miss=0.0, permute=True):
    """tab [B,max_obj,S,4]: object o of frame b is the model under a random pose plus isotropic noise (sigma `noise`), each key point
    missing with probability `miss` (at least three point pairs stay), the detected order within a type shuffled; every object is drawn
    again until it is conditioned.  -> tab, truth {(b, o): (R, t)}."""
    rng = np.random.default_rng(seed)
    S = model.shape[0]
    tab = np.full((B, max_obj, S, 4), np.nan)
    truth = {}
    for b in range(B):
        for o in range(int(n_obj[b])):
            while True:
                R, t = rotation(rng), np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.5, 1.5)])
                rows = np.full((S, 4), np.nan)
                base = 1
                rows[0, :3] = R @ model[0] + t + rng.normal(scale=noise, size=3)
                for c in type_count:
                    order = rng.permutation(c) if permute else np.arange(c)
                    seen = [i for i in order if rng.uniform() >= miss]
                    for j, i in enumerate(seen):              # compacted: the detected key points of a type fill its first slots
                        rows[base + j, :3] = R @ model[base + i] + t + rng.normal(scale=noise, size=3)
                    base += c
                if rng.uniform() < miss:
                    rows[0] = np.nan                          # the centre's own 3D point may be missing too
                ok = np.isfinite(rows[:, 0])
                rows[ok, 3] = rng.uniform(0.5, 1.0, size=int(ok.sum()))
                if conditioned(model, type_count, rows):
                    break
            tab[b, o] = rows
            truth[(b, o)] = (R, t)
    return tab, truth


def _case(name, type_count, model, tab, n_obj, max_rmse=np.inf, truth=None, kind="conditioned", noise=0.0):
    return {"name": name, "type_count": list(type_count), "model": model, "tab": tab, "n_obj": np.asarray(n_obj, dtype=np.int32),
            "max_rmse": max_rmse, "truth": truth, "kind": kind, "noise": noise}


def cases():
    out = []
    valve, cups = generic_model(VALVE, 1), generic_model(CUPS, 2)
    # batch 1 and batch 64, mixed object counts
    tab, truth = scene(VALVE, valve, 1, 4, [3], seed=10)
    out.append(_case("valve_b1", VALVE, valve, tab, [3], truth=truth, noise=2e-3))
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 5, size=64)
    tab, truth = scene(CUPS, cups, 64, 4, counts, seed=12)
    out.append(_case("cups_b64_mixed_counts", CUPS, cups, tab, counts, truth=truth, noise=2e-3))
    counts = rng.integers(0, 5, size=64)
    tab, truth = scene(VALVE, valve, 64, 4, counts, seed=13, miss=0.25)
    out.append(_case("valve_b64_missing_keypoints", VALVE, valve, tab, counts, truth=truth, noise=2e-3))
    # noise-free: the generating pose comes back
    tab, truth = scene(VALVE, valve, 2, 4, [4, 2], seed=14, noise=0.0, miss=0.2)
    out.append(_case("valve_noise_free", VALVE, valve, tab, [4, 2], truth=truth))
    # used = 2 (FEW), used = 3 (a pose), used = 1 and an object of empty slots
    tab, truth = scene(VALVE, valve, 1, 8, [4], seed=15)
    tab[0, 0, [1, 2, 3]] = np.nan                                # centre + 1 key point
    tab[0, 1, [0, 4]] = np.nan                                   # three key points: drawn again below until conditioned
    tab[0, 2, 1:] = np.nan                                       # the centre alone
    tab[0, 3] = np.nan                                           # a live object without a single point
    seed = 150
    while not conditioned(valve, VALVE, tab[0, 1]):
        t2, _ = scene(VALVE, valve, 1, 1, [1], seed=seed)
        tab[0, 1] = t2[0, 0]
        tab[0, 1, [0, 4]] = np.nan
        seed += 1
    out.append(_case("used_1_2_3", VALVE, valve, tab, [4], kind="few", noise=2e-3))
    # collinear detected points (small integers: the scatter is exact) and a collinear model subset under well-spread detections
    four = [1, 1, 1, 1]
    line = spec.model_of(np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 3.0, 1.0]]), four)
    tab = np.full((1, 4, 5, 4), np.nan)
    tab[0, 0, 1:4, :3] = [[1.0, 1.0, 2.0], [2.0, 3.0, 2.0], [3.0, 5.0, 2.0]]                       # on a line, all slots of a subset
    tab[0, 1, :, :3] = [[0.0, 0.0, 4.0], [1.0, 1.0, 5.0], [2.0, 2.0, 6.0], [3.0, 3.0, 7.0], [-2.0, -2.0, 2.0]]   # five points on a line
    tab[0, 2, 1:4, :3] = [[0.0, 0.0, 5.0], [2.0, 1.0, 5.0], [1.0, 3.0, 6.0]]                       # a triangle against model rows 1..3: a line
    tab[0, 3, :, :3] = [[7.0, 7.0, 7.0]] * 5                                                      # five coincident points
    tab[..., 3] = np.where(np.isfinite(tab[..., 0]), 0.75, np.nan)
    out.append(_case("collinear", four, line, tab, [4], kind="degenerate"))
    # POOR: the bound between the noise of the good objects and the bad ones
    tab, truth = scene(VALVE, valve, 1, 4, [4], seed=16, noise=5e-4)
    bad, _ = scene(VALVE, valve, 1, 4, [4], seed=17, noise=8e-3)
    tab[0, 1], tab[0, 3] = bad[0, 1], bad[0, 3]
    out.append(_case("poor", VALVE, valve, tab, [4], max_rmse=3e-3, kind="poor", noise=8e-3))
    # nothing to do; a full frame of 64 objects
    out.append(_case("n_obj_0", VALVE, valve, scene(VALVE, valve, 2, 4, [3, 2], seed=18)[0], [0, 0], kind="empty"))
    tab, truth = scene(CUPS, cups, 1, 64, [64], seed=19)
    out.append(_case("max_obj_64", CUPS, cups, tab, [64], truth=truth, noise=2e-3))
    # the widest table, the longest search
    wide = [1] * 15
    m16 = generic_model(wide, 3, scale=0.2)
    tab, truth = scene(wide, m16, 2, 3, [3, 1], seed=20, miss=0.2)
    out.append(_case("S_16", wide, m16, tab, [3, 1], truth=truth, noise=2e-3))
    two4 = [4, 4]
    m9 = generic_model(two4, 4, scale=0.15, min_sep=0.06)
    tab, truth = scene(two4, m9, 2, 3, [3, 2], seed=21, noise=1e-3)
    out.append(_case("H_576", two4, m9, tab, [3, 2], truth=truth, noise=1e-3))
    both = [4, 4, 1, 1, 1, 1, 1, 1, 1]
    m16b = generic_model(both, 5, scale=0.2, min_sep=0.06)
    tab, truth = scene(both, m16b, 1, 2, [2], seed=22, noise=1e-3)
    out.append(_case("S_16_H_576", both, m16b, tab, [2], truth=truth, noise=1e-3))
    # one object, its three type-2 key points detected in each of the six orders
    one, truth = scene(VALVE, valve, 1, 1, [1], seed=23, permute=False)
    tab = np.full((1, 8, 5, 4), np.nan)
    for o, perm in enumerate(itertools.permutations(range(3))):
        tab[0, o] = one[0, 0]
        tab[0, o, 2:5] = one[0, 0, 2:5][list(perm)]
    out.append(_case("permutations", VALVE, valve, tab, [6], truth={(0, o): truth[(0, 0)] for o in range(6)}, kind="permutations", noise=2e-3))
    # a symmetric valve: three handle points 120 degrees apart around the stem's axis - every assignment of them fits as well as the others
    a = np.deg2rad([90.0, 210.0, 330.0])
    sym = spec.model_of(np.concatenate([[[0.0, 0.0, 0.08]], 0.1 * np.stack([np.cos(a), np.sin(a), np.zeros(3)], axis=1)]), VALVE)
    rng = np.random.default_rng(24)
    tab = np.full((1, 4, 5, 4), np.nan)
    for o in range(4):
        R, t = rotation(rng), np.array([0.1 * o, -0.2, 1.0])
        tab[0, o, :, :3] = sym @ R.T + t + rng.normal(scale=1e-3, size=(5, 3))
        tab[0, o, :, 3] = 0.9
    out.append(_case("symmetric_valve", VALVE, sym, tab, [4], kind="symmetric", noise=1e-3))
    return out


def disagreement(case):
    """Largest |Kabsch - Horn| in R, t and both rmse values over the case's posed objects."""
    a = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"], fit=spec.fit_kabsch)
    b = spec.object_pose(case["tab"], case["n_obj"], case["model"], case["type_count"], case["max_rmse"], fit=spec.fit_horn)
    pa, pb = a["pose"].reshape(a["pose"].shape[:2] + (3, 4)), b["pose"].reshape(b["pose"].shape[:2] + (3, 4))
    d = lambda x, y: float(np.nanmax(np.abs(x - y), initial=0.0))
    return {"R": d(pa[..., :3], pb[..., :3]), "t": d(pa[..., 3], pb[..., 3]), "rmse": d(a["fit"], b["fit"])}


if __name__ == "__main__":
    import sys
    if "--write" in sys.argv:
        rec = {c["name"]: disagreement(c) for c in cases() if c["kind"] != "symmetric"}
        with open(GOLDEN, "w") as f:
            json.dump({"what": "largest |Kabsch (SVD) - Horn (eigh)| of the two NumPy formulations of the fit per case: R (unitless), t and rmse (metres)",
                       "cases": rec}, f, indent=1)
            f.write("\n")
        print(json.dumps(rec, indent=1))
