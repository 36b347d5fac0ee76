"""Golden vectors of the target maps and the loss: the REFERENCE's own _set_keypoints / SceneDataset._compute_centers /
SceneDataset._compute_depth / the three normalisation lines of _extract_example (perception/datasets/video.py) and KeypointLoss
(perception/loss.py), run on hand-made labels.  Needs the reference tree (see _ref_import.py); writes targets.npz and targets.json here.

    python tests/golden/make_goldens_targets.py

Conditions on the fixtures (they concern the reference alone; enforced by rejection, recorded in targets.json): no target heat value
within 1e-4 of the 0.01 mask threshold, and no pixel centre within 1e-3 px of a disc edge - otherwise a last-bit difference flips a
mask pixel and a comparison means nothing."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import import_reference   # noqa: E402
import targets_spec as spec                # noqa: E402  (logits(): the seeded predictions; nothing else of the spec is used here)

import_reference()
import torch                                # noqa: E402
import perception.datasets.video as V      # noqa: E402
from perception.loss import KeypointLoss   # noqa: E402

MASK_MARGIN, EDGE_MARGIN = 1e-4, 1e-3
MAX_OBJ = 4
CONFIGS = {"valve": [1, 3], "cups": [1, 1, 1]}          # config/valve.json, config/cups.json
LOGIT_SEEDS = {"valve": 101, "cups": 102}


def reference_targets(cfg, n_obj, kp, z):
    """kp [n_obj * nk, 2] input pixels, z [n_obj * nk] -> the reference's heat, depth, centre targets and the two margins."""
    K, nk = len(cfg), sum(cfg)
    ds = types.SimpleNamespace(target_size=V.SceneDataset.prediction_size, image_size=(511, 511), keypoint_maps=K, n_objects=n_obj,
                               n_keypoints=nk, keypoint_config=cfg, target_pixel_indices=V._pixel_indices(64, 64))
    p_C = np.concatenate([np.zeros((n_obj * nk, 2)), z[:, None]], 1)
    scaling_factor = np.array([ds.target_size]) / np.array([ds.image_size])
    target = np.zeros((K, 64, 64), dtype=np.float32)
    for o in range(n_obj):                                   # video.py:201-209
        points = kp[o * nk:(o + 1) * nk] * scaling_factor
        for i, n_points in enumerate(cfg):
            start = sum(cfg[:i])
            V._set_keypoints(target[i], points[start:start + n_points])
    centers = V.SceneDataset._compute_centers(ds, kp)
    depth = V.SceneDataset._compute_depth(ds, kp, p_C)
    raw_max = target.reshape(K, -1).max(axis=1)
    heatmap_max = np.maximum(target.max(axis=2).max(axis=1), 0.5)           # video.py:214-215
    target = np.clip(target / heatmap_max[:, None, None], 0.0, 1.0)
    edge = np.inf
    for p in kp * float(64 / 511):
        edge = min(edge, np.abs(np.linalg.norm(p[:, None, None] - ds.target_pixel_indices, axis=0) - 4.0).min())
    return target, depth, centers, float(np.abs(target.astype(np.float64) - 0.01).min()), float(edge), raw_max


def frames_of(cfg, rng):
    """[(what, n_obj, make(rng) -> kp [n_obj * nk, 2])]: 0, 1, 2 and 4 objects, a key point off every border and one in (-1, 0) of the
    map, two overlapping discs, and two same-type key points so close that the map maximum exceeds 1."""
    nk = sum(cfg)

    def scattered(n_obj):
        def make(rng):
            c = rng.uniform(40, 470, (n_obj, 1, 2))
            return np.concatenate([c, c + rng.uniform(-45, 45, (n_obj, nk - 1, 2))], 1).reshape(-1, 2)
        return make

    def off_borders(rng):               # 4 objects: one key point beyond each border; object 0's centre in (-1, 0) of the map (x in (-7.98, 0) px)
        kp = scattered(4)(rng).reshape(4, nk, 2)
        kp[0, 0] = [rng.uniform(-7.0, -1.0), rng.uniform(100, 400)]
        kp[0, 1] = [rng.uniform(-30.0, -9.0), rng.uniform(100, 400)]
        kp[1, 1] = [rng.uniform(513.0, 540.0), rng.uniform(100, 400)]
        kp[2, 1] = [rng.uniform(100, 400), rng.uniform(-30.0, -9.0)]
        kp[3, 1] = [rng.uniform(100, 400), rng.uniform(513.0, 540.0)]
        kp[3, nk - 1] = [rng.uniform(-6.0, -1.0), rng.uniform(-6.0, -1.0)]
        return kp.reshape(-1, 2)

    def overlapping(rng):               # 2 objects whose type-1 key points lie ~4 map pixels apart: the discs overlap, the last one wins
        kp = scattered(2)(rng).reshape(2, nk, 2)
        kp[1, 1] = kp[0, 1] + rng.uniform(25.0, 35.0) * np.array([np.cos(0.7), np.sin(0.7)])
        kp[1, 0] = kp[0, 0] + rng.uniform(20.0, 30.0, 2)
        return kp.reshape(-1, 2)

    def coincident(rng):                # 2 objects whose last key points lie well within a map pixel of each other: map maximum > 1
        kp = scattered(2)(rng).reshape(2, nk, 2)
        kp[1, nk - 1] = kp[0, nk - 1] + rng.uniform(-2.5, 2.5, 2)
        return kp.reshape(-1, 2)

    return [("empty", 0, scattered(0)), ("one", 1, scattered(1)), ("two", 2, scattered(2)), ("four", 4, scattered(4)),
            ("off_borders", 4, off_borders), ("overlapping", 2, overlapping), ("coincident", 2, coincident)]


def main():
    arrays, meta = {}, {"mask_margin": MASK_MARGIN, "edge_margin": EDGE_MARGIN, "max_obj": MAX_OBJ, "stacks": 2, "fixtures": {}}
    for name, cfg_tail in CONFIGS.items():
        cfg = [1] + cfg_tail
        K, nk = len(cfg), sum(cfg)
        rng = np.random.default_rng(LOGIT_SEEDS[name] + 1000)
        labels, n_objs, heat, depth, centers, frames = [], [], [], [], [], []
        for what, n_obj, make in frames_of(cfg, rng):
            rejected = 0
            while True:
                kp = make(rng)
                z = rng.uniform(0.4, 1.5, n_obj * nk)
                t, d, c, mask_margin, edge_margin, raw_max = reference_targets(cfg, n_obj, kp, z)
                ok = mask_margin >= MASK_MARGIN and edge_margin >= EDGE_MARGIN
                if what == "coincident":
                    ok = ok and raw_max.max() > 1.0
                if ok:
                    break
                rejected += 1
            rows = np.zeros((MAX_OBJ * nk, 3))
            rows[:n_obj * nk, :2], rows[:n_obj * nk, 2] = kp, z
            labels.append(rows); n_objs.append(n_obj); heat.append(t); depth.append(d); centers.append(c)
            frames.append({"what": what, "n_obj": n_obj, "rejected": rejected, "mask_margin": mask_margin,
                           "edge_margin": None if not np.isfinite(edge_margin) else edge_margin, "raw_max": [float(v) for v in raw_max]})
        H, D, C = np.stack(heat).astype(np.float32), np.stack(depth).astype(np.float32), np.stack(centers).astype(np.float32)
        N = H.shape[0]
        ph, pd, pc = spec.logits(LOGIT_SEEDS[name], N, K)
        tt = torch.from_numpy
        crit = KeypointLoss(cfg_tail)
        r32 = crit([tt(x) for x in ph], tt(H), [tt(x) for x in pd], tt(D), [tt(x) for x in pc], tt(C))
        r64 = crit([tt(x).double() for x in ph], tt(H).double(), [tt(x).double() for x in pd], tt(D).double(), [tt(x).double() for x in pc], tt(C).double())
        terms = np.zeros((N, 2, 3))                          # per frame: the reference on a batch of one frame, in fp64
        for f in range(N):
            one = crit([tt(x[f:f + 1]).double() for x in ph], tt(H[f:f + 1]).double(), [tt(x[f:f + 1]).double() for x in pd], tt(D[f:f + 1]).double(),
                       [tt(x[f:f + 1]).double() for x in pc], tt(C[f:f + 1]).double())
            for s in range(2):
                terms[f, s] = [float(one[1][s]), float(one[2][s]), float(one[3][s])]

        def tup(r):
            return {"loss": float(r[0]), "heat": [float(v) for v in r[1]], "depth": [float(v) for v in r[2]], "center": [float(v) for v in r[3]]}
        e32, e64 = tup(r32), tup(r64)
        meta["fixtures"][name] = {"keypoint_config": cfg_tail, "logit_seed": LOGIT_SEEDS[name], "frames": frames, "expected_fp32": e32, "expected_fp64": e64,
                                  "reference_fp32_vs_fp64": abs(e32["loss"] - e64["loss"]) / abs(e64["loss"])}
        arrays[f"{name}_labels"] = np.stack(labels)
        arrays[f"{name}_n_obj"] = np.asarray(n_objs, np.int32)
        arrays[f"{name}_heat"], arrays[f"{name}_depth"], arrays[f"{name}_centers"] = H, D, C
        arrays[f"{name}_terms"] = terms
    np.savez_compressed(os.path.join(HERE, "targets.npz"), **arrays)
    with open(os.path.join(HERE, "targets.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: os.path.getsize(os.path.join(HERE, k)) for k in ("targets.npz", "targets.json")})
    print({k: (v["reference_fp32_vs_fp64"], [fr["rejected"] for fr in v["frames"]]) for k, v in meta["fixtures"].items()})


if __name__ == "__main__":
    main()
