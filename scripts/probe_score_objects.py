"""What okp_score_objects (csrc/okp_score.hip) costs: its two launches alone, replayed back to back as a hipGraph, device time by events around
batches of replays (docs/MEASUREMENT.md; the method of scripts/probe_window.py).  Case one: B = 64 frames, max_obj = 16, G = 16, S = 5, P = 4
pose sets (two by row, two through an index), the camera's view test on.  Case two, a rig tick: B = 1, max_obj = 64, G = 64, S = 5, P = 4, no
camera.  Every detection is live and matched, every slot lifted, so each call emits B * max_obj * S key-point records and B * max_obj pose
records into a log large enough never to overflow during the run; the log's cursors advance with every replay, which is the product's use.
There is no threshold: the number is reported.  Prints one JSON line.

    python scripts/probe_score_objects.py [--batches 30] [--per-batch 50] [--out profiles/score_objects.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_object_pose import CUPS_POINTS, map_camera                      # noqa: E402
from probe_refine import replay_time                                       # noqa: E402
from probe_refine_views import _rotation                                   # noqa: E402


def scene(B, max_obj, G, dev, seed=7):
    """B frames of G labelled objects of a five-row model on a grid 0.8-1.2 m in front of the camera, max_obj detections each a few
    millimetres off their label, and four pose sets -> the arguments of ops.score_objects."""
    rng = np.random.default_rng(seed)
    model = np.concatenate([np.zeros((1, 3)), np.asarray(CUPS_POINTS) * 0.3, [[0.0, 0.02, 0.03]]])
    S = model.shape[0]
    side = int(np.ceil(np.sqrt(G)))
    grid = np.array([[(g % side - (side - 1) / 2.0), (g // side - (side - 1) / 2.0)] for g in range(G)]) * (0.5 / side)
    R = np.stack([[_rotation(rng) for _ in range(G)] for _ in range(B)])
    t = np.concatenate([np.broadcast_to(grid, (B, G, 2)) + rng.uniform(-0.005, 0.005, (B, G, 2)), rng.uniform(0.8, 1.2, (B, G, 1))], axis=2)
    row = lambda R, t: np.concatenate([R, t[..., None]], axis=-1).reshape(R.shape[:-2] + (12,))
    truth = np.concatenate([np.einsum("bgij,sj->bgsi", R, model) + t[:, :, None], np.ones((B, G, S, 1))], axis=3)
    of = np.stack([rng.permutation(G)[np.arange(max_obj) % G] for _ in range(B)])
    Re = np.einsum("boij,bojk->boik", np.take_along_axis(R, of[:, :, None, None], axis=1), np.stack([[_rotation(rng, 0.05) for _ in range(max_obj)] for _ in range(B)]))
    te = np.take_along_axis(t, of[:, :, None], axis=1) + rng.normal(scale=0.003, size=(B, max_obj, 3))
    tab = np.concatenate([np.einsum("boij,sj->bosi", Re, model) + te[:, :, None] + rng.normal(scale=0.002, size=(B, max_obj, S, 3)), np.full((B, max_obj, S, 1), 0.9)], axis=3)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fit = row(Re, te)
    track_of = to(np.stack([rng.permutation(max_obj) for _ in range(B)]).astype(np.int32))
    sets = [to(fit), to(fit + rng.normal(scale=1e-3, size=fit.shape)), (to(fit), track_of), (to(fit[:, ::-1].copy()), track_of)]
    return dict(tab=to(tab), n_obj=to(np.full(B, max_obj, np.int32)), truth=to(truth), n_truth=to(np.full(B, G, np.int32)), pose_sets=sets,
                truth_pose=to(row(R, t)), model=to(model)), S


def measure(name, B, max_obj, G, camera, dev, batches, per_batch):
    from object_keypoints_amd import ops
    args, S = scene(B, max_obj, G, dev)
    replays = 3 + 1 + 10 + batches * per_batch
    log = ops.score_log(B * max_obj * S * (replays + 1), B * max_obj * (replays + 1), dev)
    cam = map_camera()
    kw = dict(cam=cam.okp(), size=tuple(float(v) for v in cam.image_size)) if camera else {}
    cfg = ops.ScoreConfig()
    out, us = replay_time(lambda: ops.score_objects(args["tab"], args["n_obj"], args["truth"], args["n_truth"], log, cfg, pose_sets=args["pose_sets"],
                                                    truth_pose=args["truth_pose"], model=args["model"], **kw), batches, per_batch)
    counts = log["counts"].cpu().numpy()
    calls = int(counts[ops.SCORE_CALLS])
    return {"case": name, "frames": B, "max_obj": max_obj, "labelled_objects": G, "rows": S, "pose_sets": 4, "camera": bool(camera),
            "median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)), "batches": batches, "replays_per_batch": per_batch,
            "calls": calls, "detections_per_call": int(counts[ops.SCORE_DETECTIONS]) // calls, "key_point_records_per_call": int(counts[ops.SCORE_KP_WRITTEN]) // calls,
            "pose_records_per_call": int(counts[ops.SCORE_POSE_WRITTEN]) // calls, "overflow": int(counts[ops.SCORE_OVERFLOW_WORD]),
            "note": "graph replay of the two launches, back to back: launch gaps included; the log's cursors advance with every replay"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--per-batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"probe": "score_objects", "device": torch.cuda.get_device_name(dev),
           "launch": [measure("batch", 64, 16, 16, True, dev, a.batches, a.per_batch), measure("rig tick", 1, 64, 64, False, dev, a.batches, a.per_batch)]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
