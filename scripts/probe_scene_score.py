"""Scoring labelled scenes on the device: what the fused pass costs and what it is measured against -> profiles/scene_score.json.

    python scripts/probe_scene_score.py [--out profiles/scene_score.json]

Needs a GPU.  Three measurements at N = 64, K = 4, S = 2, alternating in one process (HIP events around `reps` calls after a warm-up, median of
`rounds`; wall = host clock around the same calls ending in a synchronise):
  fused      ops.keypoint_loss from labels (two launches: render-and-score, fold)
  stock      the reference's KeypointLoss written line by line in torch ops on the device (perception/loss.py:20-48: boolean indexing, so it
             synchronises with the host) on dense targets from ops.render_targets
  score      SceneScorer.score against net.forward alone, bfloat16
and the measured distances to the golden vectors (tests/golden/targets.*): heat error over its bound, loss error over its bar."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import targets_spec as spec                                    # noqa: E402
from object_keypoints_amd import ops, synth                    # noqa: E402
from object_keypoints_amd.perception.models import KeypointNet  # noqa: E402
from object_keypoints_amd.perception.pipeline import SceneScorer  # noqa: E402


def stock_loss(p_heatmaps, gt_heatmaps, p_depth, gt_depth, p_centers, gt_centers, depth_weight=10.0, center_weight=1.0):
    heatmap_loss = depth_loss = center_loss = 0.0
    N = float(gt_heatmaps.shape[0])
    for p_hm, p_d, p_center in zip(p_heatmaps, p_depth, p_centers):
        heatmap_loss = heatmap_loss + F.binary_cross_entropy_with_logits(p_hm, gt_heatmaps, reduction='none').sum(dim=[1, 2, 3]).mean()
        where_heat = gt_heatmaps > 0.01
        depth_loss = depth_loss + F.l1_loss(p_d[where_heat], gt_depth[where_heat], reduction='sum') / N
        where_heat = where_heat[:, 1:, None].expand(-1, -1, 2, -1, -1)
        center_loss = center_loss + F.smooth_l1_loss(p_center[where_heat], gt_centers[where_heat], reduction='sum') / N
    return heatmap_loss + depth_weight * depth_loss + center_weight * center_loss


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / reps, (time.perf_counter() - t0) * 1e6 / reps        # microseconds: device span, wall


def golden_distances():
    golden = os.path.join(REPO, "tests", "golden")
    meta, z = json.load(open(os.path.join(golden, "targets.json"))), np.load(os.path.join(golden, "targets.npz"))
    out = {}
    for name, fx in meta["fixtures"].items():
        tc = [1] + fx["keypoint_config"]
        labels, n_obj = torch.from_numpy(z[f"{name}_labels"]).cuda(), torch.from_numpy(z[f"{name}_n_obj"]).cuda()
        heat = ops.render_targets(labels, n_obj, tc)[0].cpu().numpy()
        worst = max(float(np.abs(heat[f, k].astype(np.float64) - z[f"{name}_heat"][f, k]).max()) / spec.heat_tolerance(int(z[f"{name}_n_obj"][f]) * tc[k])
                    for f in range(heat.shape[0]) for k in range(len(tc)))
        ph, pd, pc = [[torch.from_numpy(x).cuda() for x in lst] for lst in spec.logits(fx["logit_seed"], heat.shape[0], len(tc), meta["stacks"])]
        loss = float(ops.keypoint_loss(ph, pd, pc, tc, labels=labels, n_obj=n_obj)["loss"])
        rel = abs(loss - fx["expected_fp64"]["loss"]) / fx["expected_fp64"]["loss"]
        out[name] = {"heat_max_error_over_bound": worst, "loss_rel_error_vs_reference_fp64": rel, "loss_bar": max(10 * fx["reference_fp32_vs_fp64"], 1e-6),
                     "reference_fp32_vs_fp64": fx["reference_fp32_vs_fp64"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_score.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    N, tc = 64, [1, 1, 1, 1]
    pts, n_obj = spec.random_labels(11, N, tc, 4)
    labels, n_dev = torch.from_numpy(pts).cuda(), torch.from_numpy(n_obj).cuda()
    ph, pd, pc = [[torch.from_numpy(x).cuda() for x in lst] for lst in spec.logits(12, N, len(tc))]
    dense = ops.render_targets(labels, n_dev, tc)
    cases = {"fused_from_labels": lambda: ops.keypoint_loss(ph, pd, pc, tc, labels=labels, n_obj=n_dev),
             "fused_dense": lambda: ops.keypoint_loss(ph, pd, pc, tc, targets=dense),
             "render_targets": lambda: ops.render_targets(labels, n_dev, tc),
             "stock_torch_ops": lambda: stock_loss(ph, dense[0], pd, dense[1], pc, dense[2])}
    net = KeypointNet(features=128, heatmaps_out=4, compute_dtype=torch.bfloat16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().cuda()
    frames = torch.from_numpy(synth.frames(N, seed=1)).cuda()
    scorer = SceneScorer(net, [1, 1, 1])
    lab = {"points": labels, "n_obj": n_dev}
    net_cases = {"net_forward_bf16": lambda: net.forward(frames, check_range=False), "score_bf16": lambda: scorer.score(frames, lab)}
    res = {}
    for group, reps in ((cases, a.reps), (net_cases, max(3, a.reps // 10))):
        for fn in group.values():
            for _ in range(3):
                fn()
        samples = {k: [] for k in group}
        for _ in range(a.rounds):                      # alternate the cases inside every round
            for k, fn in group.items():
                samples[k].append(timed(fn, reps))
        for k, v in samples.items():
            res[k] = {"device_span_us": float(np.median([s[0] for s in v])), "wall_us": float(np.median([s[1] for s in v])),
                      "device_span_us_all": [round(s[0], 2) for s in v]}
    stock = float(stock_loss(ph, dense[0], pd, dense[1], pc, dense[2]))
    fused = float(ops.keypoint_loss(ph, pd, pc, tc, targets=dense)["loss"])
    out = {"shape": {"N": N, "K": len(tc), "S": 2}, "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "times": res, "stock_vs_fused_rel": abs(stock - fused) / fused, "goldens": golden_distances(),
           "note": "device_span_us: HIP events around `reps` back-to-back calls, per call (launch gaps included: the pass is launch- and latency-bound); "
                   "the stock loss synchronises with the host inside each call, so its figure depends on the host"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (round(v["device_span_us"], 1), round(v["wall_us"], 1)) for k, v in res.items()}))


if __name__ == "__main__":
    main()
