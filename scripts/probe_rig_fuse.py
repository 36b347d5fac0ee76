"""What rig fusion (okp_rig_fuse, csrc/okp_rig.hip) costs.  (1) The stage alone - its two launches replayed as one hipGraph, device time by
events around batches of replays - at P = 4, K = 3, cap = 16 and at P = 8, K = 4, cap = 64, on payloads of points seen by most pairs.
(2) The captured whole tick of a rig of four posed pairs (synth.stereo_rig / synth.rig_poses, fp16 network, capacity 16, injected heat maps
of synth.render_rig_fuse_heat) with and without the stage: both graphs live in ONE process and alternate in rounds of --per-round ticks, so
that drift of the host or the GPU falls on both; a tick = replay + synchronise, host wall time.  Prints one JSON line: the stage's median
per shape, each arm's median, the difference, and the spread of the per-round medians of each arm.

    python scripts/probe_rig_fuse.py [--rounds 10] [--per-round 40] [--warmup 20] [--out profiles/rig_fuse.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def payload(P, K, cap, n_points, seed, dev):
    """points [P,K,cap,4] of n_points[k] lattice points per type, each seen by a pair with probability 0.85, in random slots; identity
    poses with small offsets."""
    rng = np.random.default_rng(seed)
    points = np.full((P, K, cap, 4), np.nan)
    poses = np.tile(np.eye(4)[:3].reshape(12), (P, 1))
    poses[:, [3, 7, 11]] = rng.uniform(-0.3, 0.3, size=(P, 3))
    for k in range(K):
        cells = rng.permutation(64)[:n_points[k]]
        world = np.stack([cells % 4, (cells // 4) % 4, cells // 16], axis=1) * 0.25
        for p in range(P):
            seen = [i for i in range(n_points[k]) if rng.uniform() < 0.85][:cap]
            for s, i in zip(rng.permutation(cap), seen):
                points[p, k, s, :3] = world[i] + rng.uniform(-0.004, 0.004, size=3) - poses[p, [3, 7, 11]]
                points[p, k, s, 3] = rng.uniform(0.3, 1.0)
    return torch.from_numpy(points).to(dev), torch.from_numpy(poses).to(dev)


def stage_time(P, K, cap, n_points, type_count, cap_f, dev, batches=30, per_batch=50):
    from object_keypoints_amd import ops
    points, poses = payload(P, K, cap, n_points, 5, dev)
    for _ in range(3):
        out = ops.rig_fuse(points, poses, type_count, 0.05, 0.4, cap_f)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.rig_fuse(points, poses, type_count, 0.05, 0.4, cap_f)
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_batch):
            graph.replay()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / per_batch)
    return {"P": P, "K": K, "cap": cap, "cap_f": cap_f, "candidates": int((~points[..., 3].isnan()).sum()), "clusters": out["n_fused"].tolist(),
            "median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)),
            "note": "graph replay of the two launches, back to back: launch gaps included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"probe": "rig_fuse", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "per_round": args.per_round,
           "stage": [stage_time(4, 3, 16, [2, 2, 6], [1, 3], 16, dev), stage_time(8, 4, 64, [6, 20, 40, 60], [2, 4, 6], 64, dev)]}
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    poses = synth.rig_poses()
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, poses)).to(dev)
    arms = {}
    for name, kw in (("plain", {}), ("fused", dict(rig_poses=poses, merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS,
                                                   fuse_capacity=16))):
        pipe = pp.StereoStreamPipeline(net, rig, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5, **kw)
        arms[name] = (pipe, pipe.capture_device(frames, heat_override=heat))
    assert len(arms["fused"][0].rig_objects(arms["fused"][1].replay())) == 2

    def tick(name):
        arms[name][1].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(args.warmup):
            tick(name)
    lat, rounds = {n: [] for n in arms}, {n: [] for n in arms}
    for r in range(args.rounds):
        for name in (arms if r % 2 == 0 else reversed(list(arms))):
            this = []
            for _ in range(args.per_round):
                t0 = time.perf_counter()
                tick(name)
                this.append((time.perf_counter() - t0) * 1e3)
            lat[name] += this
            rounds[name].append(float(np.median(this)))
    res["tick"] = {"pairs": 4, "dtype": "float16", "capacity": 16, "what": "captured tick_device: replay + synchronise, host wall time, ms"}
    for name in arms:
        res["tick"][name] = {"median_ms": float(np.median(lat[name])), "p99_ms": float(np.percentile(lat[name], 99)),
                             "round_medians_ms": [round(v, 4) for v in rounds[name]],
                             "round_spread_ms": float(np.max(rounds[name]) - np.min(rounds[name]))}
    res["tick"]["fused_minus_plain_us"] = (res["tick"]["fused"]["median_ms"] - res["tick"]["plain"]["median_ms"]) * 1e3
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
