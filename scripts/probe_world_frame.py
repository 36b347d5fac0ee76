"""What the world-frame stage (okp_change_frame, csrc/okp_frame.hip; world_frame=True on either device pipeline) costs.  (1) The captured
batch-64 cups step of BatchedKeypointPipeline with the object model and the tracker, with and without world_frame.  (2) The captured fused
tick of four posed pairs with the object model and the tracker, with and without world_frame.  Each pair of graphs lives in ONE process and
alternates in rounds in A B B A order, so that drift of the host or the GPU falls on both; a step = replay + synchronise, host wall time.  With
world_frame a step carries three more launches (points; table and poses; track poses back), and the replay does not copy a new pose in: the
copy of 12 doubles per stream is the caller's, like the frames'.  Prints one JSON line.

    python scripts/probe_world_frame.py [--rounds 12] [--per-round 30] [--warmup 20] [--out profiles/world_frame.json]
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
sys.path.insert(0, os.path.join(REPO, "scripts"))

CUPS_POINTS = [[0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]


def config():
    from object_keypoints_amd import ops
    return ops.TrackConfig(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.1, alpha_R=0.5, min_hits=2, max_misses=5, max_tracks=16)


def poses(n, dev):
    """n camera poses: a turn of 0.1 rad about z and an offset, the same for every stream."""
    from object_keypoints_amd import ops
    c, s = np.cos(0.1), np.sin(0.1)
    T = np.array([[c, -s, 0.0, 0.3], [s, c, 0.0, -0.2], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])
    return ops.frame_poses(np.stack([T] * n)).to(dev)


def abba(arms, rounds, per_round, warmup):
    """arms: {"plain": step, "world": step} of captured steps -> per-arm medians, per-round spans and their difference."""
    def tick(name):
        arms[name].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(warmup):
            tick(name)
    lat, meds = {n: [] for n in arms}, {n: [] for n in arms}
    order = ["plain", "world", "world", "plain"]
    for r in range(rounds):
        name = order[r % 4]
        this = []
        for _ in range(per_round):
            t0 = time.perf_counter()
            tick(name)
            this.append((time.perf_counter() - t0) * 1e3)
        lat[name] += this
        meds[name].append(float(np.median(this)))
    res = {}
    for name in arms:
        res[name] = {"median_ms": float(np.median(lat[name])), "p99_ms": float(np.percentile(lat[name], 99)), "round_medians_ms": [round(v, 4) for v in meds[name]],
                     "round_spread_ms": float(np.max(meds[name]) - np.min(meds[name]))}
    res["world_minus_plain_us"] = (res["world"]["median_ms"] - res["plain"]["median_ms"]) * 1e3
    res["world_over_plain_percent"] = 100.0 * (res["world"]["median_ms"] / res["plain"]["median_ms"] - 1.0)
    return res


def captured_step(dev, world_frame, batch=64):
    """The captured batch-64 cups step with the object model and the tracker."""
    from probe_object_pose import network
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    frames = torch.randn((batch, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    params = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    cam = cu.FisheyeCamera(params["K"], params["D"], params["image_size"])
    pipe = pp.BatchedKeypointPipeline(network(4, dev), {"keypoint_config": [1, 1, 1]}, cam, points_3d=CUPS_POINTS, track=config(), world_frame=world_frame)
    return pipe, pipe.capture(frames, poses(batch, dev) if world_frame else None)


def captured_tick(dev, world_frame):
    """The captured fused tick of four posed pairs with the object model and the tracker."""
    from probe_object_pose import network
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    rig_poses = synth.rig_poses()
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, rig_poses)).to(dev)
    o = synth.rig_fuse_scene()[0]
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5, rig_poses=rig_poses,
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), track=config(), world_frame=world_frame)
    return pipe, pipe.capture_device(frames, heat_override=heat, rig_pose=poses(1, dev) if world_frame else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"probe": "world_frame", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process", "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        plain, (pipe, world) = captured_step(dev, False, args.batch)[1], captured_step(dev, True, args.batch)
        assert "world" in world.replay() and "world" not in plain.replay()
        res["step"] = dict(abba({"plain": plain, "world": world}, args.rounds, args.per_round, args.warmup), batch=args.batch, dtype="float16",
                           what="captured BatchedKeypointPipeline step with the object model and the tracker: replay + synchronise, host wall time, ms")
        del plain, world, pipe
        plain, (pipe, world) = captured_tick(dev, False)[1], captured_tick(dev, True)
        assert len(pipe.rig_tracks(world.replay())) >= 1
        res["tick"] = dict(abba({"plain": plain, "world": world}, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", capacity=16, objects=2,
                           what="captured fused tick_device with the object model and the tracker: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
