"""What the object pose stage (okp_object_points / okp_rig_object_points + okp_object_pose, csrc/okp_pose.hip) costs.  (1) The stage alone
- its two launches replayed as one hipGraph, device time by events around batches of replays - on the grouping of the batch-64 cups scene
of the tests (synth.bump_scene, 160 objects, one hypothesis each) and of a batch-64 valve scene (six hypotheses per object).  (2) The captured
batch-64 cups step (fp16 network, forward_device) and (3) the captured fused tick of four posed pairs, each with and without a model.  A
pipeline built without a model launches exactly what the parent commit launches; both graphs live in ONE process and alternate in rounds
in A B B A order, so that drift of the host or the GPU falls on both; a step = replay + synchronise, host wall time.  (4) With --parent-lib
(the parent commit's build of libokp_hip.so) the same two captured graphs against THAT library, selected through OKP_LIB: one fresh process
per arm in A B B A order (parent library without a model, this tree's library with one; both through the ctypes binding, which OKP_LIB
selects - a replay marshals nothing either way).  This arm also sees what moving the lifting helpers into okp_internal.h did to the
existing kernels; it carries the process-to-process scatter of a capture on top.  Prints one JSON line.

    python scripts/probe_object_pose.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/object_pose.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CUPS_POINTS = [[0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]
VALVE_POINTS = [[0.0, 0.0, 0.12], [0.09, 0.01, 0.0], [-0.05, 0.08, 0.01], [-0.03, -0.085, 0.02]]


def map_camera():
    """The camera of the 64 x 64 maps (scripts/eval_model.py:61-69: scale to 511, centre-crop, scale to 64), as bench.py builds it."""
    from object_keypoints_amd.perception.utils import camera_utils as cu
    params = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    return cu.FisheyeCamera(params["K"], params["D"], params["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)


def stage_time(cfg, points_3d, n_objects, dev, batches=30, per_batch=50):
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = map_camera()
    scenes = [synth.bump_scene(cfg, n_objects=n_objects(i), seed=11, index=i) for i in range(64)]
    maps = [torch.from_numpy(np.stack([s[key] for s in scenes])).to(dev) for key in ("heat", "depth", "centers")]
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": cfg}, cam)
    out = pipe.postprocess_device(*maps)
    model = ops.object_model(points_3d, cfg).to(dev)

    def stage():
        tab = ops.object_points(pipe.cam, out, cfg, 63, 63)
        return ops.object_pose(tab, out["n_obj"], model, cfg)

    for _ in range(3):
        res = stage()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = stage()
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
    hyp = 1
    for c in cfg:
        hyp *= int(np.prod(np.arange(1, c + 1)))
    return {"keypoint_config": cfg, "batch": 64, "max_objects": 16, "objects": int(out["n_obj"].sum()), "posed": int((res["used"] >= 3).sum()),
            "hypotheses_per_object": hyp, "median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)),
            "note": "graph replay of the two launches, back to back: launch gaps included"}


def abba(arms, rounds, per_round, warmup):
    """arms: {"plain": step, "pose": step} of captured steps -> per-arm medians and their difference."""
    def tick(name):
        arms[name].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(warmup):
            tick(name)
    lat, meds = {n: [] for n in arms}, {n: [] for n in arms}
    order = ["plain", "pose", "pose", "plain"]
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
    res["pose_minus_plain_us"] = (res["pose"]["median_ms"] - res["plain"]["median_ms"]) * 1e3
    res["pose_over_plain_percent"] = 100.0 * (res["pose"]["median_ms"] / res["plain"]["median_ms"] - 1.0)
    return res


def network(heatmaps_out, dev):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=heatmaps_out, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().to(dev)


NEW_ENTRY_POINTS = ("okp_object_points", "okp_rig_object_points", "okp_object_pose")


def captured_step(dev, with_model):
    """The captured batch-64 cups step (fp16 network, forward_device), with or without the object model."""
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pipe = pp.BatchedKeypointPipeline(network(4, dev), {"keypoint_config": [1, 1, 1]}, map_camera(), **({"points_3d": CUPS_POINTS} if with_model else {}))
    return pipe, pipe.capture(frames)


def captured_tick(dev, with_model):
    """The captured fused tick of four posed pairs, with or without the object model."""
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    poses = synth.rig_poses()
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, poses)).to(dev)
    o = synth.rig_fuse_scene()[0]
    kw = dict(rig_poses=poses, merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16)
    if with_model:
        kw["points_3d"] = np.concatenate([o[1], o[2]])
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5, **kw)
    return pipe, pipe.capture_device(frames, heat_override=heat)


def one_arm(what, arm, n, warmup):
    """Child process of --parent-lib: one captured graph, n replays -> one JSON line.  The parent commit's library does not export the three
    pose entry points, so the parent arm takes them off the signature table before the library is loaded (it never calls them)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = (captured_step if what == "step" else captured_tick)(dev, arm == "pose")
        assert ("pose" in step.static_out) == (arm == "pose")
        lat = []
        for i in range(warmup + n):
            t0 = time.perf_counter()
            step.replay()
            torch.cuda.synchronize()
            if i >= warmup:
                lat.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": what, "arm": arm, "lib": _lib.LIB_PATH, "median_ms": float(np.median(lat)), "p99_ms": float(np.percentile(lat, 99))}))


def against_parent_library(parent_lib, n, warmup):
    """One fresh process per arm and graph, A B B A; the first failure ends the series."""
    from object_keypoints_amd import _lib
    libs = {"parent": os.path.abspath(parent_lib), "pose": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    res = {"order": "parent pose pose parent, one process each", "replays_per_process": n}
    for what in ("step", "tick"):
        runs = {"parent": [], "pose": []}
        for arm in ("parent", "pose", "pose", "parent"):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--what", what, "--per-round", str(n), "--warmup", str(warmup)]
            done = subprocess.run(cmd, env=dict(os.environ, OKP_LIB=libs[arm]), capture_output=True, text=True, timeout=240)
            if done.returncode != 0:
                raise SystemExit(f"{' '.join(cmd)} ended with {done.returncode}:\n{done.stderr[-2000:]}")
            runs[arm].append(json.loads(done.stdout.strip().splitlines()[-1])["median_ms"])
        mean = {arm: float(np.mean(v)) for arm, v in runs.items()}
        res[what] = {"parent_median_ms": runs["parent"], "pose_median_ms": runs["pose"], "pose_minus_parent_us": (mean["pose"] - mean["parent"]) * 1e3,
                     "pose_over_parent_percent": 100.0 * (mean["pose"] / mean["parent"] - 1.0),
                     "process_scatter_us": 1e3 * max(abs(v[0] - v[1]) for v in runs.values())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time both graphs against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "pose"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--what", choices=["step", "tick"], default="step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.what, args.arm, args.per_round, args.warmup)
    res = {"probe": "object_pose", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["stage"] = [stage_time([1, 1, 1], CUPS_POINTS, lambda i: 1 + (i % 4), dev), stage_time([1, 3], VALVE_POINTS, lambda i: 1 + (i % 3), dev)]
    with torch.no_grad():
        arms = {"plain": captured_step(dev, False)[1], "pose": captured_step(dev, True)[1]}
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1],
                           objects=int(arms["pose"].static_out["n_obj"].sum()), what="captured forward_device: replay + synchronise, host wall time, ms")
        del arms
        plain, (pipe, posed) = captured_tick(dev, False)[1], captured_tick(dev, True)
        assert len(pipe.rig_objects(posed.replay())) == 2
        res["tick"] = dict(abba({"plain": plain, "pose": posed}, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", capacity=16, objects=2,
                           what="captured fused tick_device: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
