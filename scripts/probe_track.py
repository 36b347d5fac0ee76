"""What the tracking stage (okp_track_objects, csrc/okp_track.hip) costs.  (1) The launch alone, replayed as a hipGraph - device time by events
around batches of replays - at (B, T, max_obj) = (1, 16, 16) and (64, 64, 16), every stream holding max_obj objects that step a centimetre per
tick, so that every call predicts, gates, associates and filters max_obj tracks per stream.  (2) The captured fused tick of four posed pairs
with the object model, with and without `track`: both graphs live in ONE process and alternate in rounds in A B B A order, so that drift of the
host or the GPU falls on both; a tick = replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of
libokp_hip.so) the same captured tick against THAT library, selected through OKP_LIB: one fresh process per arm in A B B A order (parent library
without a tracker, this tree's library with one; both through the ctypes binding, which OKP_LIB selects - a replay marshals nothing either
way); it carries the process-to-process scatter of a capture on top.  Prints one JSON line.

    python scripts/probe_track.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/track.json]
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
sys.path.insert(0, os.path.join(REPO, "scripts"))

NEW_ENTRY_POINTS = ("okp_track_objects",)
MODEL = [[0.0, 0.0, 0.0], [0.10, 0.0, 0.0], [-0.04, 0.09, 0.01], [-0.05, -0.08, 0.03]]


def config(max_tracks=16):
    from object_keypoints_amd import ops
    return ops.TrackConfig(gate=0.1, dt=1.0 / 30.0, alpha=0.5, beta=0.1, alpha_R=0.5, min_hits=2, max_misses=5, max_tracks=max_tracks)


def launch_time(B, T, max_obj, dev, batches=30, per_batch=50):
    """The launch alone: two alternating ticks (the objects a centimetre apart) so that every replay matches and blends every track."""
    from object_keypoints_amd import ops
    S = len(MODEL)
    model = torch.tensor(MODEL, dtype=torch.float64, device=dev)
    cfg = config(T)
    ticks = []
    for shift in (0.0, 0.01):
        z = np.stack([np.array([(o % 4) * 0.5 + shift, (o // 4) * 0.5, 1.0 + 0.01 * b]) for b in range(B) for o in range(max_obj)]).reshape(B, max_obj, 3)
        c, s = np.cos(0.1 + shift), np.sin(0.1 + shift)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        pose = np.concatenate([np.broadcast_to(R, (B, max_obj, 3, 3)), (z - R @ np.array(MODEL[0]))[..., None]], axis=3).reshape(B, max_obj, 12)
        tab = np.full((B, max_obj, S, 4), np.nan)
        tab[:, :, 0, :3], tab[:, :, 0, 3] = z, 1.0
        ticks.append((torch.from_numpy(tab).to(dev), torch.from_numpy(pose).to(dev)))
    status = torch.zeros((B, max_obj), dtype=torch.int32, device=dev)
    n_obj = torch.full((B,), max_obj, dtype=torch.int32, device=dev)
    state = ops.track_state(B, T, dev)

    def both():
        for tab, pose in ticks:
            out = ops.track_objects(state, tab, pose, status, n_obj, model, cfg)
        return out

    for _ in range(3):
        out = both()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = both()
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
        us.append(a.elapsed_time(b) * 1e3 / (2 * per_batch))
    assert int(out["n_tracks"].sum()) == B * min(T, max_obj) and int(out["overflow"]) == 0
    return {"B": B, "T": T, "max_obj": max_obj, "tracks": int(out["n_tracks"].sum()), "median_us": float(np.median(us)), "min_us": float(np.min(us)),
            "max_us": float(np.max(us)), "note": "graph replay of two launches back to back, per launch: launch gaps included"}


def abba(arms, rounds, per_round, warmup):
    """arms: {"plain": tick, "track": tick} of captured ticks -> per-arm medians, per-round spans and their difference."""
    def tick(name):
        arms[name].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(warmup):
            tick(name)
    lat, meds = {n: [] for n in arms}, {n: [] for n in arms}
    order = ["plain", "track", "track", "plain"]
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
    res["track_minus_plain_us"] = (res["track"]["median_ms"] - res["plain"]["median_ms"]) * 1e3
    res["track_over_plain_percent"] = 100.0 * (res["track"]["median_ms"] / res["plain"]["median_ms"] - 1.0)
    return res


def captured_tick(dev, with_track):
    """The captured fused tick of four posed pairs with the object model, with or without the tracker."""
    from probe_object_pose import network
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
    kw = dict(rig_poses=poses, merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
              points_3d=np.concatenate([o[1], o[2]]))
    if with_track:
        kw["track"] = config()
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5, **kw)
    return pipe, pipe.capture_device(frames, heat_override=heat)


def one_arm(arm, n, warmup):
    """Child process of --parent-lib: one captured tick, n replays -> one JSON line.  The parent commit's library does not export the new entry
    point, so the parent arm takes it off the signature table before the library is loaded (it never calls it)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_tick(dev, arm == "track")
        assert ("track" in step.static_out) == (arm == "track")
        lat = []
        for i in range(warmup + n):
            t0 = time.perf_counter()
            step.replay()
            torch.cuda.synchronize()
            if i >= warmup:
                lat.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"arm": arm, "lib": _lib.LIB_PATH, "median_ms": float(np.median(lat)), "p99_ms": float(np.percentile(lat, 99))}))


def against_parent_library(parent_lib, n, warmup):
    """One fresh process per arm, A B B A; the first failure ends the series."""
    from object_keypoints_amd import _lib
    libs = {"parent": os.path.abspath(parent_lib), "track": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    runs = {"parent": [], "track": []}
    for arm in ("parent", "track", "track", "parent"):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--per-round", str(n), "--warmup", str(warmup)]
        done = subprocess.run(cmd, env=dict(os.environ, OKP_LIB=libs[arm]), capture_output=True, text=True, timeout=240)
        if done.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} ended with {done.returncode}:\n{done.stderr[-2000:]}")
        runs[arm].append(json.loads(done.stdout.strip().splitlines()[-1])["median_ms"])
    mean = {arm: float(np.mean(v)) for arm, v in runs.items()}
    return {"order": "parent track track parent, one process each", "replays_per_process": n, "parent_median_ms": runs["parent"], "track_median_ms": runs["track"],
            "track_minus_parent_us": (mean["track"] - mean["parent"]) * 1e3, "track_over_parent_percent": 100.0 * (mean["track"] / mean["parent"] - 1.0),
            "process_scatter_us": 1e3 * max(abs(v[0] - v[1]) for v in runs.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the captured tick against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "track"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "track", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = [launch_time(1, 16, 16, dev), launch_time(64, 64, 16, dev)]
    with torch.no_grad():
        plain, (pipe, tracked) = captured_tick(dev, False)[1], captured_tick(dev, True)
        assert len(pipe.rig_tracks(tracked.replay())) >= 1
        res["tick"] = dict(abba({"plain": plain, "track": tracked}, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", capacity=16, objects=2,
                           what="captured fused tick_device with the object model: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
