"""What the pose refinement under a Huber loss (okp_refine_pose_views_robust, csrc/okp_refine_views.hip) costs next to the plain one.
(1) The launch alone - replayed as a hipGraph, device time by events around batches of replays - next to the plain launch of the SAME
process on the same tensors, 6 iterations: the rig of probe_refine_views.py (4 pairs, V = 8, 64 objects of five points: one table for every
object) and the rings of probe_window.py (64 streams x 16 track slots, W = 16 and W = 64, every ring full: a table per object), each with a
tenth of its bearings displaced by 3 - 10 map pixels, so the weights have something to do.  (2) The captured 4-pair fused tick with
refine = RefineConfig() and RefineConfig(huber_px=0.5), and the captured batch-64 cups step with window = WindowConfig(16) and
WindowConfig(16, huber_px=0.5): both graphs of a pair live in ONE process and alternate in rounds in A B B A order; a step = replay +
synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of libokp_hip.so) the keyword-off tick and step against that
library, selected through OKP_LIB: one fresh process per turn in A B B A order, twice, both through the ctypes binding; the file states
whether the difference of the arms' means lies inside the scatter of the parent arm's own round medians.
Prints one JSON line.

    python scripts/probe_refine_robust.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_robust.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import probe_refine_views as rig_probe                                   # noqa: E402
import probe_window as window_probe                                      # noqa: E402
from probe_refine import replay_time                                     # noqa: E402
from probe_refine_assignments import abba                                # noqa: E402

NEW_ENTRY_POINTS = ("okp_refine_pose_views_robust",)
HUBER_PX = 0.5


def displaced(obs, focal, seed=9, share=0.1):
    """A tenth of the filled bearings of obs [...,S,V,2] moved by 3 - 10 map pixels in a random direction (focal: map pixels) -> a new tensor."""
    rng = np.random.default_rng(seed)
    a = obs.cpu().numpy().copy()
    filled = np.isfinite(a).all(axis=-1)
    hit = filled & (rng.random(filled.shape) < share)
    r, phi = rng.uniform(3.0, 10.0, size=filled.shape), rng.uniform(0.0, 2.0 * np.pi, size=filled.shape)
    a[..., 0][hit] += (r * np.cos(phi))[hit] / focal
    a[..., 1][hit] += (r * np.sin(phi))[hit] / focal
    return torch.from_numpy(a).to(obs.device), int(hit.sum())


def _row(name, plain, us_p, robust, us_r, moved, **shape):
    med = lambda us: float(np.median(us))
    return dict(shape, what=name, displaced_bearings=moved, bearings=int(robust["n_obs"].sum()), down_weighted=int((robust["n_obs"] - robust["n_inlier"])[robust["status"] == 0].sum()),
                accepted_plain=int((plain["status"] == 0).sum()), accepted_robust=int((robust["status"] == 0).sum()), plain_median_us=med(us_p), plain_min_us=float(np.min(us_p)),
                plain_max_us=float(np.max(us_p)), robust_median_us=med(us_r), robust_min_us=float(np.min(us_r)), robust_max_us=float(np.max(us_r)),
                robust_over_plain=med(us_r) / med(us_p), note="graph replay of the one launch, back to back: launch gaps included; both launches in one process on the same tensors")


def launch_time(dev, iters=6):
    from object_keypoints_amd import ops
    rows = []
    t = rig_probe.rig_tick(4, dev)
    focal = float(t["views"][0, 12])
    obs, moved = displaced(ops.rig_bearings(t["table"], t["count"], t["xyc"], t["match"], t["fused"], rig_probe.ONE_EACH), focal)
    run = lambda cfg: replay_time(lambda: ops.refine_pose_views(obs, t["views"], t["pose"], t["n_obj"], t["model"], cfg))
    (plain, us_p), (robust, us_r) = run(ops.RefineConfig(iters=iters)), run(ops.RefineConfig(iters=iters, huber_px=HUBER_PX))
    rows.append(_row("rig: refine_pose_views, one table for every object", plain, us_p, robust, us_r, moved, views=8, objects=rig_probe.OBJECTS, model_points=5, iters=iters))
    for W in (16, 64):
        w = window_probe.window_tick(W, dev)
        st = w["state"]
        start = ops.window_push(st, w["tab"], w["assignment"], w["status"], w["track"], w["T_WC"], w["cam"], w["cfg"])["start"]
        obs, moved = displaced(st["win_obs"], float(w["cam"].fx))
        run = lambda cfg: replay_time(lambda: ops.refine_pose_views_each(obs, st["win_views"], {"pose": start, "assignment": st["win_assignment"]}, st["win_n"], w["model"], cfg))
        (plain, us_p), (robust, us_r) = run(ops.WindowConfig(W, iters=iters)), run(ops.WindowConfig(W, iters=iters, huber_px=HUBER_PX))
        rows.append(_row("window: refine_pose_views_each, a table per track", plain, us_p, robust, us_r, moved, views=W, objects=window_probe.STREAMS * window_probe.SLOTS,
                         model_points=4, iters=iters))
    return rows


def captured_tick(dev, huber_px):
    """probe_refine_views.captured_tick with refine on, with or without the keyword."""
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).to(dev)
    o = synth.rig_fuse_scene()[0]
    pipe = pp.StereoStreamPipeline(rig_probe.network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, refine=ops.RefineConfig(huber_px=huber_px))
    return pipe, pipe.capture_device(frames, heat_override=heat)


def captured_step(dev, huber_px):
    """probe_window.captured_step with the window on, with or without the keyword."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pose = ops.frame_poses(np.tile(np.eye(4), (64, 1, 1))).to(dev)
    pipe = pp.BatchedKeypointPipeline(window_probe.network(4, dev), {"keypoint_config": [1, 1, 1]}, window_probe.map_camera(), points_3d=window_probe.CUPS_POINTS,
                                      track=ops.TrackConfig(gate=0.1, dt=1 / 30, max_tracks=16), world_frame=True, window=ops.WindowConfig(16, huber_px=huber_px))
    return pipe, pipe.capture(frames, pose)


def one_arm(arm, what, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured tick (refine on) or step (window on) WITHOUT the keyword, n replays in rounds of per_round ->
    one JSON line.  The parent commit's library does not export the new entry point, so the parent arm takes it off the signature table before
    the library is loaded (a keyword-off step never calls it)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = (captured_tick if what == "tick" else captured_step)(dev, None)
        key = "refine" if what == "tick" else "window"
        assert key in step.static_out and "n_inlier" not in step.static_out[key]
        lat = []
        for i in range(warmup + n):
            t0 = time.perf_counter()
            step.replay()
            torch.cuda.synchronize()
            if i >= warmup:
                lat.append((time.perf_counter() - t0) * 1e3)
    rounds = [float(np.median(lat[i:i + per_round])) for i in range(0, len(lat) - per_round + 1, per_round)]
    print(json.dumps({"arm": arm, "lib": _lib.LIB_PATH, "median_ms": float(np.median(lat)), "p99_ms": float(np.percentile(lat, 99)), "round_medians_ms": rounds}))


def against_parent_library(parent_lib, what, n, warmup):
    """One fresh process per turn, A B B A twice; the first failure ends the series."""
    from object_keypoints_amd import _lib
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    runs, rounds = {"parent": [], "this": []}, {"parent": [], "this": []}
    order = ("parent", "this", "this", "parent", "parent", "this", "this", "parent")
    for arm in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--what", what, "--per-round", str(n), "--warmup", str(warmup)]
        done = subprocess.run(cmd, env=dict(os.environ, OKP_LIB=libs[arm]), capture_output=True, text=True, timeout=240)
        if done.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} ended with {done.returncode}:\n{done.stderr[-2000:]}")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        runs[arm].append(line["median_ms"])
        rounds[arm] += line["round_medians_ms"]
    mean = {arm: float(np.mean(v)) for arm, v in runs.items()}
    spread = {arm: 1e3 * (max(v) - min(v)) for arm, v in rounds.items()}
    diff = (mean["this"] - mean["parent"]) * 1e3
    names = {"tick": "the captured 4-pair fused tick with the model and refine = RefineConfig(): no huber_px",
             "step": "the captured batch-64 cups step with the model, the tracker, the world frame and window = WindowConfig(16): no huber_px"}
    return {"order": " ".join(order) + ", one process each", "replays_per_process": n, "replays_per_round": 30, "what": names[what], "parent_median_ms": runs["parent"],
            "this_median_ms": runs["this"], "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_medians_ms": [round(v, 4) for v in rounds["parent"]], "this_round_medians_ms": [round(v, 4) for v in rounds["this"]],
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"],
            "parent_process_spread_us": 1e3 * (max(runs["parent"]) - min(runs["parent"])), "inside_parent_round_spread": bool(abs(diff) <= spread["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the keyword-off tick and step against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--what", choices=["tick", "step"], default="tick", help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.what, args.per_round, args.warmup)
    res = {"probe": "refine_robust", "huber_px": HUBER_PX, "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = {what: against_parent_library(args.parent_lib, what, args.rounds * args.per_round // 2, args.warmup) for what in ("tick", "step")}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_tick(dev, None)[1], "on": captured_tick(dev, HUBER_PX)[1]}
        r = arms["on"].static_out["refine"]
        res["tick"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", keypoint_config=[1, 3], refined=int((r["status"] == 0).sum()),
                           bearings=r["n_obs"][0, :2].tolist(), inliers=r["n_inlier"][0, :2].tolist(),
                           what="captured tick_device with rig_poses, the object model and refine; off = RefineConfig(), on = RefineConfig(huber_px=0.5): replay + synchronise, host wall time, ms")
        del arms
        arms = {"off": captured_step(dev, None)[1], "on": captured_step(dev, HUBER_PX)[1]}
        w = arms["on"].static_out["window"]
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1], ticks=16,
                           refined=int((w["status"] == 0).sum()), filled=int(w["n_views"].max()),
                           what="captured forward_device with the object model, the tracker, the world frame and the window; off = WindowConfig(16), on = WindowConfig(16, huber_px=0.5): "
                                "replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
