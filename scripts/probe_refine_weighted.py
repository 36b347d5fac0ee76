"""What weighting the views refinements by the peaks' confidences (okp_refine_pose_views_weighted and its producers) costs next to the
unweighted launches.
(1) The launch alone - replayed as a hipGraph, device time by events around batches of replays - next to the unweighted launch of the SAME
process on the same tensors, 6 iterations, plain and under the Huber loss: the rig of probe_refine_views.py (4 pairs, V = 8, 64 objects of
five points), the rings of probe_window.py (64 streams x 16 track slots, W = 16 and W = 64, every ring full) and the rig windows of
probe_rig_window.py at 128 and 512 views (4 pairs x 16 ticks, 4 pairs x 64 ticks; 64 tracks), every observation with a prior drawn from
{1, 1/4, 1/16}.  The three producers next to theirs in the same way.  (2) The captured 4-pair fused tick with refine = RefineConfig() and
RefineConfig(confidence=...), and the captured batch-64 cups step with window = WindowConfig(16) and WindowConfig(16, confidence=...): both
graphs of a pair live in ONE process and alternate in rounds in A B B A order; a step = replay + synchronise, host wall time.  (3) With
--parent-lib (the parent commit's build of libokp_hip.so) the keyword-off tick and step against that library, selected through OKP_LIB: one
fresh process per turn in A B B A order, twice, both through the ctypes binding; the file states whether the difference of the arms' means
lies inside the scatter of the parent arm's own round medians.  The baseline is always the unweighted launch or the parent build.
Prints one JSON line.

    python scripts/probe_refine_weighted.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_weighted.json]
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
import probe_rig_window as rig_window_probe                              # noqa: E402
import probe_window as window_probe                                      # noqa: E402
from probe_refine import replay_time                                     # noqa: E402
from probe_refine_assignments import abba                                # noqa: E402

NEW_ENTRY_POINTS = ("okp_refine_pose_views_weighted", "okp_refine_pose_views_weighted_wide", "okp_rig_bearings_weighted", "okp_window_push_weighted", "okp_window_push_views_weighted")
HUBER_PX = 0.5
LEVELS = (1.0, 0.25, 0.0625)
REF, FLOOR = 15.8, 1.0                                                   # the sum of p of a clean bump of length scale 2, and a sixteenth of it


def priors_for(obs, seed=9):
    """A prior from LEVELS for every entry of obs [...,S,V,2] that holds a bearing, NaN elsewhere -> a device tensor [...,S,V]."""
    rng = np.random.default_rng(seed)
    seen = torch.isfinite(obs).all(dim=-1).cpu().numpy()
    return torch.from_numpy(np.where(seen, rng.choice(LEVELS, size=seen.shape), np.nan)).to(obs.device)


def _med(us):
    return float(np.median(us))


def _row(name, plain, us_p, weighted, us_w, **shape):
    return dict(shape, what=name, bearings=int(weighted["n_obs"].sum()), accepted_unweighted=int((plain["status"] == 0).sum()), accepted_weighted=int((weighted["status"] == 0).sum()),
                unweighted_median_us=_med(us_p), unweighted_min_us=float(np.min(us_p)), unweighted_max_us=float(np.max(us_p)), weighted_median_us=_med(us_w),
                weighted_min_us=float(np.min(us_w)), weighted_max_us=float(np.max(us_w)), weighted_over_unweighted=_med(us_w) / _med(us_p),
                note="graph replay of the one launch, back to back: launch gaps included; both launches in one process on the same tensors")


def launch_time(dev, iters=6):
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(REF, FLOOR)
    rows, producers = [], []
    t = rig_probe.rig_tick(4, dev)
    bearings = (t["table"], t["count"], t["xyc"], t["match"], t["fused"], rig_probe.ONE_EACH)
    obs, us_b = replay_time(lambda: ops.rig_bearings(*bearings))
    (_, made), us_bw = replay_time(lambda: ops.rig_bearings_weighted(*bearings, cw))
    producers.append(dict(what="rig_bearings (4 pairs, 64 objects) next to rig_bearings_weighted", unweighted_median_us=_med(us_b), weighted_median_us=_med(us_bw),
                          weighted_over_unweighted=_med(us_bw) / _med(us_b), priors=int(torch.isfinite(made).sum()), priors_at_one=int((made == 1.0).sum())))
    prior = priors_for(obs)
    for huber_px in (None, HUBER_PX):
        kw = {} if huber_px is None else {"huber_px": huber_px}
        plain, us_p = replay_time(lambda: ops.refine_pose_views(obs, t["views"], t["pose"], t["n_obj"], t["model"], ops.RefineConfig(iters=iters, **kw)))
        weighted, us_w = replay_time(lambda: ops.refine_pose_views_weighted(obs, prior, t["views"], t["pose"], t["n_obj"], t["model"], ops.RefineConfig(iters=iters, confidence=cw, **kw)))
        rows.append(_row("rig: refine_pose_views next to refine_pose_views_weighted, one table for every object", plain, us_p, weighted, us_w, views=8, objects=rig_probe.OBJECTS,
                         model_points=5, iters=iters, huber_px=huber_px))
    for W in (16, 64):
        w = window_probe.window_tick(W, dev)
        st = w["state"]
        push_args = (w["tab"], w["assignment"], w["status"], w["track"], w["T_WC"], w["cam"])
        pushed, us_push = replay_time(lambda: ops.window_push(st, *push_args, w["cfg"]))
        wst = dict(ops.window_state(window_probe.STREAMS, window_probe.SLOTS, st["win_obs"].shape[2], W, dev, prior=True))
        wcfg = ops.WindowConfig(W, confidence=ops.ConfidenceWeights(0.9, 0.3))
        for k in ("win_obs", "win_views", "win_i"):
            wst[k].copy_(st[k])
        _, us_pushw = replay_time(lambda: ops.window_push(wst, *push_args, wcfg))
        producers.append(dict(what=f"window_push next to its weighted launch, W = {W}, 1024 slots", unweighted_median_us=_med(us_push), weighted_median_us=_med(us_pushw),
                              weighted_over_unweighted=_med(us_pushw) / _med(us_push)))
        start = {"pose": pushed["start"], "assignment": st["win_assignment"]}
        prior = priors_for(st["win_obs"])
        for huber_px in (None, HUBER_PX):
            kw = {} if huber_px is None else {"huber_px": huber_px}
            plain, us_p = replay_time(lambda: ops.refine_pose_views_each(st["win_obs"], st["win_views"], start, st["win_n"], w["model"], ops.WindowConfig(W, iters=iters, **kw)))
            weighted, us_w = replay_time(lambda: ops.refine_pose_views_weighted(st["win_obs"], prior, st["win_views"], start, st["win_n"], w["model"],
                                                                                ops.WindowConfig(W, iters=iters, confidence=cw, **kw), each=True))
            rows.append(_row("window: refine_pose_views_each next to refine_pose_views_weighted, a table per track", plain, us_p, weighted, us_w, views=W,
                             objects=window_probe.STREAMS * window_probe.SLOTS, model_points=4, iters=iters, huber_px=huber_px))
    for P, W in ((4, 16), (4, 64)):
        w = rig_window_probe.window_tick(P, W, dev)
        st = w["state"]
        push_args = (w["assignment"], w["status"], w["track"], w["T_WB"], w["views"])
        pushed, us_push = replay_time(lambda: ops.window_push_views(st, w["obs"], *push_args, w["cfg"]))
        wst = dict(ops.window_views_state(1, rig_window_probe.SLOTS, st["win_obs"].shape[2], W, 2 * P, dev, prior=True))
        for k in ("win_obs", "win_views", "win_i"):
            wst[k].copy_(st[k])
        tick_prior = priors_for(w["obs"])
        _, us_pushw = replay_time(lambda: ops.window_push_views(wst, w["obs"], *push_args, ops.WindowConfig(W, confidence=cw), prior=tick_prior))
        producers.append(dict(what=f"window_push_views next to its weighted launch, {P} pairs x {W} ticks, 64 slots", unweighted_median_us=_med(us_push),
                              weighted_median_us=_med(us_pushw), weighted_over_unweighted=_med(us_pushw) / _med(us_push)))
        start = {"pose": pushed["start"], "assignment": st["win_assignment"]}
        prior = priors_for(st["win_obs"])
        for huber_px in (None, HUBER_PX):
            kw = {} if huber_px is None else {"huber_px": huber_px}
            plain, us_p = replay_time(lambda: ops.refine_pose_views_wide(st["win_obs"], st["win_views"], start, st["win_n"], w["model"], ops.WindowConfig(W, iters=iters, **kw), each=True))
            weighted, us_w = replay_time(lambda: ops.refine_pose_views_weighted(st["win_obs"], prior, st["win_views"], start, st["win_n"], w["model"],
                                                                                ops.WindowConfig(W, iters=iters, confidence=cw, **kw), each=True, wide=True))
            rows.append(_row("rig window: refine_pose_views_wide next to refine_pose_views_weighted, a table per track", plain, us_p, weighted, us_w, views=2 * P * W,
                             objects=rig_window_probe.SLOTS, model_points=5, iters=iters, huber_px=huber_px))
    return rows, producers


def captured_tick(dev, confidence):
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
    kw = {"confidence": confidence} if confidence is not None else {}
    pipe = pp.StereoStreamPipeline(rig_probe.network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, refine=ops.RefineConfig(**kw))
    return pipe, pipe.capture_device(frames, heat_override=heat)


def captured_step(dev, confidence):
    """probe_window.captured_step with the window on, with or without the keyword."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pose = ops.frame_poses(np.tile(np.eye(4), (64, 1, 1))).to(dev)
    kw = {"confidence": confidence} if confidence is not None else {}
    pipe = pp.BatchedKeypointPipeline(window_probe.network(4, dev), {"keypoint_config": [1, 1, 1]}, window_probe.map_camera(), points_3d=window_probe.CUPS_POINTS,
                                      track=ops.TrackConfig(gate=0.1, dt=1 / 30, max_tracks=16), world_frame=True, window=ops.WindowConfig(16, **kw))
    return pipe, pipe.capture(frames, pose)


def one_arm(arm, what, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured tick (refine on) or step (window on) WITHOUT the keyword, n replays in rounds of per_round ->
    one JSON line.  The parent commit's library does not export the new entry points, so the parent arm takes them off the signature table
    before the library is loaded (a keyword-off step never calls them)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = (captured_tick if what == "tick" else captured_step)(dev, None)
        key = "refine" if what == "tick" else "window"
        assert key in step.static_out and "prior" not in step.static_out[key]
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
    names = {"tick": "the captured 4-pair fused tick with the model and refine = RefineConfig(): no confidence",
             "step": "the captured batch-64 cups step with the model, the tracker, the world frame and window = WindowConfig(16): no confidence"}
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
    from object_keypoints_amd import ops
    cw = ops.ConfidenceWeights(REF, FLOOR)
    res = {"probe": "refine_weighted", "confidence": {"ref": REF, "floor": FLOOR}, "prior_levels": list(LEVELS), "huber_px": HUBER_PX, "rounds": args.rounds,
           "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = {what: against_parent_library(args.parent_lib, what, args.rounds * args.per_round // 2, args.warmup) for what in ("tick", "step")}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"], res["producers"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_tick(dev, None)[1], "on": captured_tick(dev, cw)[1]}
        r = arms["on"].static_out["refine"]
        p = r["prior"][torch.isfinite(r["prior"])]
        res["tick"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", keypoint_config=[1, 3], refined=int((r["status"] == 0).sum()),
                           bearings=r["n_obs"][0, :2].tolist(), priors_below_one=int((p < 1.0).sum()), priors=int(p.numel()),
                           what="captured tick_device with rig_poses, the object model and refine; off = RefineConfig(), on = RefineConfig(confidence=ConfidenceWeights(15.8, 1.0)): "
                                "replay + synchronise, host wall time, ms")
        del arms
        arms = {"off": captured_step(dev, None)[1], "on": captured_step(dev, ops.ConfidenceWeights(0.9, 0.3))[1]}
        w = arms["on"].static_out["window"]
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1], ticks=16,
                           refined=int((w["status"] == 0).sum()), filled=int(w["n_views"].max()),
                           what="captured forward_device with the object model, the tracker, the world frame and the window; off = WindowConfig(16), "
                                "on = WindowConfig(16, confidence=ConfidenceWeights(0.9, 0.3)): replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
