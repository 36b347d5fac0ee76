"""What refining a rig's poses against every camera's bearings (okp_rig_bearings + okp_refine_pose_views, csrc/okp_refine_views.hip) costs.
(1) The two launches alone - replayed as a hipGraph, device time by events around batches of replays - on 64 objects of a five-point model,
6 iterations, for a rig of P = 4 pairs (every object in all 8 views: 40 bearings each) and of P = 32 pairs (every object in 16 of them: 160
bearings each), next to okp_refine_pose at B = 1, max_obj = 64 on the same objects in the same process as the yardstick.  (2) The captured
4-pair fused tick (fp16 network, tick_device with the object model) with `refine` on and off: both graphs live in ONE process and alternate in
rounds in A B B A order; a tick = replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of libokp_hip.so)
the captured tick with refine OFF against that library, selected through OKP_LIB: one fresh process per turn in A B B A order, twice, both
through the ctypes binding, each process timing its replays in rounds - what the new entry points did to the tick a user who does not ask for them runs;
the file states whether the difference of the arms' means lies inside the scatter of the parent arm's own round medians.
Prints one JSON line.

    python scripts/probe_refine_views.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_views.json]
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

from probe_object_pose import VALVE_POINTS, map_camera, network          # noqa: E402
from probe_refine import replay_time                                     # noqa: E402
from probe_refine_assignments import abba                                # noqa: E402

NEW_ENTRY_POINTS = ("okp_rig_bearings", "okp_refine_pose_views")
ONE_EACH = [1, 1, 1, 1]                # the valve-like model with every key point a type of its own: S = 5, one assignment
OBJECTS = 64


def _rotation(rng, angle=None):
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    a = rng.uniform(0.0, np.pi) if angle is None else angle
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def rig_tick(P, dev, seed=5):
    """A fabricated fused tick of a rig of P pairs of the map camera (0.1 m baselines, yawed -30 .. +30 degrees on a 0.4 m arc) that sees 64
    objects at 0.8 .. 1.2 m: pair p sees every object (P = 4) or the objects of its own parity (P = 32: 32 peaks per map), at the exact
    projections of the model's points -> what rig_bearings and refine_pose_views take, and the same objects as a table for refine_pose."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rng = np.random.default_rng(seed)
    cam = map_camera()
    T_RL = np.eye(4)
    T_RL[0, 3] = -0.1
    stereo = cu.StereoCamera(cam, cam, T_RL)
    T_BL = []
    for p in range(P):
        a = np.radians(-30.0 + 60.0 * p / (P - 1))
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]]
        T[:3, 3] = [0.2 * np.sin(a), 0.0, 0.0]
        T_BL.append(T)
    views = ops.rig_views(stereo, T_BL)
    model = ops.object_model(VALVE_POINTS, ONE_EACH).numpy()
    S, K = model.shape[0], model.shape[0]
    every = P <= 4
    cap = OBJECTS if every else OBJECTS // 2
    count = np.full((2 * P, K), cap, dtype=np.int32)
    xyc = np.zeros((2 * P, K, cap, 3), dtype=np.float32)
    match = np.tile(np.arange(cap, dtype=np.int32), (P, K, 1))
    member = np.zeros((P, K, cap), dtype=np.int32)
    tab, pose = np.zeros((1, OBJECTS, S, 4)), np.zeros((1, OBJECTS, 12))
    for o in range(OBJECTS):
        R, t = _rotation(rng), np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.8, 1.2)])
        X = model @ R.T + t
        tab[0, o] = np.concatenate([X, np.full((S, 1), 0.9)], axis=1)
        pose[0, o] = np.concatenate([_rotation(rng, 0.05) @ R, (t + rng.normal(scale=0.01, size=3))[:, None]], axis=1).reshape(12)
        for p in range(P):
            if not every and (o - p) % 2:
                continue
            i = o if every else o // 2
            member[p, :, i] = o
            for v, c in ((2 * p, stereo.left_camera), (2 * p + 1, stereo.right_camera)):
                M = np.eye(4)
                M[:3] = views[v, :12].reshape(3, 4).numpy()
                xyc[v, :, i, :2] = c.project(X, M)
                xyc[v, :, i, 2] = 0.9
    to = lambda x: torch.from_numpy(x).to(dev)
    fused = {"member": to(member), "object": to(np.tile(np.arange(OBJECTS, dtype=np.int32), (K, 1))), "n_fused": to(np.full(K, OBJECTS, dtype=np.int32))}
    fit = {"pose": to(pose), "assignment": to(np.tile(np.arange(S, dtype=np.int32), (1, OBJECTS, 1)))}
    return dict(table=ops.stereo_rig([stereo]).to(dev), count=to(count), xyc=to(xyc), match=to(match), fused=fused, views=views.to(dev), pose=fit, tab=to(tab),
                n_obj=torch.full((1,), OBJECTS, dtype=torch.int32, device=dev), model=to(model))


def launch_time(dev, iters=6):
    from object_keypoints_amd import ops
    cfg, cam = ops.RefineConfig(iters=iters), map_camera().okp()
    rows = []
    for P in (4, 32):
        t = rig_tick(P, dev)
        bearings = lambda: ops.rig_bearings(t["table"], t["count"], t["xyc"], t["match"], t["fused"], ONE_EACH)
        obs, us_b = replay_time(bearings)
        res, us_r = replay_time(lambda: ops.refine_pose_views(obs, t["views"], t["pose"], t["n_obj"], t["model"], cfg))
        _, us_both = replay_time(lambda: ops.refine_pose_views(bearings(), t["views"], t["pose"], t["n_obj"], t["model"], cfg))
        ref, us_y = replay_time(lambda: ops.refine_pose(t["tab"], t["pose"], t["n_obj"], t["model"], cam, cfg))
        med = lambda us: float(np.median(us))
        rows.append({"pairs": P, "views": 2 * P, "objects": OBJECTS, "model_points": 5, "iters": iters, "bearings_per_object": int(res["n_obs"][0, 0]),
                     "accepted": int((res["status"] == 0).sum()), "rig_bearings_median_us": med(us_b), "rig_bearings_min_us": float(np.min(us_b)),
                     "refine_pose_views_median_us": med(us_r), "refine_pose_views_min_us": float(np.min(us_r)), "refine_pose_views_max_us": float(np.max(us_r)),
                     "both_launches_median_us": med(us_both), "refine_pose_median_us": med(us_y), "refine_pose_accepted": int((ref["status"] == 0).sum()),
                     "views_over_refine_pose": med(us_r) / med(us_y), "note": "graph replay of the launch(es), back to back: launch gaps included; refine_pose at B = 1, "
                     "max_obj = 64 on the same objects is the yardstick"})
    return rows


def captured_tick(dev, refine):
    """The captured 4-pair fused tick (fp16 network, the rig of synth.stereo_rig looking at synth.rig_fuse_scene) with the object model, refine on or off."""
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).to(dev)
    o = synth.rig_fuse_scene()[0]
    kw = {"refine": ops.RefineConfig()} if refine else {}
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, **kw)
    return pipe, pipe.capture_device(frames, heat_override=heat)


def one_arm(arm, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured tick with refine off, n replays in rounds of per_round -> one JSON line.  The parent commit's library does not export
    the new entry points, so the parent arm takes them off the signature table before the library is loaded (it never calls them)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_tick(dev, False)
        assert "refine" not in step.static_out and "pose" in step.static_out
        lat = []
        for i in range(warmup + n):
            t0 = time.perf_counter()
            step.replay()
            torch.cuda.synchronize()
            if i >= warmup:
                lat.append((time.perf_counter() - t0) * 1e3)
    rounds = [float(np.median(lat[i:i + per_round])) for i in range(0, len(lat) - per_round + 1, per_round)]
    print(json.dumps({"arm": arm, "lib": _lib.LIB_PATH, "median_ms": float(np.median(lat)), "p99_ms": float(np.percentile(lat, 99)), "round_medians_ms": rounds}))


def against_parent_library(parent_lib, n, warmup):
    """One fresh process per turn, A B B A twice; the first failure ends the series."""
    from object_keypoints_amd import _lib
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    runs, rounds = {"parent": [], "this": []}, {"parent": [], "this": []}
    order = ("parent", "this", "this", "parent", "parent", "this", "this", "parent")
    for arm in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--per-round", str(n), "--warmup", str(warmup)]
        done = subprocess.run(cmd, env=dict(os.environ, OKP_LIB=libs[arm]), capture_output=True, text=True, timeout=240)
        if done.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} ended with {done.returncode}:\n{done.stderr[-2000:]}")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        runs[arm].append(line["median_ms"])
        rounds[arm] += line["round_medians_ms"]
    mean = {arm: float(np.mean(v)) for arm, v in runs.items()}
    spread = {arm: 1e3 * (max(v) - min(v)) for arm, v in rounds.items()}
    diff = (mean["this"] - mean["parent"]) * 1e3
    return {"order": " ".join(order) + ", one process each", "replays_per_process": n, "replays_per_round": 30,
            "what": "the captured 4-pair fused tick with the model, refine off", "parent_median_ms": runs["parent"], "this_median_ms": runs["this"],
            "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_medians_ms": [round(v, 4) for v in rounds["parent"]], "this_round_medians_ms": [round(v, 4) for v in rounds["this"]],
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"],
            "parent_process_spread_us": 1e3 * (max(runs["parent"]) - min(runs["parent"])), "inside_parent_round_spread": bool(abs(diff) <= spread["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the tick with refine off against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "refine_views", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_tick(dev, False)[1], "on": captured_tick(dev, True)[1]}
        r = arms["on"].static_out["refine"]
        res["tick"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", keypoint_config=[1, 3],
                           objects=int(arms["on"].static_out["fused"]["n_obj"]), refined=int((r["status"] == 0).sum()), bearings=r["n_obs"][0, :2].tolist(),
                           what="captured tick_device with rig_poses and the object model: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
