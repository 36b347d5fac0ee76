"""What the sliding window of a rig (okp_window_push_views + okp_refine_pose_views_wide, csrc/okp_window_views.hip /
csrc/okp_refine_views_wide.hip) costs.
(1) The two launches alone - replayed as a hipGraph, device time by events around batches of replays - on 64 track slots (one stream), S = 5
model rows, 6 iterations, every ring full, for (pairs, ticks) = (4, 8), (4, 16), (4, 64) and (32, 8), plain and under a Huber loss with a tenth
of the ring's bearings displaced; next to them, in the same process, okp_refine_pose_views_each on 64 objects x 64 views.  (2) The captured
4-pair fused tick (fp16 network, the object model, the tracker and the world frame) with `rig_window` on and off: both graphs live in ONE
process and alternate in rounds in A B B A order; a tick = replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's
build of libokp_hip.so) the captured tick with rig_window OFF against that library, selected through OKP_LIB: one fresh process per turn in
A B B A order, twice, both through the ctypes binding, each process timing its replays in rounds; the file states whether the difference of
the arms' means lies inside the scatter of the parent arm's own round medians.
Prints one JSON line.

    python scripts/probe_rig_window.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/rig_window.json]
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
from probe_refine_robust import HUBER_PX, displaced                      # noqa: E402
from probe_refine_views import ONE_EACH, _rotation                       # noqa: E402

NEW_ENTRY_POINTS = ("okp_window_push_views", "okp_refine_pose_views_wide")
SLOTS = 64
SHAPES = ((4, 8), (4, 16), (4, 64), (32, 8))


def rig_views(P):
    """The views table of a rig of P pairs of the map camera (0.1 m baselines, yawed -30 .. +30 degrees on a 0.4 m arc), as probe_refine_views builds it."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = map_camera()
    T_RL = np.eye(4)
    T_RL[0, 3] = -0.1
    T_BL = []
    for p in range(P):
        a = np.radians(-30.0 + 60.0 * p / (P - 1))
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]]
        T[:3, 3] = [0.2 * np.sin(a), 0.0, 0.0]
        T_BL.append(T)
    return ops.rig_views(cu.StereoCamera(cam, cam, T_RL), T_BL)


def window_tick(P, W, dev, huber_px=None, seed=5):
    """One stream of 64 static objects of the valve-like model, every one a live track measured in this tick, and a window state filled by W
    pushes from a rig of P pairs that moves 0.32 m and yaws 0.16 rad over them (2 cm and 0.01 rad per tick at W = 16): exact bearings in
    every camera, 0.1 map pixels of noise -> what window_push_views and refine_pose_views_wide take."""
    from object_keypoints_amd import ops
    rng = np.random.default_rng(seed)
    views = rig_views(P).numpy()
    V = 2 * P
    model = ops.object_model(VALVE_POINTS, ONE_EACH).numpy()
    S = model.shape[0]
    R = np.stack([_rotation(rng) for _ in range(SLOTS)])
    t = np.concatenate([rng.uniform(-0.15, 0.15, size=(SLOTS, 2)), rng.uniform(0.8, 1.2, size=(SLOTS, 1))], axis=1)
    X_W = np.einsum("tij,sj->tsi", R, model) + t[:, None, :]
    track_pose = np.concatenate([np.einsum("ij,tjk->tik", _rotation(rng, 0.02), R), (t + rng.normal(scale=0.005, size=t.shape))[..., None]], axis=2).reshape(1, SLOTS, 12)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    track_i = np.zeros((1, SLOTS, 4), dtype=np.int32)                              # id = slot + 1, one hit, no miss, age 1
    track_i[..., 0], track_i[..., 1], track_i[..., 3] = np.arange(1, SLOTS + 1), 1, 1
    track = {"meas_of": to(np.arange(SLOTS, dtype=np.int32)[None]), "track_f": to(np.zeros((1, SLOTS, 16))), "track_pose": to(track_pose), "track_i": to(track_i)}
    fixed = dict(assignment=to(np.tile(np.arange(S, dtype=np.int32), (1, SLOTS, 1))), status=to(np.zeros((1, SLOTS), dtype=np.int32)))
    cfg = ops.WindowConfig(W, huber_px=huber_px)
    state = ops.window_views_state(1, SLOTS, S, W, V, dev)
    views_dev = to(views)
    d = np.array([0.9, 0.3, 0.3]) / np.linalg.norm([0.9, 0.3, 0.3])
    Rv, tv = views[:, :12].reshape(V, 3, 4)[:, :, :3], views[:, :12].reshape(V, 3, 4)[:, :, 3]
    for k in range(W):                                                             # the same path for every W: 0.32 m and 0.16 rad, in W steps
        a = 0.16 * k / W
        Rb, tb = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]), 0.32 * k / W * d
        X_B = (X_W - tb) @ Rb                                                      # R^T (X - t), row vectors
        q = np.einsum("vij,tsj->tsvi", Rv, X_B) + tv
        obs = q[..., :2] / q[..., 2:3] + rng.normal(scale=0.1, size=q[..., :2].shape) / views[:, 12:14]
        if huber_px is not None:
            obs = displaced(torch.from_numpy(obs), float(views[0, 12]), seed=9 + k)[0].numpy()
        obs, T_WB = to(obs[None]), to(np.concatenate([Rb, tb[:, None]], axis=1).reshape(1, 12))
        last = dict(obs=obs, T_WB=T_WB)
        ops.window_push_views(state, obs, fixed["assignment"], fixed["status"], track, T_WB, views_dev, cfg)
    return dict(state=state, track=track, cfg=cfg, views=views_dev, model=to(model), **fixed, **last)


def launch_time(dev):
    from object_keypoints_amd import ops
    med = lambda us: float(np.median(us))
    rows = []
    for P, W in SHAPES:
        for huber_px in (None, HUBER_PX):
            w = window_tick(P, W, dev, huber_px)
            st = w["state"]
            push = lambda: ops.window_push_views(st, w["obs"], w["assignment"], w["status"], w["track"], w["T_WB"], w["views"], w["cfg"])
            refine = lambda start: ops.refine_pose_views_wide(st["win_obs"], st["win_views"], {"pose": start, "assignment": st["win_assignment"]}, st["win_n"], w["model"],
                                                              w["cfg"], each=True)
            pushed, us_p = replay_time(push)
            res, us_r = replay_time(lambda: refine(pushed["start"]))
            _, us_both = replay_time(lambda: refine(push()["start"]))
            rows.append({"pairs": P, "ticks": W, "views": 2 * P * W, "track_slots": SLOTS, "model_rows": 5, "iters": w["cfg"].iters, "huber_px": huber_px,
                         "filled_ticks": int(pushed["n_views"].min()), "bearings_per_track": int(res["n_obs"][0, 0]), "accepted": int((res["status"] == 0).sum()), "of": SLOTS,
                         "inliers_per_track_median": float(res["n_inlier"].double().median()) if "n_inlier" in res else None,
                         "window_push_views_median_us": med(us_p), "window_push_views_min_us": float(np.min(us_p)), "refine_wide_median_us": med(us_r),
                         "refine_wide_min_us": float(np.min(us_r)), "refine_wide_max_us": float(np.max(us_r)), "both_launches_median_us": med(us_both),
                         "note": "graph replay of the launch(es), back to back: launch gaps included; every one of the 64 slots is live, measured and has a full ring"})
    return rows


def one_wave_time(dev):
    """okp_refine_pose_views_each on 64 objects x 64 views (one wave per object) in the same process: the ring of (4, 8), handed over as is."""
    from object_keypoints_amd import ops
    w = window_tick(4, 8, dev)
    st = w["state"]
    start = ops.window_push_views(st, w["obs"], w["assignment"], w["status"], w["track"], w["T_WB"], w["views"], w["cfg"])["start"]
    pose = {"pose": start, "assignment": st["win_assignment"]}
    cfg = ops.RefineConfig()
    old, us_old = replay_time(lambda: ops.refine_pose_views_each(st["win_obs"], st["win_views"], pose, st["win_n"], w["model"], cfg))
    new, us_new = replay_time(lambda: ops.refine_pose_views_wide(st["win_obs"], st["win_views"], pose, st["win_n"], w["model"], cfg, each=True))
    same = all(torch.equal(old[k].view(torch.uint8), new[k].view(torch.uint8)) for k in old)
    return {"objects": SLOTS, "views": 64, "model_rows": 5, "iters": cfg.iters, "refine_each_median_us": float(np.median(us_old)), "refine_each_min_us": float(np.min(us_old)),
            "refine_wide_median_us": float(np.median(us_new)), "refine_wide_min_us": float(np.min(us_new)), "same_bits": bool(same),
            "accepted": int((old["status"] == 0).sum())}


def captured_tick(dev, rig_window):
    """The captured 4-pair fused tick (fp16 network, the rig of synth.stereo_rig looking at synth.rig_fuse_scene) with the object model, the
    tracker and the world frame, rig_window on or off."""
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).to(dev)
    pose = ops.frame_poses(np.eye(4)[None]).to(dev)
    o = synth.rig_fuse_scene()[0]
    kw = {"rig_window": ops.WindowConfig(16)} if rig_window else {}
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, track=ops.TrackConfig(gate=0.1, dt=1 / 30, max_tracks=16), world_frame=True, **kw)
    return pipe, pipe.capture_device(frames, heat_override=heat, rig_pose=pose)


def one_arm(arm, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured tick with rig_window off, n replays in rounds of per_round -> one JSON line.  The parent
    commit's library does not export the new entry points, so the parent arm takes them off the signature table before the library is loaded."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_tick(dev, False)
        assert "window" not in step.static_out and "track" in step.static_out
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
            "what": "the captured 4-pair fused tick with the model, the tracker and the world frame, rig_window off", "parent_median_ms": runs["parent"],
            "this_median_ms": runs["this"], "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_medians_ms": [round(v, 4) for v in rounds["parent"]], "this_round_medians_ms": [round(v, 4) for v in rounds["this"]],
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"],
            "parent_process_spread_us": 1e3 * (max(runs["parent"]) - min(runs["parent"])), "inside_parent_round_spread": bool(abs(diff) <= spread["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the tick with rig_window off against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "rig_window", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    res["one_wave"] = one_wave_time(dev)
    with torch.no_grad():
        arms = {"off": captured_tick(dev, False)[1], "on": captured_tick(dev, True)[1]}
        w = arms["on"].static_out["window"]
        res["tick"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), pairs=4, dtype="float16", keypoint_config=[1, 3], ticks=16,
                           live_tracks=int(arms["on"].static_out["track"]["n_tracks"].sum()), refined=int((w["status"] == 0).sum()), filled=int(w["n_views"].max()),
                           what="captured tick_device of four posed pairs with the object model, the tracker and the world frame: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
