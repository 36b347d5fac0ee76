"""What the window refinement of a moving object (okp_window_push_timed / okp_window_push_views_timed + okp_refine_motion_views,
csrc/okp_refine_motion.hip) costs.
(1) okp_refine_motion_views next to okp_refine_pose_views_each in the same process ON THE SAME TENSORS - 64 streams x 16 track slots, the
valve-like model (S = 5), rings of W = 16 and W = 64 ticks filled by timed pushes of objects that translate at 0.2 m/s past a moving camera,
6 iterations - each replayed back to back as a hipGraph, device time by events around batches of replays, and their ratio.  (2) The two timed
pushes next to the plain pushes, the same way.  (3) The captured batch-64 cups step (window of 16 ticks) and the captured 4-pair x 8-tick
fused tick (rig_window of 8 ticks), with and without motion: both graphs live in ONE process and alternate in rounds in A B B A order; a step
= replay + synchronise, host wall time.  (4) With --parent-lib (the parent commit's build of libokp_hip.so) the captured cups step WITHOUT
the keyword against that library, selected through OKP_LIB: one fresh process per turn in the order parent, this, this, parent, each process
timing its replays in rounds; the file states whether the difference of the arms' means lies inside the scatter of the parent arm's own
round medians - inside it the difference is not resolved.
Prints one JSON line.

    python scripts/probe_refine_motion.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_motion.json]
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

from probe_object_pose import CUPS_POINTS, VALVE_POINTS, map_camera, network          # noqa: E402
from probe_refine import replay_time                                                   # noqa: E402
from probe_refine_assignments import abba                                              # noqa: E402
from probe_refine_views import ONE_EACH, _rotation                                     # noqa: E402
from probe_rig_window import rig_views                                                 # noqa: E402

NEW_ENTRY_POINTS = ("okp_window_push_timed", "okp_window_push_views_timed", "okp_refine_motion_views")
STREAMS, SLOTS, DT, SPEED = 64, 16, 0.1, 0.2
MOTION = "constant_velocity"


def _scene(B, T, rng, dev):
    from object_keypoints_amd import ops
    model = ops.object_model(VALVE_POINTS, ONE_EACH).numpy()
    S = model.shape[0]
    R = np.stack([[_rotation(rng) for _ in range(T)] for _ in range(B)])
    t = np.concatenate([rng.uniform(-0.15, 0.15, size=(B, T, 2)), rng.uniform(0.8, 1.2, size=(B, T, 1))], axis=2)
    nu = rng.normal(size=(B, T, 3))
    nu *= SPEED / np.linalg.norm(nu, axis=2, keepdims=True)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    track_i = np.zeros((B, T, 4), dtype=np.int32)                                    # id = slot + 1, one hit, no miss, age 1
    track_i[..., 0], track_i[..., 1], track_i[..., 3] = np.arange(1, T + 1), 1, 1
    fixed = dict(assignment=to(np.tile(np.arange(S, dtype=np.int32), (B, T, 1))), status=to(np.zeros((B, T), dtype=np.int32)))
    return model, S, R, t, nu, to, track_i, fixed


def _track(B, T, R, t_now, rng, to, track_i):
    pose = np.concatenate([np.einsum("ij,btjk->btik", _rotation(rng, 0.02), R), (t_now + rng.normal(scale=0.005, size=t_now.shape))[..., None]], axis=3).reshape(B, T, 12)
    return {"meas_of": to(np.tile(np.arange(T, dtype=np.int32), (B, 1))), "track_f": to(np.zeros((B, T, 16))), "track_pose": to(pose), "track_i": to(track_i)}


def _path(k, W):
    """The camera (or rig) of push k of W: 0.32 m and 0.16 rad over the W pushes, whatever W is."""
    d = np.array([0.9, 0.3, 0.3]) / np.linalg.norm([0.9, 0.3, 0.3])
    a = 0.16 * k / W
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]), 0.32 * k / W * d


def camera_tick(W, dev, seed=5):
    """64 streams of 16 objects of the valve-like model that translate at 0.2 m/s (0.1 s per tick), every one a live track measured in every
    tick, and a TIMED window state filled by W pushes -> what window_push, refine_pose_views_each and refine_motion_views take."""
    from object_keypoints_amd import ops
    rng = np.random.default_rng(seed)
    cam = map_camera().okp()
    model, S, R, t, nu, to, track_i, fixed = _scene(STREAMS, SLOTS, rng, dev)
    track = _track(STREAMS, SLOTS, R, t + (W - 1) * DT * nu, rng, to, track_i)
    cfg, plain = ops.WindowConfig(W, motion=MOTION), ops.WindowConfig(W)
    state, twin = ops.window_state(STREAMS, SLOTS, S, W, dev, timed=True), ops.window_state(STREAMS, SLOTS, S, W, dev)
    for k in range(W):
        Rc, tc = _path(k, W)
        X_W = np.einsum("btij,sj->btsi", R, model) + (t + k * DT * nu)[:, :, None, :]
        X_C = (X_W - tc) @ Rc                                                       # R^T (X - t), row vectors
        tab = to(np.concatenate([X_C, np.full(X_C.shape[:3] + (1,), 0.9)], axis=3))
        T_WC = to(np.tile(np.concatenate([Rc, tc[:, None]], axis=1).reshape(12), (STREAMS, 1)))
        last = dict(tab=tab, T_WC=T_WC)
        pushed = ops.window_push(state, tab, fixed["assignment"], fixed["status"], track, T_WC, cam, cfg)
        ops.window_push(twin, tab, fixed["assignment"], fixed["status"], track, T_WC, cam, plain)
    return dict(state=state, twin=twin, track=track, cam=cam, cfg=cfg, plain=plain, model=to(model), pushed=pushed, **fixed, **last)


def rig_tick(P, W, dev, seed=6):
    """One stream of 64 such objects under a rig of P pairs, and a timed and a plain window state filled by W pushes."""
    from object_keypoints_amd import ops
    rng = np.random.default_rng(seed)
    views = rig_views(P).numpy()
    V = 2 * P
    model, S, R, t, nu, to, track_i, fixed = _scene(1, 64, rng, dev)
    track = _track(1, 64, R, t + (W - 1) * DT * nu, rng, to, track_i)
    cfg, plain = ops.WindowConfig(W, motion=MOTION), ops.WindowConfig(W)
    state, twin = ops.window_views_state(1, 64, S, W, V, dev, timed=True), ops.window_views_state(1, 64, S, W, V, dev)
    views_dev = to(views)
    Rv, tv = views[:, :12].reshape(V, 3, 4)[:, :, :3], views[:, :12].reshape(V, 3, 4)[:, :, 3]
    for k in range(W):
        Rb, tb = _path(k, W)
        X_W = np.einsum("btij,sj->btsi", R, model) + (t + k * DT * nu)[:, :, None, :]
        q = np.einsum("vij,btsj->btsvi", Rv, (X_W - tb) @ Rb) + tv
        obs = to(q[..., :2] / q[..., 2:3] + rng.normal(scale=0.1, size=q[..., :2].shape) / views[:, 12:14])
        T_WB = to(np.concatenate([Rb, tb[:, None]], axis=1).reshape(1, 12))
        last = dict(obs=obs, T_WB=T_WB)
        pushed = ops.window_push_views(state, obs, fixed["assignment"], fixed["status"], track, T_WB, views_dev, cfg)
        ops.window_push_views(twin, obs, fixed["assignment"], fixed["status"], track, T_WB, views_dev, plain)
    return dict(state=state, twin=twin, track=track, cfg=cfg, plain=plain, views=views_dev, model=to(model), pushed=pushed, **fixed, **last)


def launch_time(dev):
    from object_keypoints_amd import ops
    med = lambda us: float(np.median(us))
    rows = []
    for W in (16, 64):
        w = camera_tick(W, dev)
        st = w["state"]
        start = {"pose": w["pushed"]["start"], "velocity": w["pushed"]["start_velocity"], "assignment": st["win_assignment"]}
        moving, us_m = replay_time(lambda: ops.refine_motion_views(st["win_obs"], st["win_views"], st["win_age"], start, st["win_n"], w["model"], w["cfg"], DT))
        static, us_s = replay_time(lambda: ops.refine_pose_views_each(st["win_obs"], st["win_views"], start, st["win_n"], w["model"], w["plain"]))
        # the pushes last: every replay writes the last tick once more, so the ring is no longer the scene above
        _, us_t = replay_time(lambda: ops.window_push(st, w["tab"], w["assignment"], w["status"], w["track"], w["T_WC"], w["cam"], w["cfg"]))
        _, us_p = replay_time(lambda: ops.window_push(w["twin"], w["tab"], w["assignment"], w["status"], w["track"], w["T_WC"], w["cam"], w["plain"]))
        rows.append({"streams": STREAMS, "track_slots": SLOTS, "model_rows": 5, "ticks": W, "iters": w["cfg"].iters, "bearings_per_track": int(moving["n_obs"][0, 0]),
                     "motion_accepted": int((moving["status"] == 0).sum()), "static_accepted": int((static["status"] == 0).sum()), "of": STREAMS * SLOTS,
                     "refine_motion_median_us": med(us_m), "refine_motion_min_us": float(np.min(us_m)), "refine_motion_max_us": float(np.max(us_m)),
                     "refine_each_median_us": med(us_s), "refine_each_min_us": float(np.min(us_s)), "refine_each_max_us": float(np.max(us_s)),
                     "motion_over_each": med(us_m) / med(us_s), "window_push_timed_median_us": med(us_t), "window_push_median_us": med(us_p),
                     "note": "graph replay of one launch, back to back: launch gaps included; the same win_obs and win_views for both refinements, every one of the 1024 "
                             "rings full; the static refinement of these MOVING objects is timed, not believed"})
    w = rig_tick(4, 8, dev)
    st = w["state"]
    start = {"pose": w["pushed"]["start"], "velocity": w["pushed"]["start_velocity"], "assignment": st["win_assignment"]}
    moving, us_m = replay_time(lambda: ops.refine_motion_views(st["win_obs"], st["win_views"], st["win_age"], start, st["win_n"], w["model"], w["cfg"], DT))
    static, us_s = replay_time(lambda: ops.refine_pose_views_each(st["win_obs"], st["win_views"], start, st["win_n"], w["model"], w["plain"]))
    _, us_t = replay_time(lambda: ops.window_push_views(st, w["obs"], w["assignment"], w["status"], w["track"], w["T_WB"], w["views"], w["cfg"]))       # (the pushes last, as above)
    _, us_p = replay_time(lambda: ops.window_push_views(w["twin"], w["obs"], w["assignment"], w["status"], w["track"], w["T_WB"], w["views"], w["plain"]))
    rows.append({"pairs": 4, "ticks": 8, "views": 64, "track_slots": 64, "model_rows": 5, "iters": w["cfg"].iters, "bearings_per_track": int(moving["n_obs"][0, 0]),
                 "motion_accepted": int((moving["status"] == 0).sum()), "of": 64, "refine_motion_median_us": med(us_m), "refine_each_median_us": med(us_s),
                 "motion_over_each": med(us_m) / med(us_s), "window_push_views_timed_median_us": med(us_t), "window_push_views_median_us": med(us_p)})
    return rows


def captured_step(dev, window):
    """The captured batch-64 cups step (fp16 network, forward_device with the object model, the tracker and the world frame); window: None, or a WindowConfig."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pose = ops.frame_poses(np.tile(np.eye(4), (64, 1, 1))).to(dev)
    kw = {"window": window} if window is not None else {}
    pipe = pp.BatchedKeypointPipeline(network(4, dev), {"keypoint_config": [1, 1, 1]}, map_camera(), points_3d=CUPS_POINTS, track=ops.TrackConfig(gate=0.1, dt=DT, max_tracks=16),
                                      world_frame=True, **kw)
    return pipe, pipe.capture(frames, pose)


def captured_tick(dev, rig_window):
    """The captured 4-pair fused tick of scripts/probe_rig_window.py with a rig_window of 8 ticks."""
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
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, track=ops.TrackConfig(gate=0.1, dt=DT, max_tracks=16), world_frame=True,
                                   rig_window=rig_window)
    return pipe, pipe.capture_device(frames, heat_override=heat, rig_pose=pose)


def one_arm(arm, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured step WITHOUT a window, n replays in rounds of per_round -> one JSON line.  The parent commit's
    library does not export the new entry points, so the parent arm takes them off the signature table before the library is loaded."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_step(dev, None)
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
    """One fresh process per turn: parent, this, this, parent; the first failure ends the series."""
    from object_keypoints_amd import _lib
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    runs, rounds = {"parent": [], "this": []}, {"parent": [], "this": []}
    order = ("parent", "this", "this", "parent")
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
            "what": "the captured batch-64 cups step with the model, the tracker and the world frame, no window", "parent_median_ms": runs["parent"],
            "this_median_ms": runs["this"], "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_medians_ms": [round(v, 4) for v in rounds["parent"]], "this_round_medians_ms": [round(v, 4) for v in rounds["this"]],
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"], "inside_parent_round_spread": bool(abs(diff) <= spread["parent"]),
            "verdict": "not resolved" if abs(diff) <= spread["parent"] else "resolved"}


def main():
    from object_keypoints_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the step without a window against it, one process per turn")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "refine_motion", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_step(dev, ops.WindowConfig(16))[1], "on": captured_step(dev, ops.WindowConfig(16, motion=MOTION))[1]}
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1], ticks=16,
                           what="captured forward_device with the object model, the tracker, the world frame and a window of 16 ticks, motion off / on: replay + "
                                "synchronise, host wall time, ms")
        del arms
        arms = {"off": captured_tick(dev, ops.WindowConfig(8))[1], "on": captured_tick(dev, ops.WindowConfig(8, motion=MOTION))[1]}
        res["tick"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), pairs=4, ticks=8, dtype="float16", keypoint_config=[1, 3],
                           what="captured 4-pair fused tick with the object model, the tracker, the world frame and a rig_window of 8 ticks, motion off / on: replay + "
                                "synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
