"""What the sliding window (okp_window_push + okp_refine_pose_views_each, csrc/okp_window.hip / csrc/okp_refine_views.hip) costs.
(1) The two launches alone - replayed as a hipGraph, device time by events around batches of replays - at B = 64 streams, T = 16 track slots,
S = 4 model rows, for W = 16 and W = 64: a window state filled by W pushes of a camera that moves past static objects, every slot live and
measured; the push, the refinement of the full rings, and both one after the other.  (2) The captured batch-64 cups step (fp16 network,
forward_device with the object model, the tracker and the world frame) with `window` on and off: both graphs live in ONE process and alternate
in rounds in A B B A order; a step = replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of
libokp_hip.so) the captured step with window OFF against that library, selected through OKP_LIB: one fresh process per turn in A B B A
order, twice, both through the ctypes binding, each process timing its replays in rounds; the file states whether the difference of the arms'
means lies inside the scatter of the parent arm's own round medians.
Prints one JSON line.

    python scripts/probe_window.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/window.json]
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

from probe_object_pose import CUPS_POINTS, map_camera, network          # noqa: E402
from probe_refine import replay_time                                     # noqa: E402
from probe_refine_assignments import abba                                # noqa: E402
from probe_refine_views import _rotation                                 # noqa: E402

NEW_ENTRY_POINTS = ("okp_window_push", "okp_refine_pose_views_each")
STREAMS, SLOTS = 64, 16


def window_tick(W, dev, seed=5):
    """B = 64 streams of T = 16 static objects of the cups model, every one a live track measured in this tick, and a window state filled by W
    pushes from a camera that moves 0.32 m and yaws 0.16 rad over them (2 cm and 0.01 rad per tick at W = 16) -> what window_push and
    refine_pose_views_each take."""
    from object_keypoints_amd import ops
    rng = np.random.default_rng(seed)
    cam = map_camera().okp()
    model = ops.object_model(CUPS_POINTS, [1, 1, 1]).numpy()
    S = model.shape[0]
    R = np.stack([[_rotation(rng) for _ in range(SLOTS)] for _ in range(STREAMS)])
    t = np.concatenate([rng.uniform(-0.15, 0.15, size=(STREAMS, SLOTS, 2)), rng.uniform(0.8, 1.2, size=(STREAMS, SLOTS, 1))], axis=2)
    X_W = np.einsum("btij,sj->btsi", R, model) + t[:, :, None, :]
    track_pose = np.concatenate([np.einsum("ij,btjk->btik", _rotation(rng, 0.02), R), (t + rng.normal(scale=0.005, size=t.shape))[..., None]], axis=3).reshape(STREAMS, SLOTS, 12)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    track_i = np.zeros((STREAMS, SLOTS, 4), dtype=np.int32)                        # id = slot + 1, one hit, no miss, age 1
    track_i[..., 0], track_i[..., 1], track_i[..., 3] = np.arange(1, SLOTS + 1), 1, 1
    track = {"meas_of": to(np.tile(np.arange(SLOTS, dtype=np.int32), (STREAMS, 1))), "track_f": to(np.zeros((STREAMS, SLOTS, 16))), "track_pose": to(track_pose),
             "track_i": to(track_i)}
    fixed = dict(assignment=to(np.tile(np.arange(S, dtype=np.int32), (STREAMS, SLOTS, 1))), status=to(np.zeros((STREAMS, SLOTS), dtype=np.int32)))
    cfg = ops.WindowConfig(W)
    state = ops.window_state(STREAMS, SLOTS, S, W, dev)
    d = np.array([0.9, 0.3, 0.3]) / np.linalg.norm([0.9, 0.3, 0.3])
    for k in range(W):                                                             # the same path for every W: 0.32 m and 0.16 rad, in W steps
        a = 0.16 * k / W
        Rc, tc = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]), 0.32 * k / W * d
        X_C = (X_W - tc) @ Rc                                                      # R^T (X - t), row vectors
        tab = to(np.concatenate([X_C, np.full(X_C.shape[:3] + (1,), 0.9)], axis=3))
        T_WC = to(np.tile(np.concatenate([Rc, tc[:, None]], axis=1).reshape(12), (STREAMS, 1)))
        last = dict(tab=tab, T_WC=T_WC)
        ops.window_push(state, tab, fixed["assignment"], fixed["status"], track, T_WC, cam, cfg)
    return dict(state=state, track=track, cam=cam, cfg=cfg, model=to(model), **fixed, **last)


def launch_time(dev):
    from object_keypoints_amd import ops
    rows = []
    for W in (16, 64):
        w = window_tick(W, dev)
        st = w["state"]
        push = lambda: ops.window_push(st, w["tab"], w["assignment"], w["status"], w["track"], w["T_WC"], w["cam"], w["cfg"])
        refine = lambda start: ops.refine_pose_views_each(st["win_obs"], st["win_views"], {"pose": start, "assignment": st["win_assignment"]}, st["win_n"], w["model"], w["cfg"])
        pushed, us_p = replay_time(push)
        res, us_r = replay_time(lambda: refine(pushed["start"]))
        _, us_both = replay_time(lambda: refine(push()["start"]))
        med = lambda us: float(np.median(us))
        rows.append({"streams": STREAMS, "track_slots": SLOTS, "model_rows": 4, "ticks": W, "iters": w["cfg"].iters, "filled_columns": int(pushed["n_views"].min()),
                     "bearings_per_track": int(res["n_obs"][0, 0]), "accepted": int((res["status"] == 0).sum()), "of": STREAMS * SLOTS,
                     "window_push_median_us": med(us_p), "window_push_min_us": float(np.min(us_p)), "refine_each_median_us": med(us_r), "refine_each_min_us": float(np.min(us_r)),
                     "refine_each_max_us": float(np.max(us_r)), "both_launches_median_us": med(us_both),
                     "note": "graph replay of the launch(es), back to back: launch gaps included; every one of the 1024 slots is live, measured and has a full ring"})
    return rows


def captured_step(dev, window):
    """The captured batch-64 cups step (fp16 network, forward_device with the object model, the tracker and the world frame), window on or off."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pose = ops.frame_poses(np.tile(np.eye(4), (64, 1, 1))).to(dev)
    kw = {"window": ops.WindowConfig(16)} if window else {}
    pipe = pp.BatchedKeypointPipeline(network(4, dev), {"keypoint_config": [1, 1, 1]}, map_camera(), points_3d=CUPS_POINTS, track=ops.TrackConfig(gate=0.1, dt=1 / 30, max_tracks=16),
                                      world_frame=True, **kw)
    return pipe, pipe.capture(frames, pose)


def one_arm(arm, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured step with window off, n replays in rounds of per_round -> one JSON line.  The parent commit's
    library does not export the new entry points, so the parent arm takes them off the signature table before the library is loaded."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_step(dev, False)
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
            "what": "the captured batch-64 cups step with the model, the tracker and the world frame, window off", "parent_median_ms": runs["parent"],
            "this_median_ms": runs["this"], "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_medians_ms": [round(v, 4) for v in rounds["parent"]], "this_round_medians_ms": [round(v, 4) for v in rounds["this"]],
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"],
            "parent_process_spread_us": 1e3 * (max(runs["parent"]) - min(runs["parent"])), "inside_parent_round_spread": bool(abs(diff) <= spread["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the step with window off against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "window", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_step(dev, False)[1], "on": captured_step(dev, True)[1]}
        w = arms["on"].static_out["window"]
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1], ticks=16,
                           live_tracks=int(arms["on"].static_out["track"]["n_tracks"].sum()), refined=int((w["status"] == 0).sum()), filled=int(w["n_views"].max()),
                           what="captured forward_device with the object model, the tracker and the world frame: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
