"""What resolving a rig's interchangeable key points (okp_refine_assignments_views, csrc/okp_refine_assign_views.hip) costs.  (1) The launch
alone on 64 objects, V = 8 (a rig of four pairs), 6 iterations - replayed as a hipGraph, device time by events around batches of replays -
for a valve [1, 3] (6 hypotheses: 2 rounds of four waves) and a [1, 4] model (24 hypotheses: 6 rounds), next to okp_refine_pose_views on the
same bearings in the same process.  (2) The captured 4-pair fused tick (fp16 network, the rig of synth.stereo_rig on synth.rig_fuse_scene,
with the object model and `refine`) with resolve_views on and off: both graphs live in ONE process and alternate in rounds in A B B A order;
a tick = replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of libokp_hip.so) the captured tick with
`refine` and WITHOUT the keyword against that library, selected through OKP_LIB: one fresh process per turn, both through the ctypes binding
- what the new entry point did to the tick a user who does not ask for it runs.  No bar is fixed in advance: a difference inside the arms'
own scatter is reported as not resolved.  Prints one JSON line.

    python scripts/probe_refine_assign_views.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_assign_views.json]
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
from probe_refine_assignments import ONE_FOUR_POINTS, abba               # noqa: E402
from probe_refine_views import _rotation                                 # noqa: E402

NEW_ENTRY_POINTS = ("okp_refine_assignments_views",)
OBJECTS, PAIRS = 64, 4


def rig_table(type_count, points_3d, dev, seed=5, noise_m=0.01):
    """64 objects at 0.8 .. 1.2 m in front of a rig of four pairs of the map camera (0.1 m baselines, yawed -30 .. +30 degrees): every key point
    along its exact bearing in all eight cameras, the table's points the true ones plus a centimetre of noise, the order within a type
    shuffled -> obs, views, tab, the pose stage's outputs on the table, n_obj and the model on the device."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rng = np.random.default_rng(seed)
    cam = map_camera()
    T_RL = np.eye(4)
    T_RL[0, 3] = -0.1
    stereo = cu.StereoCamera(cam, cam, T_RL)
    T_BL = []
    for p in range(PAIRS):
        a = np.radians(-30.0 + 60.0 * p / (PAIRS - 1))
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]]
        T[:3, 3] = [0.2 * np.sin(a), 0.0, 0.0]
        T_BL.append(T)
    views = ops.rig_views(stereo, T_BL)
    v = views.numpy()
    model = ops.object_model(points_3d, type_count).numpy()
    S, V = model.shape[0], 2 * PAIRS
    obs, tab = np.zeros((1, OBJECTS, S, V, 2)), np.zeros((1, OBJECTS, S, 4))
    for o in range(OBJECTS):
        R, t = _rotation(rng), np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.8, 1.2)])
        X = model @ R.T + t
        base = 1
        for c in type_count:
            X[base:base + c] = X[base + rng.permutation(c)]
            base += c
        for cam_i in range(V):
            q = X @ v[cam_i, :12].reshape(3, 4)[:, :3].T + v[cam_i, :12].reshape(3, 4)[:, 3]
            obs[0, o, :, cam_i] = q[:, :2] / q[:, 2:]
        tab[0, o] = np.concatenate([X + rng.normal(scale=noise_m, size=(S, 3)), np.full((S, 1), 0.9)], axis=1)
    to = lambda x: torch.from_numpy(x).to(dev)
    n_obj = torch.full((1,), OBJECTS, dtype=torch.int32, device=dev)
    tab, model = to(tab), to(model)
    return dict(obs=to(obs), views=views.to(dev), tab=tab, pose=ops.object_pose(tab, n_obj, model, type_count), n_obj=n_obj, model=model)


def launch_time(dev, iters=6):
    from object_keypoints_amd import ops
    cfg = ops.RefineConfig(iters=iters)
    rows = []
    med = lambda us: float(np.median(us))
    for type_count, points in (([1, 3], VALVE_POINTS), ([1, 4], ONE_FOUR_POINTS)):
        t = rig_table(type_count, points, dev)
        res_p, us_p = replay_time(lambda: ops.refine_pose_views(t["obs"], t["views"], t["pose"], t["n_obj"], t["model"], cfg))
        res_a, us_a = replay_time(lambda: ops.refine_assignments_views(t["obs"], t["views"], t["tab"], t["pose"], t["n_obj"], t["model"], type_count, cfg))
        hyps = ops.check_refine_hypotheses(type_count)
        changed = (res_a["assignment"] != t["pose"]["assignment"]).any(dim=2)
        rows.append({"type_count": type_count, "hypotheses": hyps, "rounds": (hyps + 3) // 4, "objects": OBJECTS, "views": 2 * PAIRS, "iters": iters,
                     "bearings_per_object": int(res_a["n_obs"][0, 0]), "resolved": int((res_a["status"] == 0).sum()), "assignment_changed": int(changed.sum()),
                     "refine_pose_views_accepted": int((res_p["status"] == 0).sum()),
                     "refine_assignments_views_median_us": med(us_a), "refine_assignments_views_min_us": float(np.min(us_a)), "refine_assignments_views_max_us": float(np.max(us_a)),
                     "refine_pose_views_median_us": med(us_p), "refine_pose_views_min_us": float(np.min(us_p)), "refine_pose_views_max_us": float(np.max(us_p)),
                     "ratio": med(us_a) / med(us_p), "note": "graph replay of the one launch, back to back: launch gaps included"})
    return rows


def captured_tick(dev, resolve):
    """The captured 4-pair fused tick (fp16 network, the rig of synth.stereo_rig looking at synth.rig_fuse_scene) with the object model and refine, the keyword on or off."""
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")))
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((8, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    heat = torch.from_numpy(synth.render_rig_fuse_heat(rig, synth.rig_poses())).to(dev)
    o = synth.rig_fuse_scene()[0]
    rcfg = ops.RefineConfig(resolve_views=True) if resolve else ops.RefineConfig()
    pipe = pp.StereoStreamPipeline(network(3, dev), rig, {"keypoint_config": [1, 3]}, capacity=8, max_distance=1.5, rig_poses=synth.rig_poses(),
                                   merge_radius=synth.RIG_FUSE_MERGE_RADIUS, object_radius=synth.RIG_FUSE_OBJECT_RADIUS, fuse_capacity=16,
                                   points_3d=np.concatenate([o[1], o[2]]), max_rmse=0.1, refine=rcfg)
    return pipe, pipe.capture_device(frames, heat_override=heat)


def one_arm(arm, n, warmup, per_round=30):
    """Child process of --parent-lib: the captured tick with refine and without the keyword, n replays in rounds of per_round -> one JSON line.  The
    parent commit's library does not export the new entry point, so the parent arm takes it off the signature table before the library is
    loaded (it never calls it)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_tick(dev, False)
        assert sorted(step.static_out["refine"]) == ["fit", "information", "n_obs", "obs", "pose", "status"]
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
    """One fresh process per turn, A B B A; the first failure ends the series."""
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
            "what": "the captured 4-pair fused tick with the model and refine, without resolve_views", "parent_median_ms": runs["parent"], "this_median_ms": runs["this"],
            "this_minus_parent_us": diff, "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0),
            "parent_round_spread_us": spread["parent"], "this_round_spread_us": spread["this"], "resolved": bool(abs(diff) > max(spread.values()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the tick without the keyword against it, one process per turn")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "refine_assign_views", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_tick(dev, False)[1], "on": captured_tick(dev, True)[1]}
        r = arms["on"].static_out["refine"]
        tick = abba(arms, args.rounds, args.per_round, args.warmup)
        scatter = 1e3 * max(tick["on"]["round_spread_ms"], tick["off"]["round_spread_ms"])
        res["tick"] = dict(tick, pairs=4, dtype="float16", keypoint_config=[1, 3], objects=int(arms["on"].static_out["fused"]["n_obj"]),
                           resolved_objects=int((r["status"] == 0).sum()), difference_resolved=bool(abs(tick["on_minus_off_us"]) > scatter),
                           what="captured tick_device with rig_poses, the object model and refine: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
