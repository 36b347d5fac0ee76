"""What resolving interchangeable key points (okp_refine_assignments, csrc/okp_refine_assign.hip) costs.  (1) The launch alone at B = 64,
max_obj = 16, every one of the 1024 objects live, 6 iterations - replayed as a hipGraph, device time by events around batches of replays -
for a valve [1, 3] (6 hypotheses: 2 rounds) and a [1, 4] model (24 hypotheses: 6 rounds), next to okp_refine_pose on the same tables in the
same process: the expectation is roughly rounds x that launch.  (2) The captured batch-64 valve step (fp16 network, forward_device with the
object model and `refine`) with the flag on and off: both graphs live in ONE process and alternate in rounds in A B B A order; a step =
replay + synchronise, host wall time.  (3) With --parent-lib (the parent commit's build of libokp_hip.so) the captured step with the flag
OFF against that library, selected through OKP_LIB: one fresh process per arm in A B B A order, both through the ctypes binding - what the
move of the shared arithmetic into a header and the new entry point did to the step a user who does not ask for it runs.
Prints one JSON line.

    python scripts/probe_refine_assignments.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/refine_assignments.json]
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

NEW_ENTRY_POINTS = ("okp_refine_assignments",)
ONE_FOUR_POINTS = VALVE_POINTS + [[0.06, -0.05, 0.07]]


def table(type_count, points_3d, dev, seed=3, depth_noise=0.03):
    """B = 64, max_obj = 16, every object live: the model under random poses at 0.5 .. 1.5 m, exact bearings, depths off by 3 % -> the pose
    stage's outputs on it (tab, the object_pose dict, n_obj, the model on the device)."""
    from object_keypoints_amd import ops
    rng = np.random.default_rng(seed)
    model = ops.object_model(points_3d, type_count).numpy()
    S = model.shape[0]
    tab = np.empty((64, 16, S, 4))
    for b in range(64):
        for o in range(16):
            w = rng.normal(size=3)
            a = np.linalg.norm(w)
            Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / a
            R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
            q = model @ R.T + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.5, 1.5)])
            z = q[:, 2] * (1.0 + rng.normal(scale=depth_noise, size=S))
            tab[b, o] = np.stack([q[:, 0] / q[:, 2] * z, q[:, 1] / q[:, 2] * z, z, np.full(S, 0.9)], axis=1)
    tab = torch.from_numpy(tab).to(dev)
    n_obj = torch.full((64,), 16, dtype=torch.int32, device=dev)
    model = torch.from_numpy(model).to(dev)
    return tab, ops.object_pose(tab, n_obj, model, type_count), n_obj, model


def launch_time(dev, iters=6):
    from object_keypoints_amd import ops
    cam = map_camera().okp()
    rows = []
    for type_count, points in (([1, 3], VALVE_POINTS), ([1, 4], ONE_FOUR_POINTS)):
        tab, pose, n_obj, model = table(type_count, points, dev)
        plain, resolve = ops.RefineConfig(iters=iters), ops.RefineConfig(iters=iters, resolve_assignment=True)
        res_p, us_p = replay_time(lambda: ops.refine_pose(tab, pose, n_obj, model, cam, plain))
        res_a, us_a = replay_time(lambda: ops.refine_assignments(tab, pose, n_obj, model, type_count, cam, resolve))
        hyps = ops.check_refine_hypotheses(type_count)
        changed = (res_a["assignment"] != pose["assignment"]).any(dim=2)
        rows.append({"type_count": type_count, "hypotheses": hyps, "rounds": (hyps + 3) // 4, "batch": 64, "max_objects": 16, "iters": iters, "objects": 1024,
                     "resolved": int((res_a["status"] == 0).sum()), "assignment_changed": int(changed.sum()), "refine_pose_accepted": int((res_p["status"] == 0).sum()),
                     "refine_assignments_median_us": float(np.median(us_a)), "refine_assignments_min_us": float(np.min(us_a)), "refine_assignments_max_us": float(np.max(us_a)),
                     "refine_pose_median_us": float(np.median(us_p)), "refine_pose_min_us": float(np.min(us_p)), "refine_pose_max_us": float(np.max(us_p)),
                     "ratio": float(np.median(us_a) / np.median(us_p)), "note": "graph replay of the one launch, back to back: launch gaps included"})
    return rows


def abba(arms, rounds, per_round, warmup):
    """arms: {"off": step, "on": step} of captured steps -> per-arm medians, their difference and the scatter between round medians."""
    def tick(name):
        arms[name].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(warmup):
            tick(name)
    lat, meds = {n: [] for n in arms}, {n: [] for n in arms}
    order = ["off", "on", "on", "off"]
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
    res["on_minus_off_us"] = (res["on"]["median_ms"] - res["off"]["median_ms"]) * 1e3
    res["on_over_off_percent"] = 100.0 * (res["on"]["median_ms"] / res["off"]["median_ms"] - 1.0)
    return res


def captured_step(dev, resolve):
    """The captured batch-64 valve step (fp16 network, forward_device with the object model and the refinement), the flag on or off."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    rcfg = ops.RefineConfig(resolve_assignment=True) if resolve else ops.RefineConfig()
    pipe = pp.BatchedKeypointPipeline(network(3, dev), {"keypoint_config": [1, 3]}, map_camera(), points_3d=VALVE_POINTS, refine=rcfg)
    return pipe, pipe.capture(frames)


def one_arm(arm, n, warmup):
    """Child process of --parent-lib: the captured step with the flag off, n replays -> one JSON line.  The parent commit's library does not
    export the new entry point, so the parent arm takes it off the signature table before the library is loaded (it never calls it)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_step(dev, False)
        assert sorted(step.static_out["refine"]) == ["fit", "information", "pose", "status"]
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
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "lib", "libokp_hip.so")}
    runs = {"parent": [], "this": []}
    for arm in ("parent", "this", "this", "parent"):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--per-round", str(n), "--warmup", str(warmup)]
        done = subprocess.run(cmd, env=dict(os.environ, OKP_LIB=libs[arm]), capture_output=True, text=True, timeout=240)
        if done.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)} ended with {done.returncode}:\n{done.stderr[-2000:]}")
        runs[arm].append(json.loads(done.stdout.strip().splitlines()[-1])["median_ms"])
    mean = {arm: float(np.mean(v)) for arm, v in runs.items()}
    return {"order": "parent this this parent, one process each", "replays_per_process": n, "what": "the captured batch-64 valve step with the model and refine, the flag off",
            "parent_median_ms": runs["parent"], "this_median_ms": runs["this"], "this_minus_parent_us": (mean["this"] - mean["parent"]) * 1e3,
            "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0), "process_scatter_us": 1e3 * max(abs(v[0] - v[1]) for v in runs.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the step with the flag off against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "refine_assignments", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev)
    with torch.no_grad():
        arms = {"off": captured_step(dev, False)[1], "on": captured_step(dev, True)[1]}
        status = arms["on"].static_out["refine"]["status"]
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 3],
                           objects=int(arms["on"].static_out["n_obj"].sum()), resolved=int((status == 0).sum()),
                           what="captured forward_device with the object model and refine: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
