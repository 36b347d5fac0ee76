"""What the pose refinement (okp_refine_pose, csrc/okp_refine.hip) costs.  (1) The launch alone at B = 64, max_obj = 16 - replayed as a
hipGraph, device time by events around batches of replays - on the pose stage's outputs for the batch-64 cups scene of the tests
(synth.bump_scene) and for a table with every one of the 1024 objects live.  (2) The captured batch-64 cups step (fp16 network,
forward_device with the object model) with and without `refine`: both graphs live in ONE process and alternate in rounds in A B B A order,
so that drift of the host or the GPU falls on both; a step = replay + synchronise, host wall time.  (3) With --parent-lib (the parent
commit's build of libokp_hip.so) the captured step WITHOUT refine against that library, selected through OKP_LIB: one fresh process per arm
in A B B A order, both through the ctypes binding - what adding the entry point did to the step a user who does not ask for it runs.
Prints one JSON line.

    python scripts/probe_refine.py [--rounds 12] [--per-round 30] [--warmup 20] [--parent-lib libokp_hip_parent.so] [--out profiles/object_refine.json]
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

NEW_ENTRY_POINTS = ("okp_refine_pose",)


def replay_time(fn, batches=30, per_batch=50):
    """fn captured as one hipGraph -> (its result, per-replay device time in microseconds over `batches` batches)."""
    for _ in range(3):
        res = fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fn()
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
    return res, us


def launch_time(dev, iters):
    from object_keypoints_amd import ops, synth
    from object_keypoints_amd.perception import pipeline as pp
    cfg = [1, 1, 1]
    scenes = [synth.bump_scene(cfg, n_objects=1 + (i % 4), seed=11, index=i) for i in range(64)]
    maps = [torch.from_numpy(np.stack([s[key] for s in scenes])).to(dev) for key in ("heat", "depth", "centers")]
    pipe = pp.BatchedKeypointPipeline(None, {"keypoint_config": cfg}, map_camera(), points_3d=CUPS_POINTS)
    out = pipe.postprocess_device(*maps)
    model, rcfg = pipe._model(dev), ops.RefineConfig(iters=iters)
    rows = []
    # the scene as it is, and the same table with its first object copied into all 1024 rows and every one of them live
    full = {k: out["pose"][k][:1, :1].expand(64, 16, *out["pose"][k].shape[2:]).contiguous() for k in ("tab", "pose", "assignment")}
    n_full = torch.full((64,), 16, dtype=torch.int32, device=dev)
    for name, tab, pose, n_obj in (("cups scene", out["pose"]["tab"], out["pose"], out["n_obj"]), ("every row live", full["tab"], full, n_full)):
        res, us = replay_time(lambda: ops.refine_pose(tab, pose, n_obj, model, pipe.cam, rcfg))
        status = res["status"].cpu().numpy()
        rows.append({"table": name, "batch": 64, "max_objects": 16, "S": 4, "iters": iters, "objects": int(n_obj.sum()), "accepted": int((status == 0).sum()),
                     "median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)),
                     "note": "graph replay of the one launch, back to back: launch gaps included"})
    return rows


def abba(arms, rounds, per_round, warmup):
    """arms: {"pose": step, "refine": step} of captured steps -> per-arm medians and their difference."""
    def tick(name):
        arms[name].replay()
        torch.cuda.synchronize()

    for name in arms:
        for _ in range(warmup):
            tick(name)
    lat, meds = {n: [] for n in arms}, {n: [] for n in arms}
    order = ["pose", "refine", "refine", "pose"]
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
    res["refine_minus_pose_us"] = (res["refine"]["median_ms"] - res["pose"]["median_ms"]) * 1e3
    res["refine_over_pose_percent"] = 100.0 * (res["refine"]["median_ms"] / res["pose"]["median_ms"] - 1.0)
    return res


def captured_step(dev, refine):
    """The captured batch-64 cups step (fp16 network, forward_device with the object model), with or without the refinement."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((64, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    kw = {"refine": ops.RefineConfig()} if refine else {}
    pipe = pp.BatchedKeypointPipeline(network(4, dev), {"keypoint_config": [1, 1, 1]}, map_camera(), points_3d=CUPS_POINTS, **kw)
    return pipe, pipe.capture(frames)


def one_arm(arm, n, warmup):
    """Child process of --parent-lib: the captured step without refine, n replays -> one JSON line.  The parent commit's library does not
    export the new entry point, so the parent arm takes it off the signature table before the library is loaded (it never calls it)."""
    from object_keypoints_amd import _lib
    if arm == "parent":
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if s[0] not in NEW_ENTRY_POINTS]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        _, step = captured_step(dev, False)
        assert "refine" not in step.static_out
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
    return {"order": "parent this this parent, one process each", "replays_per_process": n, "what": "the captured batch-64 cups step with the model, without refine",
            "parent_median_ms": runs["parent"], "this_median_ms": runs["this"], "this_minus_parent_us": (mean["this"] - mean["parent"]) * 1e3,
            "this_over_parent_percent": 100.0 * (mean["this"] / mean["parent"] - 1.0), "process_scatter_us": 1e3 * max(abs(v[0] - v[1]) for v in runs.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libokp_hip.so: also time the step without refine against it, one process per arm")
    ap.add_argument("--arm", choices=["parent", "this"], default=None, help="(child process of --parent-lib)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.arm:
        return one_arm(args.arm, args.per_round, args.warmup)
    res = {"probe": "object_refine", "rounds": args.rounds, "per_round": args.per_round, "order": "A B B A rounds, one process"}
    if args.parent_lib:                                  # first, while this process has not touched the GPU
        res["against_parent_library"] = against_parent_library(args.parent_lib, args.rounds * args.per_round // 2, args.warmup)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["launch"] = launch_time(dev, 6) + launch_time(dev, 16)
    with torch.no_grad():
        arms = {"pose": captured_step(dev, False)[1], "refine": captured_step(dev, True)[1]}
        status = arms["refine"].static_out["refine"]["status"]
        res["step"] = dict(abba(arms, args.rounds, args.per_round, args.warmup), batch=64, dtype="float16", keypoint_config=[1, 1, 1],
                           objects=int(arms["refine"].static_out["n_obj"].sum()), accepted=int((status == 0).sum()),
                           what="captured forward_device with the object model: replay + synchronise, host wall time, ms")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
