"""What one eager call of each of the eight ops of the views family costs the host through ops.py, per binding, against the parent commit's tree:
the six refinements against views and the two bearing collectors at B = 1, max_obj = 2, S = 3, V = 2 with no live object (the kernel does next
to nothing: the call is checks, allocation of the outputs, marshalling and the launch), batches of 100 calls timed on the host with one
synchronise after each batch, the median batch per process.  Fresh processes alternate the two trees - parent, this, this, parent, twice -, each
with its own Python and its own two libraries; the bar is the spread of the parent arm's four process medians.

    git archive PARENT object_keypoints_amd include | tar -x -C DIR && (cd DIR && python -m object_keypoints_amd.build)
    python scripts/probe_views_family_host.py --parent-tree DIR [--out profiles/views_family_host.json]

Prints the table as JSON.  (--tree DIR is the child process: one tree, one JSON line {"<op>/<binding>": [batch means in us]}.)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
B, MAX_OBJ, S, V = 1, 2, 3, 2
PAIRS, K, CAP, CAP_F = 2, 3, 4, 3


def one(tree, batches, per_batch, warmup):
    sys.path.insert(0, tree)
    import torch
    from object_keypoints_amd import _lib, ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree)), ops.__file__
    z = lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
    i32 = torch.int32
    obs, views, each_views, prior = z((B, MAX_OBJ, S, V, 2)), z((V, 14)), z((B, MAX_OBJ, V, 14)), z((B, MAX_OBJ, S, V)) + 1.0
    pose = {"pose": z((B, MAX_OBJ, 12)), "assignment": z((B, MAX_OBJ, S), i32)}
    n_obj, model = z((B,), i32), z((S, 3))
    plain, huber, conf = ops.RefineConfig(), ops.RefineConfig(huber_px=0.5), ops.RefineConfig(confidence=ops.ConfidenceWeights(0.8, 0.4))
    table, count, xyc = z((1, ops.STEREO_PAIR_BYTES), torch.uint8), z((2 * PAIRS, K), i32), z((2 * PAIRS, K, CAP, 3), torch.float32)
    match = z((PAIRS, K, CAP), i32)
    fused = {"member": z((PAIRS, K, CAP), i32), "object": z((K, CAP_F), i32), "n_fused": z((K,), i32)}
    calls = {
        "refine_pose_views": lambda: ops.refine_pose_views(obs, views, pose, n_obj, model, plain),
        "refine_pose_views_each": lambda: ops.refine_pose_views_each(obs, each_views, pose, n_obj, model, plain),
        "refine_pose_views_robust": lambda: ops.refine_pose_views(obs, views, pose, n_obj, model, huber),
        "refine_pose_views_wide": lambda: ops.refine_pose_views_wide(obs, views, pose, n_obj, model, plain),
        "refine_pose_views_weighted": lambda: ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, conf),
        "refine_pose_views_weighted_wide": lambda: ops.refine_pose_views_weighted(obs, prior, views, pose, n_obj, model, conf, wide=True),
        "rig_bearings": lambda: ops.rig_bearings(table, count, xyc, match, fused, [2, 1]),
        "rig_bearings_weighted": lambda: ops.rig_bearings_weighted(table, count, xyc, match, fused, [2, 1], conf.confidence),
    }
    out = {}
    real = _lib.torch_ops
    assert real() is not None
    for binding in ("torch", "ctypes"):
        _lib.torch_ops = real if binding == "torch" else (lambda: None)
        for name, call in calls.items():
            for _ in range(warmup):
                call()
            torch.cuda.synchronize()
            means = []
            for _ in range(batches):
                t0 = time.perf_counter()
                for _ in range(per_batch):
                    call()
                t1 = time.perf_counter()                       # host time of the calls alone; the synchronise below only keeps the queue short
                torch.cuda.synchronize()
                means.append((t1 - t0) / per_batch * 1e6)
            out[f"{name}/{binding}"] = [round(m, 3) for m in means]
    print(json.dumps(out))


def drive(parent_tree, out_path):
    import numpy as np
    trees = {"parent": os.path.abspath(parent_tree), "this": REPO}
    order = ("parent", "this", "this", "parent", "parent", "this", "this", "parent")
    runs = {"parent": [], "this": []}
    for arm in order:
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", trees[arm]], env=env, capture_output=True, text=True, timeout=150, cwd=HERE)
        if done.returncode != 0:
            raise SystemExit(f"{arm} ended with {done.returncode}:\n{done.stderr[-3000:]}")
        runs[arm].append(json.loads(done.stdout.strip().splitlines()[-1]))
    res = {}
    for key in runs["parent"][0]:
        med = {arm: [float(np.median(r[key])) for r in runs[arm]] for arm in runs}           # one median per process
        res[key] = {"parent_us": round(float(np.mean(med["parent"])), 3), "this_us": round(float(np.mean(med["this"])), 3),
                    "diff_us": round(float(np.mean(med["this"]) - np.mean(med["parent"])), 3),
                    "parent_process_scatter_us": round(max(med["parent"]) - min(med["parent"]), 3), "parent_process_medians_us": [round(m, 3) for m in med["parent"]],
                    "this_process_medians_us": [round(m, 3) for m in med["this"]]}
        res[key]["inside_parent_scatter"] = bool(abs(res[key]["diff_us"]) <= res[key]["parent_process_scatter_us"])
    text = json.dumps({"order": " ".join(order) + ", one process each", "what": "host time of one eager ops call, us (batches of 100 calls, median batch per process)", "ops": res}, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="the parent commit's object_keypoints_amd/ and include/, built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=None, help="(child process)")
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--per-batch", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=200)
    a = ap.parse_args()
    one(a.tree, a.batches, a.per_batch, a.warmup) if a.tree else drive(a.parent_tree, a.out)
