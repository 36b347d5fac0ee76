"""configs[4] tick latency in three forms, on the rendered maps of bench.py's run_stream8 (4 stereo pairs, fp16 network, capacity 16,
max_distance 1.5; the heat maps are injected as there):
  host_graph    tick(frames, use_graph=True): network pass replayed from a hipGraph, association on the host (scipy) between three
                blocking device -> host copies, one triangulation launch
  device_eager  results(tick_device(frames)): the whole tick on the device, launched eagerly, one device -> host copy at the end
  device_graph  results(step.replay()): the whole tick (network, NMS, association, triangulation, overflow word) as ONE hipGraph
Latency = host wall time per tick up to the 3D points on the host.  Prints one JSON line (median / p99 in ms per form).

    python scripts/probe_stream_device_tick.py [--ticks 200] [--warmup 20] [--out profiles/stream_device_tick.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    params = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    left = cu.FisheyeCamera(params["K"], params["D"], params["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    right = cu.FisheyeCamera(params["Kp"], params["Dp"], params["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    stereo = cu.StereoCamera(left, right, params["T_RL"])
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().to(dev)
    pipe = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5)
    n_pairs, K, size = 4, 3, 64
    # the scene of bench.py run_stream8: per pair 1 centre, 1 point of type 1, 3 points of type 2
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    base = {0: [[0.00, 0.00, 0.55]], 1: [[0.12, -0.10, 0.60]], 2: [[-0.16, 0.12, 0.50], [0.14, 0.04, 0.65], [-0.12, -0.16, 0.70]]}
    heat = np.zeros((2 * n_pairs, K, size, size), np.float32)
    for p in range(n_pairs):
        for k, pts in base.items():
            X = np.array(pts) * np.array([1.0 - 0.05 * p, 1.0 + 0.04 * p, 1.0]) + np.array([0.01 * p, -0.01 * p, 0.03 * p])
            for side, (cam, T) in enumerate(((left, np.eye(4)), (right, params["T_RL"]))):
                for px, py in cam.project(X, T):
                    heat[2 * p + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    heat_dev = torch.from_numpy(np.clip(heat, 0.0, 1.0)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((2 * n_pairs, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    pipe.capture(frames)
    step = pipe.capture_device(frames, heat_override=heat_dev)

    forms = {
        "host_graph": lambda: pipe.tick(frames, heat_override=heat_dev, use_graph=True),
        "device_eager": lambda: pipe.results(pipe.tick_device(frames, heat_override=heat_dev)),
        "device_graph": lambda: pipe.results(step.replay()),
    }
    want = forms["host_graph"]()
    res = {"probe": "stream_device_tick", "pairs": n_pairs, "dtype": "float16", "capacity": 16, "ticks": args.ticks,
           "device": torch.cuda.get_device_name(dev)}
    for name, fn in forms.items():
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        lat = []
        for _ in range(args.ticks):
            t0 = time.perf_counter()
            out = fn()
            lat.append((time.perf_counter() - t0) * 1e3)
        for p in range(n_pairs):                          # same points as the host tick (1e-9 m)
            for k in range(K):
                assert out[p][k].shape == want[p][k].shape and (out[p][k].size == 0 or np.abs(out[p][k] - want[p][k]).max() <= 1e-9)
        lat = np.array(lat)
        res[name] = {"median_ms": round(float(np.median(lat)), 4), "p99_ms": round(float(np.percentile(lat, 99)), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
