"""Bayer (bayer_rggb8) and mono8 camera frames against RGB and NV12 frames as the network's raw input, in one process, the forms alternated:
  (a) kernel        the pre-processing launch alone on a batch of 64 frames of 1280 x 720 (okp_preprocess_raw8 on an rggb mosaic and on
                    mono8, next to okp_preprocess_u8 on RGB and okp_preprocess_yuv420 on NV12; bf16 output, 511 x 511 crop): HIP events
                    around each launch, median over --reps launches per form
  (b) host_fed      the batch-64 bf16 step (network pass + peaks) with its frames starting in pinned host memory, uploaded by HostFrameFeed
                    on a copy stream under the previous step: frames/s, Bayer against RGB and NV12
  (c) stream8       StereoStreamPipeline.stream() of host ticks of 8 frames (4 stereo pairs, fp16 network, capacity 16, the rendered
                    heat maps of bench.py's configs[4] scene injected): per-tick latency median / p99, Bayer against RGB
One network serves every form: its frame_format is switched between the forms' rounds.  Every host-fed result is checked against the same
frames resident.  Prints one JSON line.

    python scripts/probe_preprocess_bayer.py [--reps 60] [--steps 12] [--ticks 100] [--rounds 3] [--out profiles/preprocess_bayer.json]
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

from probe_preprocess_yuv import _net, _scene          # noqa: E402  (the same random-weight network and injected scene)


def _formats():
    from object_keypoints_amd import ops
    return {"rgb": None, "nv12": ops.YUV420Format("nv12"), "bayer": ops.BayerFormat("rggb"), "mono": ops.Mono8Format()}


def _host_frames(n, h, w, seed, forms):
    """Pinned host frames of random bytes in each form (the content does not matter to the timing, the byte counts do)."""
    g = torch.Generator().manual_seed(seed)
    shape = {"rgb": (n, h, w, 3), "nv12": (n, 3 * h // 2, w), "bayer": (n, h, w), "mono": (n, h, w)}
    return {k: torch.randint(16, 236, shape[k], generator=g, dtype=torch.uint8).pin_memory() for k in forms}


def _stats(t):
    return {"median": round(float(np.median(t)), 2), "p10": round(float(np.percentile(t, 10)), 2), "p90": round(float(np.percentile(t, 90)), 2)}


def kernel_times(dev, reps):
    from object_keypoints_amd import ops
    n, h, w = 64, 720, 1280
    fmts = _formats()
    frames = {k: v.to(dev) for k, v in _host_frames(n, h, w, 1, fmts).items()}
    run = {"rgb": lambda: ops.preprocess_u8(frames["rgb"], torch.bfloat16, size=511),
           "nv12": lambda: ops.preprocess_yuv420(frames["nv12"], torch.bfloat16, fmts["nv12"], size=511),
           "bayer": lambda: ops.preprocess_raw8(frames["bayer"], torch.bfloat16, fmts["bayer"], size=511),
           "mono": lambda: ops.preprocess_raw8(frames["mono"], torch.bfloat16, fmts["mono"], size=511)}
    times = {k: [] for k in run}
    for _ in range(5):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in run.items():                        # alternated: rgb, nv12, bayer, mono, rgb, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    out = {"frames": n, "frame": f"{w}x{h}", "out": "bf16 [64, 517, 520, 4]", "reps": reps,
           "MB_in": {k: frames[k].numel() / 1e6 for k in run}}
    for k, t in times.items():
        out[k + "_us"] = _stats(t)
    for k in ("nv12", "bayer", "mono"):
        out[k + "_over_rgb"] = round(out[k + "_us"]["median"] / out["rgb_us"]["median"], 3)
    return out


def host_fed(dev, steps, rounds=3):
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.pipeline import HostFrameFeed
    fmts = {k: v for k, v in _formats().items() if k != "mono"}
    net = _net(torch.bfloat16, dev, None)
    n = 64
    hosts = _host_frames(n, 720, 1280, 2, fmts)
    feeds = {k: HostFrameFeed(h.shape, h.dtype, device=dev) for k, h in hosts.items()}
    with torch.no_grad():
        def step(k, frames):
            net.frame_format = fmts[k]
            return ops.peak_nms(net.deployed(frames, check_range=False)[0], cap=256)[0]

        want = {k: step(k, h.to(dev)) for k, h in hosts.items()}

        def run(k, count):
            feed, host = feeds[k], hosts[k]
            slot = feed.submit(host)
            for i in range(count):
                frames = feed.acquire(slot)
                nxt = feed.submit(host) if i + 1 < count else None
                peaks = step(k, frames)
                feed.release(slot)
                slot = nxt
            return peaks

        fps = {k: [] for k in hosts}
        for k in hosts:
            run(k, 2)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k in hosts:                             # alternated rounds of `steps` steps
                t0 = time.perf_counter()
                peaks = run(k, steps)
                torch.cuda.synchronize()
                fps[k].append(n * steps / (time.perf_counter() - t0))
                assert torch.equal(peaks, want[k])      # host-fed = resident
    out = {"batch": n, "dtype": "bf16", "steps": steps, "rounds": rounds, "step": "network pass + peak-NMS",
           "MB_per_step": {k: h.numel() / 1e6 for k, h in hosts.items()}}
    for k, v in fps.items():
        out[k + "_frames_per_s"] = {"median": round(float(np.median(v)), 1), "rounds": [round(x, 1) for x in v]}
    out["bayer_over_rgb"] = round(out["bayer_frames_per_s"]["median"] / out["rgb_frames_per_s"]["median"], 3)
    out["bayer_over_nv12"] = round(out["bayer_frames_per_s"]["median"] / out["nv12_frames_per_s"]["median"], 3)
    return out


def stream8(dev, ticks, rounds=3):
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    params = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    left = cu.FisheyeCamera(params["K"], params["D"], params["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    right = cu.FisheyeCamera(params["Kp"], params["Dp"], params["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    n_pairs = 4
    fmts = {k: v for k, v in _formats().items() if k in ("rgb", "bayer")}
    net = _net(torch.float16, dev, None)
    pipe = pp.StereoStreamPipeline(net, cu.StereoCamera(left, right, params["T_RL"]), {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5)
    heat = torch.from_numpy(_scene(left, right, params["T_RL"], n_pairs)).to(dev)
    hosts = _host_frames(2 * n_pairs, 720, 1280, 3, fmts)
    want = {}
    for k, h in hosts.items():
        net.frame_format = fmts[k]
        want[k] = pipe.tick(h.to(dev), heat_override=heat)
    lat = {k: [] for k in hosts}

    def run(k, count, record):
        net.frame_format = fmts[k]
        t0 = time.perf_counter()
        for res in pipe.stream((hosts[k] for _ in range(count)), heat_override=heat):
            t1 = time.perf_counter()
            if record:
                lat[k].append((t1 - t0) * 1e3)
            t0 = t1
        for p in range(n_pairs):
            for j in range(3):
                assert np.array_equal(res[p][j], want[k][p][j])          # host-fed = resident, bit for bit

    for k in hosts:
        run(k, 10, False)
    for _ in range(rounds):
        for k in hosts:
            run(k, ticks, True)
    out = {"pairs": n_pairs, "frames_per_tick": 2 * n_pairs, "dtype": "float16", "ticks": ticks * rounds, "rounds": rounds,
           "MB_per_tick": {k: h.numel() / 1e6 for k, h in hosts.items()}, "latency": "host wall time between consecutive stream() results"}
    for k, v in lat.items():
        v = np.array(v)
        out[k + "_tick_ms"] = {"median": round(float(np.median(v)), 4), "p99": round(float(np.percentile(v, 99)), 4),
                               "round_medians": [round(float(np.median(r)), 4) for r in v.reshape(rounds, ticks)]}
    out["bayer_over_rgb_median"] = round(out["bayer_tick_ms"]["median"] / out["rgb_tick_ms"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="kernel,host_fed,stream8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"probe": "preprocess_bayer", "device": torch.cuda.get_device_name(dev)}
    parts = args.only.split(",")
    if "kernel" in parts:
        res["kernel"] = kernel_times(dev, args.reps)
        print(json.dumps(res["kernel"]), flush=True)
    if "host_fed" in parts:
        res["host_fed"] = host_fed(dev, args.steps, args.rounds)
        print(json.dumps(res["host_fed"]), flush=True)
    if "stream8" in parts:
        res["stream8"] = stream8(dev, args.ticks, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
