"""What the colour correction of raw camera frames (okp_preprocess_raw8_color) costs next to the uncorrected launch (okp_preprocess_raw8):
  (a) kernel        in one process, on 64 frames of 1280 x 720 to 511 (bf16 output), an rggb mosaic and mono8: the corrected launch next
                    to the uncorrected one on the same frames, alternated; HIP events around each launch (`single`, the method of
                    probe_preprocess_bayer.py) and around four launches back to back (`queued`, which hides the host's share), medians per
                    round of --reps launches, so that each difference stands next to the scatter of its arms' own round medians
  (b) host_fed      the batch-64 bf16 step (network pass + peaks) with its frames starting in pinned host memory (HostFrameFeed):
                    corrected Bayer against uncorrected Bayer, rounds alternated
  (c) builds        the UNCORRECTED launch of this build against another build's library (the parent commit's, --parent-lib), one fresh
                    process per turn in the order parent, this, this, parent, both through OKP_LIB and the ctypes binding: shows whether
                    the untouched kernel instances moved
The separate elementwise pass the fusion competes with is estimated, not run: 64 x 1280 x 720 bytes read and written at the 5.4 TB/s the
stem kernel reaches (docs/HARDWARE_NOTES.md).  Prints one JSON line.

    python scripts/probe_preprocess_color.py [--reps 60] [--steps 12] [--rounds 3] [--parent-lib PATH] [--out profiles/preprocess_color.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, H, W, SIZE = 64, 720, 1280, 511
PASS_US = 2 * N * H * W / 5.4e12 * 1e6          # the separate pass: every source byte read and written once at the stem kernel's HBM rate


def _correction():
    from object_keypoints_amd import ops
    return ops.ColorCorrection(black_level=16, gains=(1.9, 1.0, 1.6), matrix=((1.6, -0.4, -0.2), (-0.3, 1.5, -0.2), (0.0, -0.6, 1.6)), gamma="srgb")


def _formats():
    from object_keypoints_amd import ops
    c = _correction()
    return {"bayer": ops.BayerFormat("rggb"), "bayer_color": ops.BayerFormat("rggb", c), "mono": ops.Mono8Format(), "mono_color": ops.Mono8Format(c)}


SMOOTH = False


def _frames(seed):
    """Random bytes - for the curve's byte reads from LDS the worst case: 64 lanes, 64 unrelated indices - or, with --smooth, a gradient
    with +-2 counts of noise, where neighbouring lanes read neighbouring bytes as they do in a camera's picture."""
    import torch
    g = torch.Generator().manual_seed(seed)
    if not SMOOTH:
        return torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8).pin_memory()
    ramp = (torch.arange(H)[:, None] * 120 // H + torch.arange(W)[None, :] * 120 // W + 8).to(torch.int16)
    noise = torch.randint(-2, 3, (N, H, W), generator=g, dtype=torch.int16)
    return (ramp[None] + noise).clamp_(0, 255).to(torch.uint8).pin_memory()


def _timed(f, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def _launch_times(run, reps, rounds):
    """{arm: {"single" / "queued": {"median", "round_medians"}}} of the arms of `run`, alternated launch by launch."""
    import torch
    for _ in range(5):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    out = {k: {} for k in run}
    for mode, inner in (("single", 1), ("queued", 4)):
        times = {k: [] for k in run}
        for _ in range(reps * rounds):
            for k, f in run.items():
                times[k].append(_timed(f, inner))
        for k, t in times.items():
            t = np.array(t).reshape(rounds, reps)
            out[k][mode] = {"median": round(float(np.median(t)), 2), "round_medians": [round(float(np.median(r)), 2) for r in t]}
    return out


def _difference(res, a, b, mode):
    """b - a in us, next to the spread (max - min) of each arm's own round medians."""
    ra, rb = res[a][mode], res[b][mode]
    spread = lambda r: round(max(r["round_medians"]) - min(r["round_medians"]), 2)
    return {"us": round(rb["median"] - ra["median"], 2), "ratio": round(rb["median"] / ra["median"], 3), "spread_" + a: spread(ra), "spread_" + b: spread(rb)}


def kernel_times(dev, reps, rounds):
    import torch
    from object_keypoints_amd import ops
    fmts = _formats()
    frames = _frames(1).to(dev)
    run = {k: (lambda fmt=fmt: ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=SIZE)) for k, fmt in fmts.items()}
    res = _launch_times(run, reps, rounds)
    out = {"frames": N, "frame": f"{W}x{H}", "out": "bf16 [64, 517, 520, 4]", "reps": reps, "rounds": rounds, "us": res,
           "separate_pass_estimate_us": round(PASS_US, 1)}
    for mode in ("single", "queued"):
        out["bayer_color_minus_bayer_" + mode] = _difference(res, "bayer", "bayer_color", mode)
        out["mono_color_minus_mono_" + mode] = _difference(res, "mono", "mono_color", mode)
    return out


def host_fed(dev, steps, rounds):
    import torch
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.pipeline import HostFrameFeed
    from probe_preprocess_yuv import _net
    fmts = {k: v for k, v in _formats().items() if k.startswith("bayer")}
    net = _net(torch.bfloat16, dev, None)
    host = _frames(2)
    feed = HostFrameFeed(host.shape, host.dtype, device=dev)
    with torch.no_grad():
        def step(k, frames):
            net.frame_format = fmts[k]
            return ops.peak_nms(net.deployed(frames, check_range=False)[0], cap=256)[0]

        want = {k: step(k, host.to(dev)) for k in fmts}

        def run(k, count):
            slot = feed.submit(host)
            for i in range(count):
                frames = feed.acquire(slot)
                nxt = feed.submit(host) if i + 1 < count else None
                peaks = step(k, frames)
                feed.release(slot)
                slot = nxt
            return peaks

        fps = {k: [] for k in fmts}
        for k in fmts:
            run(k, 2)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k in fmts:                              # alternated rounds of `steps` steps
                t0 = time.perf_counter()
                peaks = run(k, steps)
                torch.cuda.synchronize()
                fps[k].append(N * steps / (time.perf_counter() - t0))
                assert torch.equal(peaks, want[k])      # host-fed = resident
    out = {"batch": N, "dtype": "bf16", "steps": steps, "rounds": rounds, "step": "network pass + peak-NMS"}
    for k, v in fps.items():
        out[k + "_frames_per_s"] = {"median": round(float(np.median(v)), 1), "rounds": [round(x, 1) for x in v]}
    out["bayer_color_over_bayer"] = round(out["bayer_color_frames_per_s"]["median"] / out["bayer_frames_per_s"]["median"], 4)
    return out


def plain_times(dev, reps, rounds):
    """The uncorrected launch alone (a child process of `builds`, its library named by OKP_LIB)."""
    import torch
    from object_keypoints_amd import _lib, ops
    # a library from before the correction lacks its entry point: this process never calls it, so its signature is not bound
    _lib.SIGNATURES[:] = [s for s in _lib.SIGNATURES if s[0] != "okp_preprocess_raw8_color"]
    fmts = {k: v for k, v in _formats().items() if not k.endswith("_color")}
    frames = _frames(1).to(dev)
    run = {k: (lambda fmt=fmt: ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=SIZE)) for k, fmt in fmts.items()}
    return {"us": _launch_times(run, reps, rounds)}


def builds(parent_lib, reps, rounds):
    from object_keypoints_amd import build
    turns = []
    for name, path in (("parent", parent_lib), ("this", build.LIB_PATH), ("this", build.LIB_PATH), ("parent", parent_lib)):
        env = dict(os.environ, OKP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "plain", "--reps", str(reps), "--rounds", str(rounds)], env=env,
                           capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            raise RuntimeError(f"the {name} turn ended with status {r.returncode}:\n{r.stdout}\n{r.stderr}")      # nothing more is started
        turns.append({"build": name, **json.loads(r.stdout.strip().splitlines()[-1])["plain"]})
    out = {"order": [t["build"] for t in turns], "turns": turns}
    for k in ("bayer", "mono"):
        for mode in ("single", "queued"):
            med = {b: [t["us"][k][mode]["median"] for t in turns if t["build"] == b] for b in ("parent", "this")}
            out[f"{k}_{mode}"] = {"parent": med["parent"], "this": med["this"],
                                  "this_minus_parent_us": round(float(np.mean(med["this"]) - np.mean(med["parent"])), 2),
                                  "spread_parent": round(max(med["parent"]) - min(med["parent"]), 2),
                                  "spread_this": round(max(med["this"]) - min(med["this"]), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="kernel,host_fed,builds")
    ap.add_argument("--parent-lib", default=None, help="libokp_hip.so of the parent commit (part `builds` is skipped without it)")
    ap.add_argument("--smooth", action="store_true", help="smooth frames instead of random bytes (see _frames)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    global SMOOTH
    SMOOTH = args.smooth
    parts = args.only.split(",")
    res = {"probe": "preprocess_color", "frames": "smooth" if SMOOTH else "random bytes"}
    if "builds" in parts and args.parent_lib:           # first, before this process opens the device: its turns are processes of their own
        res["builds"] = builds(args.parent_lib, args.reps, args.rounds)
        print(json.dumps(res["builds"]), flush=True)
    if {"kernel", "host_fed", "plain"} & set(parts):
        import torch
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        res["device"] = torch.cuda.get_device_name(dev)
        if "plain" in parts:
            res["plain"] = plain_times(dev, args.reps, args.rounds)
        if "kernel" in parts:
            res["kernel"] = kernel_times(dev, args.reps, args.rounds)
            print(json.dumps(res["kernel"]), flush=True)
        if "host_fed" in parts:
            res["host_fed"] = host_fed(dev, args.steps, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
