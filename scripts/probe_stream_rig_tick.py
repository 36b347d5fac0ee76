"""configs[4] tick latency with one calibration for every pair against a rig of four individually calibrated pairs, in ONE process: the
whole device tick (network, NMS, association, triangulation, overflow word) replayed as one hipGraph, then results() (one device -> host
copy), 4 stereo pairs, fp16 network, capacity 16, max_distance 1.5.  As bench.py's run_stream8 does, the heat maps are injected: Gaussian
bumps rendered from known 3D points (synth.rig_scene_points) through each pair's cameras - pair 0's calibration for every pair in the
`single` form, synth.stereo_rig's four pairs in the `rig` form.  The two forms alternate in rounds of --per-round ticks so that drift of
the host or the GPU falls on both.  Latency = host wall time per tick up to the 3D points on the host.  Prints one JSON line: median / p99
in ms per form and the spread of the per-round medians.

    python scripts/probe_stream_rig_tick.py [--rounds 10] [--per-round 40] [--warmup 20] [--out profiles/stream_rig_tick.json]
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_pairs = 4
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")), n_pairs)
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    frames = torch.randn((2 * n_pairs, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    forms = {}
    for name, cal, cams in (("single", rig[0], [rig[0]] * n_pairs), ("rig", rig, rig)):
        pipe = pp.StereoStreamPipeline(net, cal, {"keypoint_config": [1, 3]}, capacity=16, max_distance=1.5)
        heat = torch.from_numpy(synth.render_rig_heat(cams)).to(dev)
        step = pipe.capture_device(frames, heat_override=heat)
        want = pipe.tick(frames, heat_override=heat)
        assert sum(len(v) for r in want for v in r.values()) == 5 * n_pairs           # every rendered point matched
        forms[name] = (pipe, step, want)

    def run(name):
        pipe, step, _ = forms[name]
        return pipe.results(step.replay())

    for name in forms:
        for _ in range(args.warmup):
            run(name)
    torch.cuda.synchronize()
    lat = {name: [] for name in forms}
    rounds = {name: [] for name in forms}
    for r in range(args.rounds):
        for name in (forms if r % 2 == 0 else reversed(list(forms))):
            this = []
            for _ in range(args.per_round):
                t0 = time.perf_counter()
                out = run(name)
                this.append((time.perf_counter() - t0) * 1e3)
            lat[name] += this
            rounds[name].append(float(np.median(this)))
            want = forms[name][2]
            for p in range(n_pairs):                       # the same points as the host tick (1e-9 m)
                for k in want[p]:
                    assert out[p][k].shape == want[p][k].shape and (out[p][k].size == 0 or np.abs(out[p][k] - want[p][k]).max() <= 1e-9)
    res = {"probe": "stream_rig_tick", "pairs": n_pairs, "dtype": "float16", "capacity": 16, "rounds": args.rounds, "per_round": args.per_round,
           "device": torch.cuda.get_device_name(dev)}
    for name in forms:
        a = np.array(lat[name])
        res[name] = {"median_ms": round(float(np.median(a)), 4), "p99_ms": round(float(np.percentile(a, 99)), 4),
                     "round_median_min_ms": round(min(rounds[name]), 4), "round_median_max_ms": round(max(rounds[name]), 4)}
    res["rig_minus_single_median_ms"] = round(res["rig"]["median_ms"] - res["single"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
