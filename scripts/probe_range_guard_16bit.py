"""What the fp16-range guard of the float16 configuration costs (KeypointNet(range_guard=True)), in ONE process, the arms
alternated ABBA so that clock drift cancels:

  * the float16 64-frame step (deployed(), 511 x 511 frames), unguarded vs guarded (on_overflow="defer": no host read in either arm);
  * the 4-pair float16 whole-tick graph (StereoStreamPipeline.capture_device, replayed, + results()), unguarded vs guarded.

    python scripts/probe_range_guard_16bit.py [--out FILE] [--rounds R] [--steps K]

--mix-step prints one JSON line with the float32mix 64-frame step instead (one arm: the library / tree it runs on is the other variable;
an A/B of two trees alternates such processes in palindromic order).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _net(dtype, range_guard=None):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    kw = {} if range_guard is None else {"range_guard": range_guard}
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=dtype, **kw)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.on_overflow = "defer"
    return net.eval().cuda()


def _time(fn, steps):
    """ms per call of fn over `steps` calls (one pair of events around the block)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _abba(arms, rounds, steps, warmup):
    """arms: {name: fn}; two arms, ABBA rounds -> {name: [ms per block]}."""
    names = list(arms)
    for n in names:
        for _ in range(warmup):
            arms[n]()
    torch.cuda.synchronize()
    got = {n: [] for n in names}
    for _ in range(rounds):
        for n in (names[0], names[1], names[1], names[0]):
            got[n].append(_time(arms[n], steps))
    return got


def _summary(got, base, other):
    med = {n: statistics.median(v) for n, v in got.items()}
    return {"ms_median": med, "ms_blocks": got, "cost_pct": 100.0 * (med[other] / med[base] - 1.0),
            "spread_pct": {n: 100.0 * (max(v) - min(v)) / statistics.median(v) for n, v in got.items()}}


def _box():
    try:
        return torch.cuda.get_device_name(0) + f" ({torch.cuda.get_device_properties(0).gcnArchName})"
    except Exception:
        return "unknown"


def mix_step(steps, warmup):
    net = _net("float32mix")
    x = torch.randn((64, 3, 511, 511), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    with torch.no_grad():
        for _ in range(warmup):
            net.deployed(x, check_range=False)
        torch.cuda.synchronize()
        ms = [_time(lambda: net.deployed(x, check_range=False), steps) for _ in range(3)]
    return {"probe": "float32mix_step", "frames": 64, "ms_blocks": ms, "ms_median": statistics.median(ms), "box": _box()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mix-step", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.mix_step:
        res = mix_step(a.steps, a.warmup)
    else:
        from object_keypoints_amd.perception import pipeline as pp
        from object_keypoints_amd.perception.utils import camera_utils as cu
        plain, guarded = _net(torch.float16), _net(torch.float16, range_guard=True)
        x = torch.randn((64, 3, 511, 511), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        with torch.no_grad():
            step = _abba({"unguarded": lambda: plain.deployed(x), "guarded": lambda: guarded.deployed(x, check_range=False)},
                         a.rounds, a.steps, a.warmup)
        assert not guarded.range_overflow()
        p = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
        offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
        mk = lambda K, D: cu.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
        stereo = cu.StereoCamera(mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"]), p["T_RL"])
        frames = torch.randn((8, 3, 511, 511), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
        ticks = {}
        with torch.no_grad():
            for name, net in (("unguarded", plain), ("guarded", guarded)):
                pipe = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=256, max_distance=1.5)
                g = pipe.capture_device(frames)
                ticks[name] = (pipe, g)

            def tick(name):
                pipe, g = ticks[name]
                g.replay()
                pipe.results(g.static_out)
            graph = _abba({"unguarded": lambda: tick("unguarded"), "guarded": lambda: tick("guarded")}, a.rounds, a.steps, a.warmup)
        res = {"probe": "range_guard_16bit", "box": _box(), "order": "ABBA x %d, %d calls per block" % (a.rounds, a.steps),
               "float16_step_64_frames": _summary(step, "unguarded", "guarded"),
               "float16_tick_graph_4_pairs": _summary(graph, "unguarded", "guarded")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
