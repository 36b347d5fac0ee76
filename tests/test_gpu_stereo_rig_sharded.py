"""configs[4] across GPUs with a calibration per stereo pair: the rig's pairs sharded over the ranks, every rank runs the device tick on its
pairs calibrated by their rig-wide index (first_pair = the shard's start), ONE all_gather_keypoints collects the [P, K, cap, 4] payload and
the overflow word is folded over the ranks.  Two spawned ranks on the one GPU with gloo carrying the collectives (as test_gpu_stereo_sharded.py
does), rigs of 4, 3 and 1 pairs of synth.stereo_rig (rank 1 has no pairs in the last): the gathered payload must equal what one process's
tick_device computes for the whole rig, bit for bit, results() of it must equal the rig's tick(), and an overflow on one rank's pair must
show on both ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

WORLD, CAP = 2, 8
RIGS = (4, 3, 1)              # pairs: blocks 2 / 2, 2 / 1 and 1 / 0 (rank 1 without pairs still joins the collectives)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(dev):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    rig = synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")), max(RIGS))
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().to(dev)
    pipes = {n: pp.StereoStreamPipeline(net, rig[:n], {"keypoint_config": [1, 3]}, capacity=CAP, max_distance=1.5) for n in RIGS}
    return pipes, rig


def _tick(rig, start, count, dev, crowd_pair=None):
    """Frames [2 count, 3, 511, 511] and heat maps [2 count, 3, 64, 64] of pairs start .. start + count of the rig (frames seeded per
    GLOBAL pair index, maps rendered through each pair's own cameras); crowd_pair: that pair's right map of type 2 gets twelve extra peaks."""
    from object_keypoints_amd import synth
    frames = torch.empty((2 * count, 3, 511, 511), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    for i in range(count):
        gen.manual_seed(700 + start + i)
        frames[2 * i:2 * i + 2] = torch.randn((2, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
    crowd = None if crowd_pair is None else (crowd_pair, 1, 2)
    heat = synth.render_rig_heat(rig, pairs=range(start, start + count), crowd=crowd)
    return frames, torch.from_numpy(heat).to(dev)


def _rank(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from object_keypoints_amd import distributed as d
    r, _, w = d.init(backend="gloo")                     # (the gloo group; the compute below is the HIP path on cuda:0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipes, rig = _setup(dev)
    out = []
    for n_pairs in RIGS:
        pipe = pipes[n_pairs]
        start, count = d.shard(n_pairs, r, w)
        frames, heat = _tick(rig, start, count, dev)
        res = pipe.tick_sharded(frames, n_pairs, heat_override=heat)
        crowded = _tick(rig, start, count, dev, crowd_pair=0)[1]          # pair 0: on rank 0
        flag = int(pipe.tick_sharded(frames, n_pairs, heat_override=crowded)["overflow"])
        cleared = int(pipe.tick_sharded(frames, n_pairs, heat_override=heat)["overflow"])
        out.append((n_pairs, start, count, res["points"].cpu().numpy(), int(res["overflow"]), flag, cleared))
    d.barrier()
    q.put((rank, out))
    d.barrier()


def test_pair_sharded_rig_of_individual_calibrations_gathers_what_one_process_computes():
    ctx = mp.get_context("spawn")                        # fresh interpreters: the children initialise HIP themselves
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for pr in procs:
        pr.start()
    try:
        # meanwhile, the single-process rig in this process (three processes with the GPU open in all)
        dev = torch.device("cuda", 0)
        pipes, rig = _setup(dev)
        single = {}
        for n_pairs in RIGS:
            frames, heat = _tick(rig, 0, n_pairs, dev)
            dt = pipes[n_pairs].tick_device(frames, heat_override=heat)
            single[n_pairs] = (dt["points"].cpu().numpy(), pipes[n_pairs].tick(frames, heat_override=heat))
        results, waited = [], 0
        while len(results) < WORLD:
            try:
                results.append(q.get(timeout=5))
            except Exception:                            # queue.Empty: a rank that died will never answer
                waited += 5
                assert all(pr.is_alive() or pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
                assert waited < 900, "ranks did not answer"
        for pr in procs:
            pr.join(timeout=120)
            assert pr.exitcode == 0
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.kill()                                # (this exact child, by handle)
    results.sort(key=lambda t: t[0])
    for i, n_pairs in enumerate(RIGS):
        want_points, want_tick = single[n_pairs]
        assert sum(len(v) for r in want_tick for v in r.values()) == 5 * n_pairs       # every rendered point of every pair matched
        covered = []
        for rank, out in results:
            got_pairs, start, count, points, overflow, crowded, cleared = out[i]
            assert got_pairs == n_pairs
            covered += list(range(start, start + count))
            assert points.shape == (n_pairs, 3, CAP, 4) == want_points.shape
            assert np.array_equal(points, want_points, equal_nan=True)            # every rank: bit for bit, NaN slots equal
            assert overflow == 0 and crowded == 1 and cleared == 0               # rank 0's overflow shows on every rank
            got = pipes[n_pairs].results({"points": torch.from_numpy(points), "overflow": torch.tensor(overflow, dtype=torch.int32)})
            assert len(got) == n_pairs
            for a, b in zip(got, want_tick):
                for k in b:
                    assert a[k].shape == b[k].shape and (a[k].size == 0 or np.abs(a[k] - b[k]).max() <= 1e-9)
        assert covered == list(range(n_pairs))
    # without a process group, tick_sharded is tick_device on the whole rig (and refuses a pair count that is not the rig's)
    frames, heat = _tick(rig, 0, 4, dev)
    assert np.array_equal(pipes[4].tick_sharded(frames, 4, heat_override=heat)["points"].cpu().numpy(), single[4][0], equal_nan=True)
    from object_keypoints_amd.ops import OkpError
    with pytest.raises(OkpError, match="the rig has 3"):
        pipes[3].tick_sharded(frames, 4, heat_override=heat)
