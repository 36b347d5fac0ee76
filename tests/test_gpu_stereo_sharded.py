"""configs[4] across GPUs: the rig's stereo pairs sharded over the ranks (both views of a pair on one rank), every rank runs the device
tick on its pairs and ONE all_gather_keypoints collects the [P, K, cap, 4] payload; the overflow word is folded over the ranks on the
device.  Two spawned ranks on the one GPU with gloo carrying the collectives (as in test_gpu_two_process.py): the gathered payload must
equal what one process's tick_device computes for the whole rig, bit for bit, and results() of it must equal tick()."""
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


def _pipe(dev):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.models import KeypointNet
    from object_keypoints_amd.perception.utils import camera_utils as cu
    p = cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml"))
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    mk = lambda K, D: cu.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    stereo = cu.StereoCamera(mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"]), p["T_RL"])
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    net.eval().to(dev)
    return pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=CAP, max_distance=1.5), stereo, p


def _rig(stereo, p, start, count, dev, crowd_pair=None):
    """Frames [2 count, 3, 511, 511] and rendered heat maps [2 count, 3, 64, 64] of pairs start .. start + count of the rig, seeded /
    placed per GLOBAL pair index; crowd_pair: that pair's right map of type 2 gets twelve extra peaks (more than CAP)."""
    size = 64
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    base = {0: [[0.00, 0.00, 0.55]], 1: [[0.12, -0.10, 0.60]], 2: [[-0.16, 0.12, 0.50], [0.14, 0.04, 0.65], [-0.12, -0.16, 0.70]]}
    heat = np.zeros((2 * count, 3, size, size), np.float32)
    frames = torch.empty((2 * count, 3, 511, 511), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    for i in range(count):
        q = start + i
        gen.manual_seed(900 + q)
        frames[2 * i:2 * i + 2] = torch.randn((2, 3, 511, 511), generator=gen, device=dev, dtype=torch.float32)
        for k, pts in base.items():
            X = np.array(pts) * np.array([1.0 - 0.05 * q, 1.0 + 0.04 * q, 1.0]) + np.array([0.01 * q, -0.01 * q, 0.03 * q])
            for side, (cam, T) in enumerate(((stereo.left_camera, np.eye(4)), (stereo.right_camera, p["T_RL"]))):
                for px, py in cam.project(X, T):
                    heat[2 * i + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
        if q == crowd_pair:
            for a in range(4):
                for b in range(3):
                    heat[2 * i + 1, 2] += np.exp(-((xs - 8 - 12 * a) ** 2 + (ys - 50 - 5 * b) ** 2) / 2.0)
    return frames, torch.from_numpy(np.clip(heat, 0, 1)).to(dev)


def _rank(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from object_keypoints_amd import distributed as d
    r, _, w = d.init(backend="gloo")                     # (the gloo group; the compute below is the HIP path on cuda:0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe, stereo, p = _pipe(dev)
    out = []
    for n_pairs in RIGS:
        start, count = d.shard(n_pairs, r, w)
        frames, heat = _rig(stereo, p, start, count, dev)
        res = pipe.tick_sharded(frames, n_pairs, heat_override=heat)
        crowded = _rig(stereo, p, start, count, dev, crowd_pair=n_pairs - 1)[1]        # the rig's last pair: on the last rank with pairs
        flag = int(pipe.tick_sharded(frames, n_pairs, heat_override=crowded)["overflow"])
        cleared = int(pipe.tick_sharded(frames, n_pairs, heat_override=heat)["overflow"])
        out.append((n_pairs, start, count, res["points"].cpu().numpy(), int(res["overflow"]), flag, cleared))
    d.barrier()
    q.put((rank, out))
    d.barrier()


def test_pair_sharded_rig_gathers_what_one_process_computes():
    ctx = mp.get_context("spawn")                        # fresh interpreters: the children initialise HIP themselves
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for pr in procs:
        pr.start()
    try:
        # meanwhile, the single-process rig in this process (three processes with the GPU open in all)
        dev = torch.device("cuda", 0)
        pipe, stereo, p = _pipe(dev)
        single = {}
        for n_pairs in RIGS:
            frames, heat = _rig(stereo, p, 0, n_pairs, dev)
            dt = pipe.tick_device(frames, heat_override=heat)
            single[n_pairs] = (dt["points"].cpu().numpy(), pipe.tick(frames, heat_override=heat))
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
        covered = []
        for rank, out in results:
            got_pairs, start, count, points, overflow, crowded, cleared = out[i]
            assert got_pairs == n_pairs
            covered += list(range(start, start + count))
            assert points.shape == (n_pairs, 3, CAP, 4) == want_points.shape
            assert np.array_equal(points, want_points, equal_nan=True)            # every rank: bit for bit, NaN slots equal
            assert overflow == 0 and crowded == 1 and cleared == 0               # the overflow of one rank's pair shows on every rank
            got = pipe.results({"points": torch.from_numpy(points), "overflow": torch.tensor(overflow, dtype=torch.int32)})
            assert len(got) == n_pairs
            for a, b in zip(got, want_tick):
                for k in b:
                    assert a[k].shape == b[k].shape and (a[k].size == 0 or np.abs(a[k] - b[k]).max() <= 1e-9)
        assert covered == list(range(n_pairs))
    # without a process group, tick_sharded is tick_device on the whole rig
    frames, heat = _rig(stereo, p, 0, 4, dev)
    assert np.array_equal(pipe.tick_sharded(frames, 4, heat_override=heat)["points"].cpu().numpy(), single[4][0], equal_nan=True)
