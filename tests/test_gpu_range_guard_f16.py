"""The fp16-range guard of the float16 configuration (KeypointNet(range_guard=True); include/okp.h okp_conv_set_range_flag on OKP_F16 plans).

float16 stores every activation in fp16: a result beyond 65504 is rounded to inf, the next layer's sums with mixed-sign weights make NaN of it
and the next ReLU turns the NaN into 0 - silently.  The range-guarded fp16 instantiations raise the same device flag as the split-product
kernels when a value they hand on in fp16 is not finite; a guarded float16 network obeys on_overflow as float32x3 does.  Unguarded passes and
healthy guarded passes are bit-identical."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
F16 = torch.float16
OKP_OK, OKP_EINVAL = 0, -1          # include/okp.h


def _state(seed=0, k=3):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    shapes = {kk: tuple(v.shape) for kk, v in KeypointNet(features=128, heatmaps_out=k).state_dict().items()}
    return {kk: torch.from_numpy(np.array(v)) for kk, v in synth.fill_state_dict(shapes, seed=seed).items()}


def _big(sd):
    big = dict(sd)
    big["backbone.pre.1.bn2.weight"] = sd["backbone.pre.1.bn2.weight"] * 3.0e5
    return big


def _net(dtype, sd, k=3, on_overflow="raise", range_guard=None):
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=k, compute_dtype=dtype, range_guard=range_guard)
    net.load_state_dict(sd)
    net.on_overflow = on_overflow
    return net.eval().cuda()


def _frames(n, seed=77):
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device="cuda", dtype=torch.float32)


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == F16 else t.contiguous().view(torch.int32)


def _module_state(m, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
        elif v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) / float(np.sqrt(v[0].numel()))
        elif k.endswith(("running_var", "weight")):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    m.load_state_dict(sd)
    return m.eval().cuda()


def _guarded(flag):
    from object_keypoints_amd import ops
    return ops.f32_split(False, False, flag, guard16=True)


def _healthy_and_poisoned(run, make_x, poison, flag, what):
    """run(x, flag or None) -> output tensor, with plans built inside the matching context.  Healthy input: the guarded launch leaves the flag 0
    and writes the bits of the unguarded one; poisoned input (operands in range, results beyond it): the flag is raised."""
    x = make_x()
    flag.zero_()
    a = run(x, None)
    g = run(x, flag)
    torch.cuda.synchronize()
    assert int(flag) == 0, what
    assert torch.equal(_bits(a), _bits(g)), what
    flag.zero_()
    run(poison(x), flag)
    torch.cuda.synchronize()
    assert int(flag) == 1, what


def test_conv_plans_gather_and_patch_kernels():
    """The gather tiles (64 x 64 / 128 x 128 / 256 x 256 on both MFMA shapes, 128 x 256), the patch-resident kernel at stride 1 and 2, and its
    transposed (unpool-merge) classes, with and without a residual."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import conv_taps, unpool_merge
    dev = torch.device("cuda")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w = (_rand((256, 256, 3, 3), 1) / np.sqrt(256 * 9)).numpy()
    b = np.zeros(256, np.float32)

    def conv(n, hw, stride, tile, res):
        ho = (hw - 1) // stride + 1

        def run(x, fl):
            with _guarded(fl):
                plan = ops.ConvPlan(F16, [256], [stride], 256, conv_taps(w), b, relu=True)
            out = ops.Act.empty(n, ho, ho, 256, F16, dev)
            r = ops.Act(torch.full((n, ho, ho, 256), 0.5, dtype=F16, device=dev)) if res else None
            plan([ops.Act(x)], out, ho, ho, res=r, tile=tile)
            return out.t.clone()
        return run

    # (an operand of 6e4 - in range - times a channel's 2 304 weights, ~N(0, 1) summed: most results are far beyond 65504)
    poison = lambda x: torch.full_like(x, 6.0e4)
    for n, hw, stride, tile, res in ((1, 16, 1, 1, False), (1, 16, 1, 8, False), (4, 32, 1, 2, True), (4, 32, 1, 3, False), (4, 32, 1, 4, True),
                                     (4, 32, 1, 6, False), (16, 32, 1, 13, False), (16, 32, 1, 13, True), (16, 64, 2, 13, False), (16, 32, 1, 14, False)):
        _healthy_and_poisoned(conv(n, hw, stride, tile, res), lambda: _rand((n, hw, hw, 256), 2).to(dev, F16), poison, flag,
                              f"conv n={n} {hw}x{hw} stride {stride} tile {tile} res {res}")
    # the transposed convolution's four sub-pixel classes (unpool + merge add): patch-resident at 64 frames of 16 x 16, gather tiles at 4
    um = unpool_merge(256).eval().cuda()
    with torch.no_grad():
        um.weight.mul_(4.0)              # (default init: a class's 1 024 weights sum to ~0.3; x4 puts 6e4 x that beyond the range)
    for n in (64, 4):
        up1 = _rand((n, 32, 32, 256), 4).to(dev, F16)

        def run(x, fl, n=n, up1=up1):
            um._drop_plans()
            with _guarded(fl):
                return um(ops.Act(x), ops.Act(up1)).t.clone()
        _healthy_and_poisoned(run, lambda n=n: _rand((n, 16, 16, 256), 3).to(dev, F16), poison, flag, f"unpool_merge n={n}")


def test_fire_modules_and_chains():
    """Every okp_fire2 instance (stride 1 and 2), and the fire chain in its three forms: 384-wide, 512-wide and entry / exit (EE)."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import fire_module, run_fire_modules
    dev = torch.device("cuda")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    big = lambda x: ((torch.rand(x.shape, generator=torch.Generator().manual_seed(6)) * 2 - 1) * 6.0e4).to(dev, F16)
    seed = 10
    for stride, configs in sorted(ops._FIRE2_CONFIGS.items()):
        for cin, mid in sorted(configs):
            seed += 1
            fm = _module_state(fire_module(cin, 2 * mid, stride=stride), seed)
            hw = 16 * stride
            assert ops.fire_fusable(cin, mid, stride, hw, hw)

            def run(x, fl, fm=fm):
                fm._drop_plans()
                with _guarded(fl):
                    return fm(ops.Act(x)).t.clone()
            _healthy_and_poisoned(run, lambda cin=cin, hw=hw: _rand((4, hw, hw, cin), seed).to(dev, F16), big, flag, f"fire2 {cin} -> {mid} stride {stride}")
    for dims, hw in (([(384, 384)] * 2, 8), ([(512, 512)] * 3, 4), ([(384, 512, 2), (512, 512), (512, 512), (512, 384)], 8)):
        mods = [_module_state(fire_module(d[0], d[1], stride=d[2] if len(d) > 2 else 1), 40 + i) for i, d in enumerate(dims)]

        def run(x, fl, mods=mods):
            for m in mods:
                m._drop_plans()
            launches = ops.COUNTERS["launches"]
            with _guarded(fl):
                out = run_fire_modules(mods, ops.Act(x)).t.clone()
            assert ops.COUNTERS["launches"] == launches + 1          # one resident chain launch
            return out
        _healthy_and_poisoned(run, lambda d=dims, hw=hw: _rand((4, hw, hw, d[0][0]), 7).to(dev, F16), big, flag, f"fire chain {dims} at {hw}x{hw}")


def test_stem_and_heads():
    """The stem (results beyond the range; frame values of 1e5, NaN and -inf, checked where they are read) and the fused heads."""
    from object_keypoints_amd import ops
    dev = torch.device("cuda", 0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w = (_rand((128, 3, 7, 7), 8) / np.sqrt(147)).numpy()
    b = np.zeros(128, np.float32)

    def stem(x, fl):
        with _guarded(fl):
            plan = ops.StemPlan(w, b, F16)
        ho = (x.shape[2] - 1) // 2 + 1
        out = ops.Act.empty(x.shape[0], ho, ho, 128, F16, dev)
        plan.from_nchw(x, out)
        return out.t.clone()
    make = lambda: _rand((2, 3, 127, 127), 9).to(dev)
    _healthy_and_poisoned(stem, make, lambda x: torch.full_like(x, 6.0e4) * torch.sign(torch.randn_like(x)), flag, "stem results")
    for bad in (1.0e5, float("nan"), -float("inf")):
        x = make()
        x[1, 2, 100, 100] = bad
        flag.zero_()
        stem(x, flag)
        torch.cuda.synchronize()
        assert int(flag) == 1, f"stem frame value {bad}"
    sd = _state()
    for head in ("heatmap", "depth", "center"):      # first layer of each head x 100: an operand of 6e4 takes its hidden values beyond the range
        sd[f"{head}_head.output_head2.0.bn.weight"] = sd[f"{head}_head.output_head2.0.bn.weight"] * 100.0
    net = _net(F16, sd)
    net_g = _net(F16, sd, range_guard=True)

    def heads(x, fl):
        n = net_g if fl is not None else net
        n._drop_all_plans()
        if fl is not None:
            n.range_flag(dev).zero_()
        out = n._run_heads(1, ops.Act(x), sigmoid=False)
        if fl is not None:
            fl.copy_(n._range_flag)
        return torch.cat([t.reshape(t.shape[0], -1) for t in out], 1)
    _healthy_and_poisoned(heads, lambda: _rand((2, 64, 64, 256), 11).to(dev, F16), lambda x: torch.full_like(x, 6.0e4), flag, "heads")


def test_float32mix_interior_fp16_plans_carry_the_flag():
    """fp16 plans built inside the mixed configuration's context (its fp16 residual branches and hourglass levels) get the flag: an inf
    inside an fp16 level is caught where it is made, not only at the fp32 boundary."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import conv_taps, fire_module
    dev = torch.device("cuda")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w = (_rand((256, 256, 3, 3), 1) / np.sqrt(256 * 9)).numpy()
    with ops.f32_split(True, True, flag):
        plan = ops.ConvPlan(F16, [256], [1], 256, conv_taps(w), np.zeros(256, np.float32), relu=True)
    assert plan._range_flag is flag
    out = ops.Act.empty(4, 32, 32, 256, F16, dev)
    plan([ops.Act(_rand((4, 32, 32, 256), 2).to(dev, F16))], out, 32, 32)
    torch.cuda.synchronize()
    assert int(flag) == 0
    plan([ops.Act(torch.full((4, 32, 32, 256), 6.0e4, dtype=F16, device=dev))], out, 32, 32)
    torch.cuda.synchronize()
    assert int(flag) == 1
    fm = _module_state(fire_module(256, 256), 3)
    flag.zero_()
    with ops.f32_split(True, True, flag):
        fm(ops.Act(((torch.rand((4, 32, 32, 256), generator=torch.Generator().manual_seed(6)) * 2 - 1) * 6.0e4).to(dev, F16)))
    torch.cuda.synchronize()
    assert int(flag) == 1


def test_network_with_one_large_batchnorm_gain():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import pipeline as op
    sd = _state()
    big = _big(sd)
    x = _frames(16)
    raising = _net(F16, big, range_guard=True)
    with torch.no_grad(), pytest.raises(ops.OkpError, match="fp16 range"):
        raising.deployed(x[:2])
    assert raising.range_overflow() and raising.range_guard
    exact = _net(torch.float32, big)
    with torch.no_grad():
        want = [t.clone() for t in exact.deployed(x[:2])]
    falling = _net(F16, big, on_overflow="float32", range_guard=True)
    with torch.no_grad(), pytest.warns(RuntimeWarning, match="re-run with the exact float32 kernels"):
        got = falling.deployed(x[:2])
    assert all(torch.equal(u, v) for u, v in zip(got, want)) and falling.configuration() == "float16"
    cam_o = op.eval_camera(CALIB)
    cam = cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size)
    pipe = pp.BatchedKeypointPipeline(_net(F16, big, on_overflow="defer", range_guard=True), {"keypoint_config": [1, 3]}, cam, capacity=4096, max_objects=64)
    with torch.no_grad():
        out = pipe.forward_device(x[:2])
    assert int(out["overflow"]) & ops.RANGE_OVERFLOW
    with pytest.raises(ops.OkpError):
        pipe.objects(out, 0)
    plain = _net(F16, big)                                       # unguarded: behaviour unchanged, no flag, nothing raised
    with torch.no_grad():
        plain.deployed(x[:2])
    assert plain.range_flag() is None and not plain.range_overflow()
    # healthy weights: guarded and unguarded passes are bit-identical, the flag stays 0; a pass after a flagged one is clean
    good = _net(F16, sd)
    good_g = _net(F16, sd, range_guard=True)
    healthy = {}
    for n in (2, 16):
        with torch.no_grad():
            a = [t.clone() for t in good.deployed(x[:n])]
            g = [t.clone() for t in good_g.deployed(x[:n])]
        assert not good_g.range_overflow()
        assert all(torch.equal(u, v) for u, v in zip(a, g)), n
        healthy[n] = a
    y = x[:2].clone()
    y[1, 0, 10, 10] = float("nan")
    with torch.no_grad(), pytest.raises(ops.OkpError, match="fp16 range"):
        good_g.deployed(y)
    with torch.no_grad():
        c = good_g.deployed(x[:2])
    assert not good_g.range_overflow() and all(torch.equal(u, v) for u, v in zip(c, healthy[2]))


def _stereo():
    from object_keypoints_amd.perception.utils import camera_utils as cu
    p = cu.load_calibration_params(CALIB)
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    mk = lambda K, D: cu.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    return cu.StereoCamera(mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"]), p["T_RL"]), p


def _heat(n_pairs, stereo, p):
    size = 64
    ys, xs = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    heat = np.zeros((2 * n_pairs, 3, size, size), np.float32)
    for pr in range(n_pairs):
        for k, pts in {0: [[0.0, 0.0, 0.55]], 1: [[0.12, -0.10, 0.60]], 2: [[-0.16, 0.12, 0.5], [0.14, 0.04, 0.65], [-0.12, -0.16, 0.7]]}.items():
            X = np.array(pts) + np.array([0.02 * pr, -0.015 * pr, 0.04 * pr])
            for side, (cam, T) in enumerate(((stereo.left_camera, np.eye(4)), (stereo.right_camera, p["T_RL"]))):
                for px, py in cam.project(X, T):
                    heat[2 * pr + side, k] += np.exp(-((xs - px) ** 2 + (ys - py) ** 2) / 4.0)
    return torch.from_numpy(np.clip(heat, 0, 1)).cuda()


def test_stream_tick_graph_and_host_tick():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    stereo, p = _stereo()
    sd = _state()
    pipe = pp.StereoStreamPipeline(_net(F16, sd, on_overflow="defer", range_guard=True), stereo, {"keypoint_config": [1, 3]}, capacity=8,
                                   max_distance=1.5)
    heat = _heat(4, stereo, p)
    frames = _frames(8, seed=31)
    bad = frames.clone()
    bad[3, 1, 200, 200] = float("nan")
    with torch.no_grad():
        assert int(pipe.tick_device(frames, heat_override=heat)["overflow"]) == 0
        out = pipe.tick_device(bad, heat_override=heat)
        assert int(out["overflow"]) & ops.RANGE_OVERFLOW
        with pytest.raises(ops.OkpError):
            pipe.results(out)
        step = pipe.capture_device(frames, heat_override=heat)
        step.replay(bad, heat_override=heat)
        torch.cuda.synchronize()
        assert int(step.static_out["overflow"]) & ops.RANGE_OVERFLOW        # the flag is zeroed and read inside the graph
        step.replay(frames, heat_override=heat)
        torch.cuda.synchronize()
        assert int(step.static_out["overflow"]) == 0
        pipe.results(step.static_out)
    raising = pp.StereoStreamPipeline(_net(F16, sd, on_overflow="raise", range_guard=True), stereo, {"keypoint_config": [1, 3]}, capacity=8,
                                      max_distance=1.5)
    with torch.no_grad(), pytest.raises(ops.OkpError):
        raising.tick(bad, heat_override=heat)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from object_keypoints_amd import distributed as d
    from object_keypoints_amd.perception import pipeline as pp
    r, _, w = d.init(backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stereo, p = _stereo()
    pipe = pp.StereoStreamPipeline(_net(F16, _state(), on_overflow="defer", range_guard=True), stereo, {"keypoint_config": [1, 3]}, capacity=8,
                                   max_distance=1.5)
    n_pairs = 4
    start, count = d.shard(n_pairs, r, w)
    frames = _frames(2 * count, seed=50 + r)
    heat = _heat(count, stereo, p)
    with torch.no_grad():
        clean = int(pipe.tick_sharded(frames, n_pairs, heat_override=heat)["overflow"])
        bad = frames.clone()
        if r == 1:
            bad[1, 0, 7, 7] = float("nan")                 # a poisoned pair on rank 1 only
        poisoned = int(pipe.tick_sharded(bad, n_pairs, heat_override=heat)["overflow"])
    d.barrier()
    q.put((rank, clean, poisoned))
    d.barrier()


def test_sharded_tick_folds_the_flag_over_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    results, waited = [], 0
    try:
        while len(results) < 2:
            try:
                results.append(q.get(timeout=5))
            except Exception:
                waited += 5
                assert all(pr.is_alive() or pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
                assert waited < 900, "ranks did not answer"
        for pr in procs:
            pr.join(timeout=120)
            assert pr.exitcode == 0
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.kill()
    for rank, clean, poisoned in results:
        assert clean == 0 and poisoned & 2, (rank, clean, poisoned)


def test_set_range_flag_accepts_f16_and_refuses_bf16_and_f32():
    """okp_conv_set_range_flag / okp_stem_set_range_flag through torch.ops and through ctypes: OKP_F16 (and OKP_F32X3) accepted, OKP_BF16 and
    OKP_F32 refused with OKP_EINVAL."""
    from object_keypoints_amd import _lib, ops
    dev = torch.device("cuda")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w = np.zeros((8, 64), np.float32)
    ws = (np.zeros((128, 3, 7, 7), np.float32), np.zeros(128, np.float32))
    L = _lib.lib()
    T = ops._ops()
    for dtype, ok in ((torch.float16, True), (torch.bfloat16, False), (torch.float32, False)):
        plan = ops.ConvPlan(dtype, [64], [1], 8, [(0, 0, 0, w)])
        rc = L.okp_conv_set_range_flag(plan._h, flag.data_ptr())
        assert rc == (OKP_OK if ok else OKP_EINVAL), (dtype, rc)
        if T is not None:
            if ok:
                T.conv_set_range_flag(plan._h, flag)
            else:
                with pytest.raises(RuntimeError):
                    T.conv_set_range_flag(plan._h, flag)
        if dtype != torch.float32:
            stem = ops.StemPlan(*ws, dtype=dtype)
            rc = L.okp_stem_set_range_flag(stem._h, flag.data_ptr())
            assert rc == (OKP_OK if ok else OKP_EINVAL), (dtype, rc)
            if T is not None:
                if ok:
                    T.stem_set_range_flag(stem._h, flag)
                else:
                    with pytest.raises(RuntimeError):
                        T.stem_set_range_flag(stem._h, flag)


def test_inf_made_inside_a_chain_module_is_caught():
    """Healthy input, one middle module of the chain with a large BatchNorm gain: the inf it makes is zeroed by a later module's ReLU before
    the chain's output - the flag still rises (every module's output is checked, not only the last)."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import fire_module, run_fire_modules
    dev = torch.device("cuda", 0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for dims, hw in (([(384, 384)] * 3, 8), ([(512, 512)] * 3, 4), ([(384, 512, 2), (512, 512), (512, 512), (512, 384)], 8)):
        mods = [_module_state(fire_module(d[0], d[1], stride=d[2] if len(d) > 2 else 1), 60 + i) for i, d in enumerate(dims)]
        with torch.no_grad():
            mods[1].bn2.weight.mul_(1.0e6)
        x = _rand((2, hw, hw, dims[0][0]), 8).to(dev, F16)
        for m in mods:
            m._drop_plans()
        flag.zero_()
        launches = ops.COUNTERS["launches"]
        with _guarded(flag):
            run_fire_modules(mods, ops.Act(x))
        torch.cuda.synchronize()
        assert ops.COUNTERS["launches"] == launches + 1 and int(flag) == 1, dims


def test_guarded_fire_modules_off_the_matrix_pipe_geometry_take_two_launches():
    """A guarded fire module whose output width is not a multiple of 16 (stride 1) / 8 (stride 2) runs as the squeeze plan + fused tail on the
    guarded gather tiles (okp_fire2 has no guarded vector-ALU form: it would spill), with the bits of the unguarded two-launch path; the
    one-launch entry refuses it."""
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.backbone import fire_module
    dev = torch.device("cuda", 0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    big = lambda x: ((torch.rand(x.shape, generator=torch.Generator().manual_seed(6)) * 2 - 1) * 6.0e4).to(dev, F16)
    for cin, cout, stride, hw in ((256, 256, 1, 24), (384, 384, 1, 40), (256, 384, 2, 20)):
        fm = _module_state(fire_module(cin, cout, stride=stride), 70 + hw)
        assert ops.fire_fusable(cin, cout // 2, stride, hw, hw) and not ops.fire_fusable(cin, cout // 2, stride, hw, hw, guarded=True)

        def run(x, fl, fm=fm):
            fm._drop_plans()
            keep = ops.FUSE_FIRE
            ops.FUSE_FIRE = fl is not None          # (unguarded: the same two launches, for the bit comparison)
            try:
                launches = ops.COUNTERS["launches"]
                with _guarded(fl):
                    out = fm(ops.Act(x)).t.clone()
                assert ops.COUNTERS["launches"] == launches + 2
            finally:
                ops.FUSE_FIRE = keep
            return out
        _healthy_and_poisoned(run, lambda: _rand((2, hw, hw, cin), 9).to(dev, F16), big, flag, f"fire {cin} -> {cout} stride {stride} at {hw}")
        fm._drop_plans()
        with _guarded(flag):
            sq, ex, wd, bd = fm._build(F16, dev)
        x = ops.Act(_rand((2, hw, hw, cin), 9).to(dev, F16))
        out = ops.Act.empty(2, (hw - 1) // stride + 1, (hw - 1) // stride + 1, cout, F16, dev)
        with pytest.raises((ops.OkpError, RuntimeError), match="matrix-pipe form"):
            ops.fire_fused(sq, ex, wd, bd, x, out, stride, fm.skip)


def test_stem_on_packed_frames_checks_them():
    """The stem on packed frames (ops.pack_frames: the path without the direct NCHW kernel) checks the frames in the guarded instance too."""
    from object_keypoints_amd import ops
    dev = torch.device("cuda", 0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w = (_rand((128, 3, 7, 7), 8) / np.sqrt(147)).numpy()
    b = np.zeros(128, np.float32)

    def stem(x, fl):
        with _guarded(fl):
            plan = ops.StemPlan(w, b, F16)
        ho = (x.shape[2] - 1) // 2 + 1
        out = ops.Act.empty(x.shape[0], ho, ho, 128, F16, dev)
        plan(ops.pack_frames(x, F16), out)
        return out.t.clone()
    make = lambda: _rand((2, 3, 127, 127), 9).to(dev)
    _healthy_and_poisoned(stem, make, lambda x: torch.full_like(x, 6.0e4) * torch.sign(torch.randn_like(x)), flag, "packed stem results")
    for bad in (1.0e5, float("nan"), -float("inf")):
        x = make()
        x[1, 2, 100, 100] = bad
        flag.zero_()
        stem(x, flag)
        torch.cuda.synchronize()
        assert int(flag) == 1, f"packed stem frame value {bad}"


def test_plans_follow_the_guard_across_configuration_switches():
    """Whether a float16 plan carries the flag is part of its cache key: after a round trip through float32x3 that switches the guard off
    (its resolved state does not change while split, so nothing is dropped then), the unguarded float16 pass does not reuse the guarded
    plans - the old flag is left alone - and switching it on again guards the next pass."""
    from object_keypoints_amd import ops
    sd = _big(_state())
    x = _frames(2)
    net = _net(F16, sd, range_guard=True)
    with torch.no_grad():
        with pytest.raises(ops.OkpError, match="fp16 range"):
            net.deployed(x)                               # guarded float16 plans cached, the flag allocated
        old = net._range_flag
        net.set_compute_dtype("float32x3")
        net.range_guard = None
        net.set_compute_dtype(torch.float16)              # unguarded float16 now
        old.zero_()
        net.deployed(x)
        torch.cuda.synchronize()
        assert int(old) == 0 and net.range_flag() is None
        net.set_compute_dtype("float32x3")
        net.range_guard = True
        net.set_compute_dtype(torch.float16)
        with pytest.raises(ops.OkpError, match="fp16 range"):
            net.deployed(x)
