"""Bayer mosaics and mono8 camera frames straight into the network (okp_preprocess_raw8): the device path equals the specification
(tests/bayer_spec.py) followed by the existing, oracle-pinned resize + crop + normalisation (okp_preprocess_u8), byte for byte, for the
four patterns and mono8, mirrored borders, clamped taps, pitched buffers, saturating mosaics and both bindings; and the network and
pipelines give on raw frames exactly what they give on the demosaiced RGB frames."""
import functools
import os

import numpy as np
import pytest
import torch

import bayer_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
FORMATS = bayer_spec.PATTERNS + ("mono",)
SHAPES = [((1, 2, 2), 2),             # every neighbour is a mirror image
          ((1, 4, 6), 4),
          ((1, 8, 10), 13),           # upscaling: taps clamped at the last row and column (s1 == s0)
          ((1, 98, 62), 33),
          ((3, 40, 40), 40),          # no resize
          ((1, 34, 200), 21),
          ((2, 720, 1280), 511)]


def _fmt(name):
    from object_keypoints_amd import ops
    return ops.Mono8Format() if name == "mono" else ops.BayerFormat(name)


@functools.lru_cache(maxsize=None)
def _frames(n, h, w, seed):
    f = np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _rgb(n, h, w, seed, name):
    """The specification's RGB frames of _frames(n, h, w, seed), computed once per format."""
    rgb = bayer_spec.frames_to_rgb(_frames(n, h, w, seed), name)
    rgb.setflags(write=False)
    return rgb


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _net(compute_dtype, frame_format):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=compute_dtype, frame_format=frame_format)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().cuda()


@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("name", FORMATS)
def test_raw_path_equals_spec_then_rgb_path_bit_exact(name, shape, size):
    from object_keypoints_amd import ops
    from oracle import pipeline as op
    from oracle import preprocess as pre
    n, h, w = shape
    rgb = _rgb(n, h, w, h + w, name)
    got = ops.preprocess_raw8(_dev(_frames(n, h, w, h + w)), torch.float32, _fmt(name), size=size).t.cpu().numpy()
    want = ops.preprocess_u8(_dev(rgb), torch.float32, size=size).t.cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    # the interior is the oracle's resize + crop + normalisation of the demosaiced frames
    ref = op.normalize_frames(np.stack([pre.resize_center_crop(f, size) for f in rgb]))
    assert np.array_equal(got[:, 3:3 + size, 3:3 + size, :3].transpose(0, 3, 1, 2), ref)
    halo = got.copy()
    halo[:, 3:3 + size, 3:3 + size, :3] = 0
    assert not halo.any()                                               # zero halo and zero 4th channel


def test_mono_takes_odd_sizes_a_single_row_and_a_single_column():
    from object_keypoints_amd import ops
    for (n, h, w), size in [((2, 7, 5), 5), ((1, 1, 9), 1), ((1, 9, 1), 1), ((1, 1, 1), 1), ((1, 3, 3), 8)]:
        f = _frames(n, h, w, 7)
        got = ops.preprocess_raw8(_dev(f), torch.float32, _fmt("mono"), size=size).t
        want = ops.preprocess_u8(_dev(bayer_spec.mono_to_rgb(f)), torch.float32, size=size).t
        assert torch.equal(got, want), (n, h, w)


@pytest.mark.parametrize("size", [16, 23])           # the identity resize keeps each demosaiced sample; 23 interpolates between them
@pytest.mark.parametrize("name", FORMATS)
def test_saturating_mosaics(name, size):
    """Columns alternating 0 and 255, rows alternating, both, and all 255: every sum of the demosaic at its extremes (4 x 255 + 2), the
    rounding of the halves, and the resize on 0 / 255 neighbours."""
    from object_keypoints_amd import ops
    h = w = 16
    y, x = np.mgrid[0:h, 0:w]
    frames = np.stack([(x & 1) * 255, ((x + 1) & 1) * 255, (y & 1) * 255, ((y + 1) & 1) * 255, ((x ^ y) & 1) * 255, np.full((h, w), 255),
                       np.where((x & 1) & (y & 1), 254, 255), np.where((x & 1) | (y & 1), 1, 0)]).astype(np.uint8)
    rgb = bayer_spec.frames_to_rgb(frames, name)
    assert (rgb == 0).any() and (rgb == 255).any()
    got = ops.preprocess_raw8(_dev(frames), torch.float32, _fmt(name), size=size).t
    want = ops.preprocess_u8(_dev(rgb), torch.float32, size=size).t
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["gbrg", "mono"])
def test_raw_path_16bit_outputs_equal_the_rgb_path(name, dtype):
    from object_keypoints_amd import ops
    got = ops.preprocess_raw8(_dev(_frames(2, 720, 1280, 2000)), dtype, _fmt(name), size=511).t
    want = ops.preprocess_u8(_dev(_rgb(2, 720, 1280, 2000, name)), dtype, size=511).t
    assert got.dtype == dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("pitch,spare_rows", [(62 + 65, 0), (62 + 64, 3), (62 + 1, 1)])          # an odd and an even pitch; frames more than H * pitch apart
@pytest.mark.parametrize("name", FORMATS)
def test_pitched_view_equals_the_contiguous_frames(name, pitch, spare_rows):
    """0xAB between the width and the pitch and in the spare rows: the right edge mirrors to W-2 and the bottom edge to H-2, never into
    the padding."""
    from object_keypoints_amd import ops
    n, h, w = 3, 98, 62
    f = _frames(n, h, w, 11)
    buf = np.full((n, h + spare_rows, pitch), 0xAB, np.uint8)
    buf[:, :h, :w] = f
    view = torch.from_numpy(buf).cuda()[:, :h, :w]
    assert view.stride() == ((h + spare_rows) * pitch, pitch, 1) and not view.is_contiguous()
    assert ops.check_raw8_frames(view, _fmt(name)) == (n, h, w, pitch, (h + spare_rows) * pitch)
    got = ops.preprocess_raw8(view, torch.float32, _fmt(name), size=33).t
    want = ops.preprocess_raw8(_dev(f), torch.float32, _fmt(name), size=33).t
    assert torch.equal(got, want)
    assert torch.equal(got, ops.preprocess_u8(_dev(_rgb(n, h, w, 11, name)), torch.float32, size=33).t)
    # a view at an offset inside the buffer: upscaled, so the last row and column are tapped and their neighbours mirrored
    sub = torch.from_numpy(buf).cuda()[1:, 4:12, 6:16]
    got = ops.preprocess_raw8(sub, torch.float32, _fmt(name), size=13).t
    want = ops.preprocess_u8(_dev(bayer_spec.frames_to_rgb(buf[1:, 4:12, 6:16], name)), torch.float32, size=13).t
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["bggr", "mono"])
def test_ctypes_and_torch_ops_bindings_give_the_same_bytes(name):
    from object_keypoints_amd import _lib, ops
    buf = np.full((2, 100, 127), 0xAB, np.uint8)
    buf[:, :98, :62] = _frames(2, 98, 62, 5)
    frames = torch.from_numpy(buf).cuda()[:, :98, :62]
    fmt = _fmt(name)
    assert _lib.torch_ops() is not None
    launches = ops.COUNTERS["ctypes_launches"]
    a = ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=33).t
    assert ops.COUNTERS["ctypes_launches"] == launches
    keep = _lib._torch_ops
    try:
        _lib._torch_ops = None                        # the ctypes binding serves the launch
        b = ops.preprocess_raw8(frames, torch.bfloat16, fmt, size=33).t
    finally:
        _lib._torch_ops = keep
    assert ops.COUNTERS["ctypes_launches"] == launches + 1
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.view(torch.int16), ops.preprocess_u8(_dev(_rgb(2, 98, 62, 5, name)), torch.bfloat16, size=33).t.view(torch.int16))


@pytest.mark.parametrize("name", ["grbg", "mono"])
def test_network_on_raw_frames_equals_the_network_on_spec_rgb(name):
    net = _net(torch.bfloat16, _fmt(name))
    with torch.no_grad():
        a = net.deployed(_dev(_frames(2, 720, 1280, 2000)))
        b = net.deployed(_dev(_rgb(2, 720, 1280, 2000, name)))
    assert len(a) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert tuple(a[0].shape) == (2, 3, 64, 64)


def test_network_refusals_on_device_frames():
    from object_keypoints_amd import ops
    net = _net(torch.bfloat16, None)
    frames = torch.zeros((1, 96, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(ops.OkpError, match=r"4:2:0 \(YUV\) frames \[N, 3H/2, W\]: set frame_format"):
        net.deployed(frames)
    net.frame_format = _fmt("rggb")
    with pytest.raises(ops.OkpError, match="inner stride"):
        net.deployed(torch.zeros((1, 64, 96), dtype=torch.uint8, device="cuda").transpose(1, 2))
    with pytest.raises(ops.OkpError, match="must be even"):
        net.deployed(torch.zeros((1, 95, 64), dtype=torch.uint8, device="cuda"))
    net.raw_frame_size = None
    with pytest.raises(ops.OkpError, match="raw_frame_size"):
        net.deployed(frames)


def _stereo():
    from object_keypoints_amd.perception.utils import camera_utils as cu
    p = cu.load_calibration_params(CALIB)
    offset = np.array([(511 / 720 * 1280 - 511.0) / 2.0, 0.0])
    mk = lambda K, D: cu.FisheyeCamera(K, D, p["image_size"]).scale(511 / 720).cut(offset).scale(64 / 511)
    return cu.StereoCamera(mk(p["K"], p["D"]), mk(p["Kp"], p["Dp"]), p["T_RL"])


def _same(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert sorted(pa) == sorted(pb)
        for k in pa:
            assert pa[k].shape == pb[k].shape and np.array_equal(pa[k], pb[k])


def _bits_equal(x, y, keys):
    for key in keys:
        a, b = x[key], y[key]
        if a.is_floating_point():
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)), key
        else:
            assert torch.equal(a, b), key


def test_batched_pipeline_step_eager_and_captured_equals_the_rgb_run():
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import pipeline as op
    name = "rggb"
    net = _net(torch.bfloat16, _fmt(name))
    cam_o = op.eval_camera(CALIB)
    batched = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 3]}, cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size), capacity=256)
    raw = [_dev(_frames(4, 240, 320, 50 + i)) for i in range(2)]
    rgb = [_dev(_rgb(4, 240, 320, 50 + i, name)) for i in range(2)]
    keys = ("heat", "depth", "count", "xyc", "points", "overflow")
    with torch.no_grad():
        want = [{k: batched.forward_device(f)[k].clone() for k in keys} for f in rgb]
        eager = {k: batched.forward_device(raw[0])[k].clone() for k in keys}
        _bits_equal(eager, want[0], keys)
        step = batched.capture(raw[0])
        _bits_equal(step.replay(), want[0], keys)
        _bits_equal(step.replay(raw[1]), want[1], keys)
    # InferenceComponent and load_keypoint_net carry the format
    comp = pp.InferenceComponent(net, compute_dtype=torch.bfloat16, frame_format=_fmt("mono"))
    assert comp.model.frame_format == _fmt("mono")
    a = comp(torch.from_numpy(np.array(_frames(4, 240, 320, 50))))
    b = comp(torch.from_numpy(np.array(_rgb(4, 240, 320, 50, "mono"))))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fresh = pp.load_keypoint_net(net.state_dict(), torch.bfloat16, frame_format=_fmt("gbrg"))
    assert fresh.frame_format == _fmt("gbrg")


def test_stereo_stream_pipeline_device_tick_and_host_fed_stream_equal_the_rgb_run():
    from object_keypoints_amd.perception import pipeline as pp
    name = "bggr"
    net = _net(torch.float16, _fmt(name))
    stereo = _stereo()
    h, w, n_pairs = 240, 320, 2
    raw = [_frames(2 * n_pairs, h, w, 40 + t) for t in range(3)]
    rgb = [_rgb(2 * n_pairs, h, w, 40 + t, name) for t in range(3)]
    # the device tick on Bayer frames equals the same tick on the demosaiced frames
    dev = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=256)
    keys = ("count", "xyc", "match", "points", "overflow")
    _bits_equal(dev.tick_device(_dev(raw[0])), dev.tick_device(_dev(rgb[0])), keys)
    # host-fed: pinned Bayer ticks [2P,H,W] through HostFrameFeed give the RGB ticks (capacity far above the random network's peak count)
    host = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=4096)
    want = [host.tick(_dev(f)) for f in rgb]
    ticks = [torch.from_numpy(np.array(f)).pin_memory() for f in raw]
    assert tuple(ticks[0].shape) == (2 * n_pairs, h, w)
    streamed = list(host.stream(ticks))
    assert len(streamed) == 3
    for s, r in zip(streamed, want):
        _same(s, r)


def test_one_net_switched_between_yuv_bayer_and_none():
    """The 4:2:0 path's results do not depend on the presence of the new formats: one net gives on NV12 frames the same bits before and
    after it served Bayer and mono8 frames, and refuses 3-D frames again once its format is None."""
    import yuv_spec
    from object_keypoints_amd import ops
    yuv = ops.YUV420Format("nv12")
    net = _net(torch.bfloat16, yuv)
    h, w = 240, 320
    nv12 = np.random.default_rng(60).integers(0, 256, (2, 3 * h // 2, w), dtype=np.uint8)
    rgb_of_nv12 = _dev(yuv_spec.frames_to_rgb(nv12, w, "nv12"))
    raw = _frames(2, 360, 320, 61)                                       # the same tensor shape as the NV12 frames: only the format tells them apart
    assert raw.shape == nv12.shape
    with torch.no_grad():
        want = [t.clone() for t in net.deployed(rgb_of_nv12)]
        before = [t.clone() for t in net.deployed(_dev(nv12))]
        for name in ("rggb", "mono"):
            net.frame_format = _fmt(name)
            a, b = net.deployed(_dev(raw)), net.deployed(_dev(_rgb(2, 360, 320, 61, name)))
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            assert not torch.equal(a[0], before[0])
        net.frame_format = yuv
        after = net.deployed(_dev(nv12))
        for x, y, z in zip(before, after, want):
            assert torch.equal(x, y) and torch.equal(x, z)
        net.frame_format = None
        with pytest.raises(ops.OkpError, match="frame_format"):
            net.deployed(_dev(raw))
        with pytest.raises(ops.OkpError, match="YUV420Format"):
            ops.preprocess_yuv420(_dev(raw), torch.bfloat16, _fmt("rggb"), size=64)
