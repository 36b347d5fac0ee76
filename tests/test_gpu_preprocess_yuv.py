"""4:2:0 decoder output straight into the network (okp_preprocess_yuv420): the device path equals the specification (tests/yuv_spec.py)
followed by the existing, oracle-pinned resize + crop + normalisation (okp_preprocess_u8), byte for byte, for NV12 and I420, every matrix
and range, pitched surfaces, saturating samples and both bindings; and the network and pipelines give on 4:2:0 frames exactly what they
give on the converted RGB frames."""
import os

import numpy as np
import pytest
import torch

import yuv_spec

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(REPO, "config", "calibration.yaml")
LAYOUTS = ("nv12", "i420")


def _yuv(n, h, w, seed, pitch=None, layout="nv12"):
    """Random 4:2:0 frames as pitched buffers [n, 3h/2, pitch] (0xAB where `layout` has padding) -> (host buffer, host view [..., :w])."""
    pitch = pitch or w
    rng = np.random.default_rng(seed)
    buf = np.full((n, 3 * h // 2, pitch), 0xAB, np.uint8)
    buf[..., :w] = rng.integers(0, 256, (n, 3 * h // 2, w), dtype=np.uint8)
    if pitch > w and layout == "i420":       # the chroma planes are packed rows of pitch/2 bytes, of which the first w/2 are samples
        for f in buf:
            flat = f.reshape(-1)
            c = flat[h * pitch:].reshape(h, pitch // 2)
            c[:, w // 2:] = 0xAB
            c[:, :w // 2] = rng.integers(0, 256, (h, w // 2), dtype=np.uint8)
    t = torch.from_numpy(buf)
    return buf, t[..., :w]


def _fmt(layout, matrix="bt601", full_range=False):
    from object_keypoints_amd import ops
    return ops.YUV420Format(layout, matrix, full_range)


def _rgb(buf, w, fmt):
    return yuv_spec.frames_to_rgb(buf, w, fmt.layout, fmt.matrix, fmt.full_range)


def _net(compute_dtype, frame_format):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=compute_dtype, frame_format=frame_format)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
    return net.eval().cuda()


@pytest.mark.parametrize("shape,size", [((2, 720, 1280), 511), ((1, 98, 62), 33), ((3, 40, 40), 40), ((1, 34, 200), 21)])
@pytest.mark.parametrize("matrix,full_range", yuv_spec.FORMATS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yuv_path_equals_spec_then_rgb_path_bit_exact(layout, matrix, full_range, shape, size):
    from object_keypoints_amd import ops
    from oracle import pipeline as op
    from oracle import preprocess as pre
    n, h, w = shape
    fmt = _fmt(layout, matrix, full_range)
    buf, view = _yuv(n, h, w, seed=h + w + full_range)
    rgb = _rgb(buf, w, fmt)
    got = ops.preprocess_yuv420(view.cuda(), torch.float32, fmt, size=size).t.cpu().numpy()
    want = ops.preprocess_u8(torch.from_numpy(rgb).cuda(), torch.float32, size=size).t.cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    # the interior is the oracle's resize + crop + normalisation of the converted frames
    ref = op.normalize_frames(np.stack([pre.resize_center_crop(f, size) for f in rgb]))
    assert np.array_equal(got[:, 3:3 + size, 3:3 + size, :3].transpose(0, 3, 1, 2), ref)
    halo = got.copy()
    halo[:, 3:3 + size, 3:3 + size, :3] = 0
    assert not halo.any()                                               # zero halo and zero 4th channel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yuv_path_16bit_outputs_equal_the_rgb_path(layout, dtype):
    from object_keypoints_amd import ops
    fmt = _fmt(layout, "bt709")
    buf, view = _yuv(2, 720, 1280, seed=3)
    got = ops.preprocess_yuv420(view.cuda(), dtype, fmt, size=511).t
    want = ops.preprocess_u8(torch.from_numpy(_rgb(buf, 1280, fmt)).cuda(), dtype, size=511).t
    assert got.dtype == dtype and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pitched_surface_view_equals_the_contiguous_frames(layout):
    from object_keypoints_amd import ops
    h, w = 98, 62
    buf, view = _yuv(3, h, w, seed=11, pitch=w + 64, layout=layout)
    assert view.stride(1) == w + 64 and not view.is_contiguous()
    fmt = _fmt(layout)
    packed = np.empty((3, 3 * h // 2, w), np.uint8)                   # the same frames without the padding
    for i in range(3):
        Y, U, V = yuv_spec.planes(buf[i], h, w, layout)
        flat = packed[i].reshape(-1)
        flat[:h * w] = Y.reshape(-1)
        if layout == "nv12":
            uv = flat[h * w:].reshape(h // 2, w)
            uv[:, 0::2], uv[:, 1::2] = U, V
        else:
            flat[h * w:h * w + h * w // 4], flat[h * w + h * w // 4:] = U.reshape(-1), V.reshape(-1)
    assert np.array_equal(yuv_spec.frames_to_rgb(packed, w, layout), _rgb(buf, w, fmt))
    got = ops.preprocess_yuv420(torch.from_numpy(buf).cuda()[..., :w], torch.float32, fmt, size=33).t
    want = ops.preprocess_yuv420(torch.from_numpy(packed).cuda(), torch.float32, fmt, size=33).t
    assert torch.equal(got, want)


@pytest.mark.parametrize("matrix,full_range", yuv_spec.FORMATS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_saturation_every_y_with_the_extreme_chroma_corners(layout, matrix, full_range):
    """Frame k: every Y value 0..255 (16 times) over chroma corner k; the identity resize keeps each converted sample."""
    from object_keypoints_amd import ops
    h = w = 64
    corners = [(0, 0), (0, 255), (255, 0), (255, 255), (128, 128)]
    frames = np.empty((len(corners), 3 * h // 2, w), np.uint8)
    for k, (u, v) in enumerate(corners):
        flat = frames[k].reshape(-1)
        flat[:h * w] = np.arange(h * w) % 256
        if layout == "nv12":
            uv = flat[h * w:].reshape(h // 2, w)
            uv[:, 0::2], uv[:, 1::2] = u, v
        else:
            flat[h * w:h * w + h * w // 4], flat[h * w + h * w // 4:] = u, v
    fmt = _fmt(layout, matrix, full_range)
    rgb = _rgb(frames, w, fmt)
    assert (rgb == 0).any() and (rgb == 255).any()                      # the conversion saturates on both ends
    got = ops.preprocess_yuv420(torch.from_numpy(frames).cuda(), torch.float32, fmt, size=h).t
    want = ops.preprocess_u8(torch.from_numpy(rgb).cuda(), torch.float32, size=h).t
    assert torch.equal(got, want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ctypes_and_torch_ops_bindings_give_the_same_bytes(layout):
    from object_keypoints_amd import _lib, ops
    buf, _ = _yuv(2, 98, 62, seed=5, pitch=128, layout=layout)
    fmt = _fmt(layout, "bt709", True)
    frames = torch.from_numpy(buf).cuda()[..., :62]
    assert _lib.torch_ops() is not None
    launches = ops.COUNTERS["ctypes_launches"]
    a = ops.preprocess_yuv420(frames, torch.bfloat16, fmt, size=33).t
    assert ops.COUNTERS["ctypes_launches"] == launches
    keep = _lib._torch_ops
    try:
        _lib._torch_ops = None                        # the ctypes binding serves the launch
        b = ops.preprocess_yuv420(frames, torch.bfloat16, fmt, size=33).t
    finally:
        _lib._torch_ops = keep
    assert ops.COUNTERS["ctypes_launches"] == launches + 1
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("compute_dtype", [torch.bfloat16, "float32x3"])
def test_network_on_nv12_equals_the_network_on_spec_rgb(compute_dtype):
    fmt = _fmt("nv12")
    net = _net(compute_dtype, fmt)
    buf, view = _yuv(2, 720, 1280, seed=21)
    rgb = torch.from_numpy(_rgb(buf, 1280, fmt)).cuda()
    with torch.no_grad():
        a = net.deployed(view.cuda())
        b = net.deployed(rgb)
    assert len(a) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert tuple(a[0].shape) == (2, 3, 64, 64)


def test_network_refuses_yuv_frames_without_a_format_and_non_unit_strides():
    from object_keypoints_amd import ops
    net = _net(torch.bfloat16, None)
    frames = torch.zeros((1, 96, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(ops.OkpError, match="frame_format"):
        net.deployed(frames)
    net.frame_format = _fmt("i420")
    with pytest.raises(ops.OkpError, match="inner stride"):
        net.deployed(torch.zeros((1, 64, 96), dtype=torch.uint8, device="cuda").transpose(1, 2))
    with pytest.raises(ops.OkpError, match="inner stride"):
        ops.preprocess_yuv420(torch.zeros((1, 64, 96), dtype=torch.uint8, device="cuda").transpose(1, 2), torch.float32, _fmt("nv12"), size=16)


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


def test_stereo_stream_pipeline_on_nv12_frames():
    from object_keypoints_amd.perception import pipeline as pp
    fmt = _fmt("nv12")
    net = _net(torch.float16, fmt)
    stereo = _stereo()
    h, w, n_pairs = 240, 320, 2
    bufs = [_yuv(2 * n_pairs, h, w, seed=40 + t)[0] for t in range(3)]
    # the host tick (capacity far above the random network's peak count) on NV12 equals the same tick on the converted frames
    host = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=4096)
    want = host.tick(torch.from_numpy(_rgb(bufs[0], w, fmt)).cuda())
    resident = [host.tick(torch.from_numpy(b).cuda()) for b in bufs]
    _same(resident[0], want)
    # host-fed: pinned NV12 ticks through HostFrameFeed give the resident ticks
    ticks = [torch.from_numpy(b).pin_memory() for b in bufs]
    streamed = list(host.stream(ticks))
    assert len(streamed) == 3
    for s, r in zip(streamed, resident):
        _same(s, r)
    # the device tick and its graph on NV12 frames
    dev = pp.StereoStreamPipeline(net, stereo, {"keypoint_config": [1, 3]}, capacity=256)
    frames = torch.from_numpy(bufs[0]).cuda()
    keys = ("count", "xyc", "match", "points", "overflow")
    eager = dev.tick_device(frames)
    _bits_equal(eager, dev.tick_device(torch.from_numpy(_rgb(bufs[0], w, fmt)).cuda()), keys)
    step = dev.capture_device(frames)
    step.replay()
    torch.cuda.synchronize()
    _bits_equal(step.static_out, eager, keys)
    frames2 = torch.from_numpy(bufs[1]).cuda()
    step.replay(frames2)
    _bits_equal(step.static_out, dev.tick_device(frames2), keys)


def test_batched_pipeline_capture_and_inference_component_on_nv12():
    from object_keypoints_amd.perception import pipeline as pp
    from object_keypoints_amd.perception.utils import camera_utils as cu
    from oracle import pipeline as op
    fmt = _fmt("nv12")
    net = _net(torch.bfloat16, fmt)
    cam_o = op.eval_camera(CALIB)
    batched = pp.BatchedKeypointPipeline(net, {"keypoint_config": [1, 3]}, cu.FisheyeCamera(cam_o.K, cam_o.D, cam_o.image_size), capacity=256)
    buf, _ = _yuv(4, 240, 320, seed=50)
    buf2, _ = _yuv(4, 240, 320, seed=51)
    frames, frames2 = torch.from_numpy(buf).cuda(), torch.from_numpy(buf2).cuda()
    keys = ("heat", "depth", "count", "xyc", "points", "overflow")
    with torch.no_grad():
        eager = {k: batched.forward_device(frames)[k].clone() for k in keys}
        eager2 = {k: batched.forward_device(frames2)[k].clone() for k in keys}
        step = batched.capture(frames)
        _bits_equal(step.replay(), eager, keys)
        _bits_equal(step.replay(frames2), eager2, keys)
    # InferenceComponent: NV12 frames in, the same maps as the converted RGB frames
    comp = pp.InferenceComponent(net, compute_dtype=torch.bfloat16, frame_format=fmt)
    assert comp.model.frame_format == fmt
    a = comp(torch.from_numpy(buf))
    b = comp(torch.from_numpy(_rgb(buf, 320, fmt)))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fresh = pp.load_keypoint_net(net.state_dict(), torch.bfloat16, frame_format=_fmt("i420"))
    assert fresh.frame_format == _fmt("i420")
