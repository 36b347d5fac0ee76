"""Arguments of the fp16-range guard (KeypointNet(range_guard=...), load_keypoint_net, InferenceComponent, LearnedKeypointTrackingPipeline):
what each configuration accepts, what it resolves to, and that nothing of it needs a device."""
import pytest
import torch


def _net(dtype, **kw):
    from object_keypoints_amd.perception.models import KeypointNet
    return KeypointNet(features=128, heatmaps_out=3, compute_dtype=dtype, **kw)


def test_float16_default_is_unguarded_and_true_guards_it():
    net = _net(torch.float16)
    assert net.range_guard is False and net.range_flag() is None and not net.range_overflow()
    assert _net(torch.float16, range_guard=False).range_guard is False
    assert _net(torch.float16, range_guard=True).range_guard is True


def test_split_configurations_are_always_guarded():
    from object_keypoints_amd import ops
    for cfg in ("float32x3", "float32mix"):
        assert _net(cfg).range_guard is True and _net(cfg, range_guard=True).range_guard is True
        with pytest.raises(ops.OkpError, match="cannot be switched off"):
            _net(cfg, range_guard=False)
        net = _net(cfg)
        with pytest.raises(ops.OkpError):
            net.range_guard = False
        assert net.range_guard is True


def test_fp32_range_types_refuse_an_explicit_guard():
    from object_keypoints_amd import ops
    for dtype in (torch.bfloat16, torch.float32):
        with pytest.raises(ops.OkpError, match="range_guard=True"):
            _net(dtype, range_guard=True)
        net = _net(dtype)
        assert net.range_guard is False and net.range_flag() is None
        with pytest.raises(ops.OkpError):
            net.range_guard = True
    with pytest.raises(ops.OkpError):
        _net(torch.float16, range_guard="yes")


def test_internal_fallbacks_keep_working_through_set_compute_dtype():
    """The audit's float16 -> float32x3 -> float32 chain and on_overflow='float32' switch the configuration of a guarded float16 network:
    that is not an explicit request, nothing raises, and the guard follows the configuration."""
    net = _net(torch.float16, range_guard=True)
    net.set_compute_dtype("float32x3")
    assert net.range_guard is True
    net.set_compute_dtype(torch.float32)
    assert net.range_guard is False and net.range_flag() is None
    net.set_compute_dtype(torch.float16)
    assert net.range_guard is True


def test_on_overflow_values_are_still_checked():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception import pipeline as pp
    net = _net(torch.float16, range_guard=True)
    net.on_overflow = "ignore"
    with pytest.raises(ops.OkpError, match="on_overflow"):
        net._guarded(torch.zeros(1), lambda: None, True)
    with pytest.raises(ops.OkpError, match="on_overflow"):
        pp.load_keypoint_net(_net(torch.float16), compute_dtype=torch.float16, device="cpu", on_overflow="ignore", range_guard=True)


def test_loader_passes_range_guard_through():
    from object_keypoints_amd.perception import pipeline as pp
    net = pp.load_keypoint_net(_net(torch.float16), compute_dtype=torch.float16, device="cpu", audit_frames=None, range_guard=True)
    assert net.range_guard is True
    keep = pp.load_keypoint_net(net, device="cpu", audit_frames=None)        # a network passed in keeps its own
    assert keep.range_guard is True
    sd = _net(torch.float16).state_dict()
    fresh = pp.load_keypoint_net(sd, compute_dtype=torch.float16, device="cpu", audit_frames=None, range_guard=True)
    assert fresh.range_guard is True and fresh.configuration() == "float16"


def test_guarded_fire_modules_take_one_launch_only_on_the_matrix_pipe_geometry():
    """okp_fire2 has range-guarded instances of its matrix-pipe forms only (output width a multiple of 16 at stride 1, of 8 at stride 2)."""
    from object_keypoints_amd import ops
    assert ops.fire_fusable(256, 128, 1, 64, 64, guarded=True) and ops.fire_fusable(256, 192, 2, 32, 32, guarded=True)
    assert ops.fire_fusable(256, 128, 1, 24, 24) and not ops.fire_fusable(256, 128, 1, 24, 24, guarded=True)
    assert ops.fire_fusable(256, 192, 2, 20, 20) and not ops.fire_fusable(256, 192, 2, 20, 20, guarded=True)
    assert ops.fire_fusable(384, 192, 1, 40, 40) and not ops.fire_fusable(384, 192, 1, 40, 40, guarded=True)
