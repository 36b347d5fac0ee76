"""A rig of individually calibrated stereo pairs on the device (StereoStreamPipeline over a sequence of StereoCameras; okp_stereo_match_rig /
okp_stereo_triangulate_rig): four clearly different pairs (synth.stereo_rig: baselines 6 - 30 cm, focal lengths and principal points 5-15 %
apart, different distortion, a few degrees of relative rotation), each pair's heat maps rendered through that pair's own cameras.  The rig
tick recovers the rendered points; each pair equals, bit for bit, a single-calibration pipeline of that pair; the device tick agrees with
the host tick; the captured graph, first_pair and the overflow word behave as for a single calibration; and the single-calibration tick
(a one-entry table) equals the by-value entry points bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"keypoint_config": [1, 3]}
BAR = 0.06                    # metres: the bar of test_stereo_stream_pipeline_tick_recovers_the_rendered_points (64 x 64 maps)


def _rig(n_pairs=4):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.utils import camera_utils as cu
    return synth.stereo_rig(cu.load_calibration_params(os.path.join(REPO, "config", "calibration.yaml")), n_pairs)


def _heat(rig, **kw):
    from object_keypoints_amd import synth
    return torch.from_numpy(synth.render_rig_heat(rig, **kw)).cuda()


_NET = []


def _net():
    if not _NET:
        from object_keypoints_amd import synth
        from object_keypoints_amd.perception.models import KeypointNet
        net = KeypointNet(features=128, heatmaps_out=3, compute_dtype=torch.float16)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.fill_state_dict(shapes, seed=0).items()})
        _NET.append(net.eval().cuda())
    return _NET[0]


def _frames(n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device="cuda", dtype=torch.float32)


def _pipe(cal, capacity=8):
    from object_keypoints_amd.perception import pipeline as pp
    return pp.StereoStreamPipeline(_net(), cal, CFG, capacity=capacity, max_distance=1.5)


def _recovered(result, pairs, shift=0.0):
    """Per pair: every rendered point found (5 per pair), each within BAR of a rendered point of its type."""
    from object_keypoints_amd import synth
    ok = []
    for got, q in zip(result, pairs):
        good = True
        for k, want in synth.rig_scene_points(q, shift).items():
            if got[k].shape != want.shape:
                good = False
                continue
            d = np.linalg.norm(got[k][:, None] - want[None], axis=2).min(axis=1)
            good = good and bool(d.max() < BAR)
        ok.append(good)
    return ok


def _same(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert sorted(pa) == sorted(pb)
        for k in pa:
            assert pa[k].shape == pb[k].shape and pa[k].dtype == pb[k].dtype == np.float64
            if pa[k].size:
                assert np.abs(pa[k] - pb[k]).max() <= 1e-9


def _bits(x, y):
    """Bit-equal tensors, NaN pattern included."""
    assert x.shape == y.shape and x.dtype == y.dtype
    if x.is_floating_point():
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))
    else:
        assert torch.equal(x, y)


def _bits_equal(x, y, keys=("count", "xyc", "match", "points", "overflow")):
    for key in keys:
        _bits(x[key], y[key])


def test_rig_tick_recovers_every_rendered_point_and_agrees_with_the_host_tick():
    rig = _rig()
    pipe = _pipe(rig)
    heat, frames = _heat(rig), _frames(8, seed=41)
    out = pipe.tick_device(frames, heat_override=heat)
    assert int(out["overflow"]) == 0 and tuple(out["points"].shape) == (4, 3, 8, 4)
    got = pipe.results(out)
    assert _recovered(got, range(4)) == [True] * 4
    _same(got, pipe.tick(frames, heat_override=heat))                              # the host path, pair by pair: 1e-9 m
    # the fixture itself: pair 0's calibration for every pair misses the bar (or loses matches) on another pair
    single = _pipe(rig[0])
    wrong = _recovered(single.results(single.tick_device(frames, heat_override=heat)), range(4))
    assert wrong[0] and not all(wrong[1:]), wrong


@pytest.mark.parametrize("capacity", [8, 7])          # 7: K cap = 21 slots per pair, not a multiple of the eight slots of a wave
def test_each_pair_equals_its_own_single_calibration_pipeline(capacity):
    rig = _rig()
    pipe = _pipe(rig, capacity)
    heat, frames = _heat(rig), _frames(8, seed=42)
    out = pipe.tick_device(frames, heat_override=heat)
    for q in range(4):
        one = _pipe(rig[q], capacity)
        o = one.tick_device(frames[2 * q:2 * q + 2], heat_override=heat[2 * q:2 * q + 2])
        _bits(out["count"][2 * q:2 * q + 2], o["count"])
        _bits(out["xyc"][2 * q:2 * q + 2], o["xyc"])
        _bits(out["match"][q:q + 1], o["match"])
        _bits(out["points"][q:q + 1], o["points"])
        _bits(out["overflow"], o["overflow"])
        assert int((o["match"] >= 0).sum()) == 5


def test_rig_graph_first_pair_and_overflow():
    rig = _rig()
    pipe = _pipe(rig)
    heat, frames = _heat(rig), _frames(8, seed=43)
    out = pipe.tick_device(frames, heat_override=heat)
    # pairs 2..3 alone, calibrated by their rig-wide index: rows 2..3 of the whole tick, bit for bit
    part = pipe.tick_device(frames[4:], heat_override=heat[4:], first_pair=2)
    for key in ("count", "xyc"):
        _bits(part[key], out[key][4:])
    for key in ("match", "points"):
        _bits(part[key], out[key][2:])
    # the whole rig tick as one graph: bit-equal to the eager tick; new static inputs -> the new tick's results
    step = pipe.capture_device(frames, heat_override=heat)
    step.replay()
    torch.cuda.synchronize()
    _bits_equal(step.static_out, out)
    heat2, frames2 = _heat(rig, shift=0.03), _frames(8, seed=44)
    step.replay(frames2, heat_override=heat2)
    torch.cuda.synchronize()
    _bits_equal(step.static_out, pipe.tick_device(frames2, heat_override=heat2))
    got = pipe.results(step.static_out)
    assert _recovered(got, range(4), shift=0.03) == [True] * 4
    _same(got, pipe.tick(frames2, heat_override=heat2))
    # a crowded map on pair 2 sets bit 0 of the overflow word; the next clean tick clears it
    crowded = _heat(rig, crowd=(2, 1, 2))
    step.replay(heat_override=crowded)
    assert int(step.static_out["overflow"]) == 1
    step.replay(heat_override=heat2)
    assert int(step.static_out["overflow"]) == 0
    assert int(pipe.tick_device(frames, heat_override=crowded)["overflow"]) == 1
    assert int(pipe.tick_device(frames, heat_override=heat)["overflow"]) == 0
    # refusals, before any launch
    from object_keypoints_amd.ops import OkpError
    with pytest.raises(OkpError, match="a tick holds 8"):
        pipe.tick(frames[:6], heat_override=heat[:6])
    with pytest.raises(OkpError, match="the rig has 4"):
        pipe.tick_device(frames[4:], heat_override=heat[4:], first_pair=3)
    with pytest.raises(OkpError, match="the rig has 4"):
        pipe.tick_device(torch.cat([frames, frames[:2]]))


def test_single_calibration_tick_equals_the_by_value_entry_points():
    """One StereoCamera: tick_device runs on a one-entry table broadcast to every pair; its payload equals what okp_stereo_match /
    okp_stereo_triangulate (calibration by value) compute on the same peaks, bit for bit."""
    from object_keypoints_amd import ops
    st = _rig(1)[0]                                 # (the scene of all four pairs stays inside its maps)
    for capacity in (8, 7):
        pipe = _pipe(st, capacity)
        heat, frames = _heat([st] * 4), _frames(8, seed=45)
        out = pipe.tick_device(frames, heat_override=heat)
        assert tuple(pipe._table(frames.device).shape)[0] == 1
        cl, cr = ops.make_camera(st.left_camera.K, st.left_camera.D), ops.make_camera(st.right_camera.K, st.right_camera.D)
        match, flag = ops.stereo_match(cl, cr, st.F, out["count"], out["xyc"], 1.5)
        points = ops.stereo_triangulate(cl, cr, st.T_RL, out["count"], out["xyc"], match, F=st.F)
        _bits(out["match"], match)
        _bits(out["points"], points)
        _bits(out["overflow"], flag)
        assert int((match >= 0).sum()) == 20
        # and through the rig entry points with a four-entry table of the same pair and a first_pair
        table = ops.stereo_rig([st] * 4).cuda()
        m2, _ = ops.stereo_match_rig(table, out["count"][4:], out["xyc"][4:], 1.5, first_pair=2)
        _bits(m2, match[2:])
        _bits(ops.stereo_triangulate_rig(table, out["count"][4:], out["xyc"][4:], m2, first_pair=2), points[2:])
