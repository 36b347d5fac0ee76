"""SceneScorer: the network's raw logits of both stacks scored against labels on the device, eagerly and as a captured step, and the
same weights compared across compute configurations."""
import numpy as np
import pytest
import torch

import targets_spec as spec

pytestmark = pytest.mark.gpu
CFG = {"keypoint_config": [1, 3]}


def _state(seed=0, k=3):
    from object_keypoints_amd import synth
    from object_keypoints_amd.perception.models import KeypointNet
    shapes = {kk: tuple(v.shape) for kk, v in KeypointNet(features=128, heatmaps_out=k).state_dict().items()}
    return {kk: torch.from_numpy(np.array(v)) for kk, v in synth.fill_state_dict(shapes, seed=seed).items()}


def _net(dtype, sd, k=3, on_overflow="raise"):
    from object_keypoints_amd.perception.models import KeypointNet
    net = KeypointNet(features=128, heatmaps_out=k, compute_dtype=dtype)
    net.load_state_dict(sd)
    net.on_overflow = on_overflow
    return net.eval().cuda()


def _frames(n, seed=77):
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    return torch.randn((n, 3, 511, 511), generator=gen, device="cuda", dtype=torch.float32)


def _labels(n, seed=3, max_obj=4):
    pts, n_obj = spec.random_labels(seed, n, [1, 1, 3], max_obj)
    return {"points": torch.from_numpy(pts).cuda(), "n_obj": torch.from_numpy(n_obj).cuda()}


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_score_is_forward_plus_the_fused_loss_and_replays_bit_equal_from_a_graph():
    from object_keypoints_amd.perception.loss import KeypointLoss
    from object_keypoints_amd.perception.pipeline import SceneScorer
    net = _net(torch.bfloat16, _state())
    scorer = SceneScorer(net, CFG, depth_weight=5.0)
    frames, labels = _frames(4), _labels(4)
    got = scorer.score(frames, labels)
    assert set(got) == {"loss", "heat", "depth", "center", "terms", "mask_count", "range_overflow"}
    assert all(v.is_cuda for v in got.values()) and got["terms"].shape == (4, 2, 3) and got["mask_count"].shape == (4, 3)
    heat, depth, centers = net.forward(frames)
    crit = KeypointLoss([1, 3], depth_weight=5.0)
    loss, hl, dl, cl = crit.from_labels(list(heat), list(depth), list(centers), labels)
    assert torch.equal(_bits(loss), _bits(got["loss"])) and torch.equal(_bits(torch.stack(hl)), _bits(got["heat"]))
    assert torch.equal(_bits(torch.stack(dl)), _bits(got["depth"])) and torch.equal(_bits(torch.stack(cl)), _bits(got["center"]))
    assert np.isfinite(float(loss)) and float(loss) > 0 and int(got["range_overflow"]) == 0
    eager = {k: v.clone() for k, v in got.items()}
    # stream capture refuses every operation that synchronises with the host: capturing the step is the proof that score() has none
    step = scorer.capture(frames, labels)
    other, other_labels = _frames(4, seed=5), _labels(4, seed=8)
    step.static_labels["points"].copy_(other_labels["points"]); step.static_labels["n_obj"].copy_(other_labels["n_obj"])
    changed = {k: v.clone() for k, v in step.replay(other).items()}
    assert not torch.equal(_bits(changed["loss"]), _bits(eager["loss"]))
    step.static_labels["points"].copy_(labels["points"]); step.static_labels["n_obj"].copy_(labels["n_obj"])
    replayed = step.replay(frames)
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(_bits(replayed[k]), _bits(eager[k])), k
    want = scorer.score(other, other_labels)
    assert torch.equal(_bits(want["loss"]), _bits(changed["loss"])) and torch.equal(_bits(want["terms"]), _bits(changed["terms"]))


def test_compare_scores_configurations_on_the_same_weights():
    from object_keypoints_amd.perception.pipeline import SceneScorer
    net = _net(torch.float32, _state())
    scorer = SceneScorer(net, CFG)
    frames, labels = _frames(2), _labels(2)
    out = scorer.compare(frames, labels, ["float32x3", torch.bfloat16])
    assert set(out) == {"float32x3", "bfloat16"} and net.configuration() == "float32"
    a, b = float(out["float32x3"]["loss"]), float(out["bfloat16"]["loss"])
    print(f"float32x3 {a:.9g} bfloat16 {b:.9g}")
    assert np.isfinite(a) and np.isfinite(b) and a != b
    assert int(out["float32x3"]["range_overflow"]) == 0 and int(out["bfloat16"]["range_overflow"]) == 0


def test_range_overflow_is_reported():
    """One BatchNorm gain scaled so that an activation passes 65504: the split-product score carries the flag, no exception, no host read."""
    from object_keypoints_amd.perception.pipeline import SceneScorer
    sd = _state()
    big = dict(sd)
    big["backbone.pre.1.bn2.weight"] = sd["backbone.pre.1.bn2.weight"] * 3.0e5
    frames, labels = _frames(2), _labels(2)
    assert int(SceneScorer(_net("float32x3", big), CFG).score(frames, labels)["range_overflow"]) != 0
    assert int(SceneScorer(_net("float32x3", sd), CFG).score(frames, labels)["range_overflow"]) == 0
    assert int(SceneScorer(_net(torch.float32, big), CFG).score(frames, labels)["range_overflow"]) == 0
