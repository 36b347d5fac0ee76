"""CPU-side checks of the scene-scoring entry points (okp_project_labels, okp_render_targets, okp_keypoint_loss): the NumPy
specification (tests/targets_spec.py) against the reference's golden vectors, every refusal of the three ops functions, the label
order of SceneTargets, and the agreement of header, ctypes table and op registry.  No GPU needed."""
import json
import os
import re

import numpy as np
import pytest
import torch

import targets_spec as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NAMES = ("project_labels", "render_targets", "keypoint_loss")


def _goldens():
    with open(os.path.join(GOLDEN, "targets.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "targets.npz"))


@pytest.mark.parametrize("name", ["valve", "cups"])
def test_spec_reproduces_the_reference_targets(name):
    meta, z = _goldens()
    fx = meta["fixtures"][name]
    tc = [1] + fx["keypoint_config"]
    pts, n_obj = z[f"{name}_labels"], z[f"{name}_n_obj"]
    assert sorted(set(n_obj.tolist())) == [0, 1, 2, 4]
    for f, frame in enumerate(fx["frames"]):
        # the conditions the generator enforced concern the reference alone; the spec sees the same margins
        assert frame["mask_margin"] >= meta["mask_margin"] and (frame["edge_margin"] is None or frame["edge_margin"] >= meta["edge_margin"])
        heat, depth, centers, _ = spec.render_frame(pts[f], int(n_obj[f]), tc)
        gh, gd, gc = z[f"{name}_heat"][f], z[f"{name}_depth"][f], z[f"{name}_centers"][f]
        assert np.array_equal(heat > np.float32(0.01), gh > np.float32(0.01)), frame["what"]
        assert np.array_equal(depth != 0, gd != 0) and np.array_equal(centers != 0, gc != 0)
        for k in range(len(tc)):
            err = float(np.abs(heat[k].astype(np.float64) - gh[k]).max())
            assert err <= spec.heat_tolerance(int(n_obj[f]) * tc[k]), (frame["what"], k, err)
        assert np.array_equal(depth, gd) and np.array_equal(centers, gc)
    assert max(max(fr["raw_max"]) for fr in fx["frames"]) > 1.0          # a map whose maximum exceeds 1 is among the fixtures


@pytest.mark.parametrize("name", ["valve", "cups"])
def test_spec_reproduces_the_reference_loss(name):
    meta, z = _goldens()
    fx = meta["fixtures"][name]
    K = len(fx["keypoint_config"]) + 1
    ph, pd, pc = spec.logits(fx["logit_seed"], z[f"{name}_heat"].shape[0], K, meta["stacks"])
    total, h, d, c, terms, _ = spec.loss(ph, pd, pc, z[f"{name}_heat"], z[f"{name}_depth"], z[f"{name}_centers"])
    e = fx["expected_fp64"]
    assert abs(total - e["loss"]) <= 1e-12 * e["loss"]
    assert np.allclose(h, e["heat"], rtol=1e-12) and np.allclose(d, e["depth"], rtol=1e-12) and np.allclose(c, e["center"], rtol=1e-12)
    assert np.allclose(terms, z[f"{name}_terms"], rtol=1e-12, atol=0)
    assert fx["reference_fp32_vs_fp64"] < 1e-6


def test_header_ctypes_and_op_registry_agree_on_the_new_names():
    from object_keypoints_amd import _lib
    header = open(os.path.join(REPO, "include", "okp.h")).read()
    version_comment = header[header.index("#define OKP_ABI_VERSION 7"):header.index("/* OKP_F16:")]
    assert "additions at 7" in version_comment
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    T = _lib.torch_ops()
    assert T is not None
    for n in NAMES:
        assert f"okp_{n}" in version_comment.split("additions at 7")[1]
        decl = re.search(rf"\bint okp_{n}\s*\(([^;]*)\)\s*;", code)
        assert decl, f"okp_{n} is not declared"
        assert len(decl.group(1).split(",")) == len(bound[f"okp_{n}"]), n
        assert hasattr(_lib.lib(), f"okp_{n}")
        schema = str(getattr(T, n).default._schema)
        assert schema.startswith(f"okp::{n}(") and "(a!)" in schema
    assert "(d!) out" in str(T.keypoint_loss.default._schema) and "(c!) centers" in str(T.render_targets.default._schema)
    assert _lib.lib().okp_abi_version() == 7


def _valid(n=2, k=4, s=2, max_obj=3, tc=(1, 1, 1, 1)):
    nk = sum(tc)
    return dict(ph=[torch.zeros(n, k, 64, 64) for _ in range(s)], pd=[torch.zeros(n, k, 64, 64) for _ in range(s)],
                pc=[torch.zeros(n, k - 1, 2, 64, 64) for _ in range(s)], labels=torch.zeros(n, max_obj * nk, 3, dtype=torch.float64),
                n_obj=torch.zeros(n, dtype=torch.int32), tc=list(tc))


def test_calls_without_a_device_raise_the_no_cpu_fallback_error():
    from object_keypoints_amd import ops
    v = _valid()
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.render_targets(v["labels"], v["n_obj"], v["tc"])
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.keypoint_loss(v["ph"], v["pd"], v["pc"], v["tc"], labels=v["labels"], n_obj=v["n_obj"])
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.keypoint_loss(v["ph"], v["pd"], v["pc"], v["tc"], targets=(torch.zeros(2, 4, 64, 64), torch.zeros(2, 4, 64, 64), torch.zeros(2, 3, 2, 64, 64)))
    cam = ops.make_camera(np.array([[400.0, 0, 320], [0, 400, 240], [0, 0, 1]]), np.zeros(4))
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        ops.project_labels(cam, torch.zeros(5, 3, dtype=torch.float64), torch.eye(4, dtype=torch.float64)[None])
    T = ops._lib.torch_ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.render_targets(v["labels"], v["n_obj"], v["tc"], torch.zeros(2, 4, 64, 64), torch.zeros(2, 4, 64, 64), torch.zeros(2, 3, 2, 64, 64), 0)
    from object_keypoints_amd.perception.loss import KeypointLoss
    with pytest.raises(ops.OkpError, match="no CPU fallback"):
        KeypointLoss([1, 1, 1]).from_labels(v["ph"], v["pd"], v["pc"], {"points": v["labels"], "n_obj": v["n_obj"]})


def test_project_labels_refusals():
    from object_keypoints_amd import ops
    cam = ops.make_camera(np.array([[400.0, 0, 320], [0, 400, 240], [0, 0, 1]]), np.zeros(4))
    w, T = torch.zeros(5, 3, dtype=torch.float64), torch.eye(4, dtype=torch.float64)[None]
    bad_cam = ops.make_camera(np.eye(3), np.zeros(4))
    bad_cam.model = 7
    for args, kw, msg in [((None, w, T), {}, "cam"), ((bad_cam, w, T), {}, "camera model"), ((cam, w.float(), T), {}, "world_points"),
                          ((cam, torch.zeros(5, 2, dtype=torch.float64), T), {}, "world_points"), ((cam, w, T.float()), {}, "T_WC"),
                          ((cam, w, T[0]), {}, "T_WC"), ((cam, w.t().contiguous().t(), T), {}, "contiguous"), ((cam, w, T), {"scale": 0.0}, "scale"),
                          ((cam, w, T), {"crop": (1.0,)}, "crop")]:
        with pytest.raises(ops.OkpError, match=msg):
            ops.project_labels(*args, **kw)
    assert ops.raw_to_input((720, 1280)) == (511 / 720, 198.0, 0.0)
    with pytest.raises(ops.OkpError, match="raw_size"):
        ops.raw_to_input((0, 0))


def test_render_targets_refusals():
    from object_keypoints_amd import ops
    v = _valid()
    L, n_obj, tc = v["labels"], v["n_obj"], v["tc"]
    for args, msg in [((L.float(), n_obj, tc), "labels"), ((L, n_obj.long(), tc), "n_obj"), ((L[:, :10], n_obj, tc), "labels"),
                      ((L[..., :2], n_obj, tc), "labels"), ((L, n_obj[:1], tc), "n_obj"), ((L, n_obj, [2, 1, 1, 1]), "centre map"),
                      ((L, n_obj, [1]), "maps"), ((L, n_obj, [1] * 17), "maps"), ((L, n_obj, [1, 0, 2, 1]), "at least one"),
                      ((L, n_obj, "abcd"), "type_count"), ((torch.zeros(2, 65 * 4, 3, dtype=torch.float64), n_obj, tc), "capacity"),
                      ((torch.zeros(2, 64 * 10, 3, dtype=torch.float64), n_obj, [1, 9]), "per map"),
                      ((torch.zeros(2, 24, 3, dtype=torch.float64)[:, ::2], n_obj, tc), "contiguous")]:
        with pytest.raises(ops.OkpError, match=msg):
            ops.render_targets(*args)


def test_keypoint_loss_refusals():
    from object_keypoints_amd import ops
    v = _valid()
    ph, pd, pc, L, n_obj, tc = v["ph"], v["pd"], v["pc"], v["labels"], v["n_obj"], v["tc"]
    dense = (torch.zeros(2, 4, 64, 64), torch.zeros(2, 4, 64, 64), torch.zeros(2, 3, 2, 64, 64))
    lab = dict(labels=L, n_obj=n_obj)
    cases = [((ph[0], pd, pc, tc), lab, "p_heatmaps"), ((ph, pd[:1], pc, tc), lab, "per stack"), ((ph * 3, pd * 3, pc * 3, tc), lab, "stacks"),
             ((ph, pd, pc, [2, 1, 1, 1]), lab, "centre map"), (([ph[0].double(), ph[1]], pd, pc, tc), lab, "float32"),
             (([ph[0][:, :3], ph[1]], pd, pc, tc), lab, "heat must be"), ((ph, [pd[0][:1], pd[1]], pc, tc), lab, "depth must be"),
             ((ph, pd, [pc[0][:, :, :1], pc[1]], tc), lab, "centers must be"), ((ph, pd, [pc[0].transpose(3, 4), pc[1]], tc), lab, "contiguous"),
             (([ph[0][0], ph[1]], pd, pc, tc), lab, "p_heatmaps"),
             ((ph, pd, pc, tc), {}, "either labels"), ((ph, pd, pc, tc), dict(labels=L, n_obj=n_obj, targets=dense), "either labels"),
             ((ph, pd, pc, tc), dict(labels=L), "n_obj"), ((ph, pd, pc, tc), dict(labels=L[:1], n_obj=n_obj[:1]), "frames"),
             ((ph, pd, pc, tc), dict(targets=dense, n_obj=n_obj), "n_obj goes with labels"), ((ph, pd, pc, tc), dict(targets=dense[:2]), "targets must be"),
             ((ph, pd, pc, tc), dict(targets=(dense[0][:1], dense[1], dense[2])), "target heat"),
             ((ph, pd, pc, tc), dict(targets=(dense[0], dense[1], dense[2].double())), "target centers"),
             ((ph, pd, pc, tc), dict(first=1, total=2, **lab), "inside the batch"), ((ph, pd, pc, tc), dict(first=-1, total=2, **lab), "inside the batch"),
             ((ph, pd, pc, tc), dict(first=2, total=4, labels=torch.zeros(4, 12, 3, dtype=torch.float64), n_obj=torch.zeros(4, dtype=torch.int32)), "state"),
             ((ph, pd, pc, tc), dict(state={"partial": torch.zeros(1)}, **lab), "state")]
    for args, kw, msg in cases:
        with pytest.raises(ops.OkpError, match=msg):
            ops.keypoint_loss(*args, **kw)
    from object_keypoints_amd.perception.loss import KeypointLoss
    with pytest.raises(NotImplementedError):
        KeypointLoss([1, 3], reduction="max")
    with pytest.raises(ops.OkpError, match="labels must be"):
        KeypointLoss([1, 3]).from_labels(ph, pd, pc, L)
    crit = KeypointLoss([1, 3], depth_weight=3.0)
    assert crit.n_keypoint_maps == 3 and crit.depth_weight == 3.0 and crit.center_weight == 1.0 and crit.type_count == [1, 1, 3]


def test_scene_targets_inserts_the_centre_and_keeps_the_label_order():
    from object_keypoints_amd import ops
    from object_keypoints_amd.perception.datasets import SceneTargets
    from object_keypoints_amd.perception.utils import camera_utils as cu
    cam = cu.FisheyeCamera(np.array([[700.0, 0, 640], [0, 700.0, 360], [0, 0, 1]]), np.array([0.01, -0.002, 0.0005, 0.0]), (720, 1280))
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (8, 4))                       # 2 objects x 4 key points ([1, 3]), with a 4th column as keypoints.json has
    st = SceneTargets({"keypoint_config": [1, 3]}, cam, pts)
    assert st.keypoint_config == [1, 1, 3] and st.n_keypoints == 5 and st.n_objects == 2 and st.keypoint_maps == 3
    assert st.world_points.shape == (10, 3)
    for o in range(2):
        assert np.array_equal(st.world_points[o * 5], pts[o * 4:(o + 1) * 4, :3].mean(axis=0))
        assert np.array_equal(st.world_points[o * 5 + 1:(o + 1) * 5], pts[o * 4:(o + 1) * 4, :3])
    assert (st.scale, st.crop_x, st.crop_y) == (511 / 720, 198.0, 0.0)
    assert SceneTargets([1, 1, 1], cam, pts[:6]).n_objects == 2
    with pytest.raises(ops.OkpError, match="wrong number of keypoints"):
        SceneTargets([1, 3], cam, pts[:7])
    if not torch.cuda.is_available():
        with pytest.raises(ops.OkpError, match="no CPU fallback"):
            st.labels(np.eye(4)[None])
