"""okp_group_objects (csrc/okp_geom.hip) against its NumPy specification (tests/group_objects_spec.py, written from include/okp.h), through
ops.group_objects, on inputs built directly (tests/group_objects_cases.py: no network, no NMS in front).  Every comparison is of WHOLE
tensors:
  * n_obj, sel, n_votes, assign: identical (torch.equal);
  * pred: bit for bit - it is one exact int -> double conversion, one exact + 0.5 and one fp64 add, which no contraction can change;
  * reduced: the same NaN pattern, and |device - spec_fp64| <= spacing_fp32(|spec_fp64|), one fp32 ulp.  The bound is derived, not measured:
    the device and the specification run the same algorithm in fp64 and differ only in the order of their sums (a wave butterfly against
    an exactly rounded sum), at most about 64 * 2^-53 relative per coordinate, far below the fp32 rounding that follows - provided no decision
    inside the algorithm is close to a tie, which tests/test_group_objects_args.py asserts for every case used here (decision margin above
    1e-9).  The hand-made integer cases, where every operation is exact, hold the exact ties and are compared bit for bit.
The oracle's k-means is not compared here (tests/test_gpu_pipeline.py does that, as a set): this file pins the kernel to the deterministic
contract the header promises."""
import numpy as np
import pytest
import torch

import group_objects_cases as gc
import group_objects_spec as spec

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_obj", "sel", "n_votes", "assign")


def _device(case, frames=None):
    from object_keypoints_amd import ops
    pick = slice(None) if frames is None else frames
    to = lambda key: torch.from_numpy(np.ascontiguousarray(case[key][pick])).cuda()
    out = ops.group_objects(to("count"), to("xyc"), to("centers"), case["type_count"], max_obj=case["max_obj"], max_sel=case["max_sel"],
                            max_dist=case["max_dist"])
    torch.cuda.synchronize()
    return out


def _bits(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype
    if x.is_floating_point():
        view = torch.int64 if x.dtype == torch.float64 else torch.int32
        x, y = x.contiguous().view(view), y.contiguous().view(view)
    return torch.equal(x, y)


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert _bits(a[key], b[key]), key


def _against_spec(case, name=""):
    want = spec.group_objects(case["count"], case["xyc"], case["centers"], case["type_count"], case["max_dist"], case["max_obj"], case["max_sel"])
    assert case["exact"] or want["margin"] > gc.MARGIN
    out = _device(case)
    got = {k: v.cpu() for k, v in out.items()}
    for key in INT_KEYS:
        assert got[key].dtype == torch.int32 and torch.equal(got[key], torch.from_numpy(want[key])), key
    assert got["pred"].dtype == torch.float64
    p_got, p_want = got["pred"].numpy(), want["pred"]
    assert np.array_equal(np.isnan(p_got), np.isnan(p_want))
    assert np.array_equal(np.nan_to_num(p_got, nan=0.0).view(np.int64), np.nan_to_num(p_want, nan=0.0).view(np.int64)), "pred differs in some bit"
    r_got, r_want = got["reduced"].numpy(), want["reduced"]
    assert r_got.dtype == np.float32 and np.array_equal(np.isnan(r_got), np.isnan(r_want))
    ran = ~np.isnan(r_want)
    if case["exact"]:
        assert np.array_equal(r_got[ran], r_want[ran])
    else:
        # the specification's centres in fp64 are within half an fp32 ulp of r_want; compare with what was rounded, bound one fp32 ulp
        err = np.abs(r_got[ran].astype(np.float64) - r_want[ran].astype(np.float64))
        ulp = np.spacing(np.abs(r_want[ran])).astype(np.float64)
        worst = float((err / ulp).max()) if err.size else 0.0
        print(f"{name}: {int(ran.sum()) // 2} reduced centres, max |device - spec| = {worst:.2f} fp32 ulp, margin {want['margin']:.2e}")
        assert (err <= ulp).all()
    return out, want


def _spec_fp64_reduced(case, want):
    """The reduction of every (frame, object, type) that ran, in fp64 (before the rounding to fp32): {(f, o, i): [want][2]}."""
    out = {}
    for f, o, i in zip(*np.nonzero(~np.isnan(want["reduced"][..., 0, 0]))):
        votes = np.nonzero(want["assign"][f, i + 1] == o)[0][:spec.KM_VOTES]
        out[(f, o, i)] = spec.reduce_votes(case["xyc"][f, i + 1, votes, :2].astype(np.float64), case["xyc"][f, i + 1, votes, 2], case["type_count"][i])
    return out


def _reduced_within_one_ulp_of_fp64(case, out, want):
    """The assertion as the contract states it: |reduced_device - spec_fp64| <= spacing_fp32(|spec_fp64|)."""
    got = out["reduced"].cpu().numpy()
    for (f, o, i), c in _spec_fp64_reduced(case, want).items():
        dev = got[f, o, i, :len(c)].astype(np.float64)
        assert (np.abs(dev - c) <= np.spacing(np.abs(c).astype(np.float32)).astype(np.float64)).all(), (f, o, i)


def _case(name):
    case = gc.HAND_MADE[name]()
    out, want = _against_spec(case, name)
    if not case["exact"]:
        _reduced_within_one_ulp_of_fp64(case, out, want)
    return case, {k: v.cpu().numpy() for k, v in out.items()}


def test_votes_across_lane_batches():
    """More than 64 peaks in a map (cap = 256): the running vote count, the "most confident, first one wins ties" rule and the slot number
    of a multi-instance vote all cross the 64-lane batches; object 0 is voted for in batches 0 and 2 but not in 1 or 3."""
    case, got = _case("votes_across_lane_batches")
    assert got["sel"][0, 1, 0, 0] == 5                           # equal top confidence in batch 0 and batch 3: the first
    assert got["sel"][0, 1, 1, 0] == 200                         # strictly larger in batch 3: the later
    assert got["sel"][0, 0, 2].tolist() == [60, 63, 130, 131, 190, -1, -1, -1]       # peak order across batches (max_sel = 8)
    assert got["sel"][0, 1, 2].tolist() == [0, 1, 64, 255, -1, -1, -1, -1]


def test_more_centres_than_max_obj():
    """count[0] = max_obj + 3: a vote nearest to a dropped centre goes to the nearest kept one, or to none."""
    case, got = _case("more_centres_than_max_obj")
    assert got["n_obj"].tolist() == [4] and got["assign"][0, 1, :2].tolist() == [3, -1]


def test_more_peaks_than_cap():
    """count[k] = cap + 5, and count[0] above cap with max_obj above cap: only what is stored takes part."""
    case, got = _case("more_peaks_than_cap")
    assert got["n_obj"].tolist() == [7]


def test_no_centre_leaves_every_output_at_its_unused_value():
    """count[0] = 0 (nobj == 0): sel -1, n_votes 0, assign -1, pred 0, reduced NaN - in a batch whose other frame is ordinary."""
    case, got = _case("no_centre")
    assert got["n_obj"].tolist() == [0, 2] and (got["sel"][0] == -1).all() and (got["n_votes"][0] == 0).all() and (got["assign"][0] == -1).all()
    assert (got["pred"][0] == 0).all() and np.isnan(got["reduced"][0]).all()


def test_every_lane_an_object():
    """max_obj = 64 with 64 centres."""
    case, got = _case("every_lane_an_object")
    assert got["n_obj"].tolist() == [64] and got["n_votes"][0, 63].sum() > 0


def test_one_object_slot():
    """max_obj = 1."""
    case, got = _case("one_object_slot")
    assert got["n_obj"].tolist() == [1]


def test_gate_and_ties_on_integer_geometry():
    """A vote at exactly max_dist is kept, the next fp32 offset above is dropped; a vote on the perpendicular bisector of two centres (3-4-5)
    goes to the lower index; coordinates 10.5 and 11.5 read pixels 10 and 12 (half to even); -3.2 and W + 7 are clipped; the k-means ties
    (lowest index, lower cluster, earliest seed) on collinear integer votes.  Exact with or without fused multiply-add: bit for bit."""
    case, got = _case("gate_and_ties_on_integer_geometry")
    assert case["exact"]
    assert got["assign"][0, 1, :3].tolist() == [0, -1, 0] and got["assign"][0, 2, :3].tolist() == [0, 0, -1]
    assert got["assign"][1, 1, :4].tolist() == [0, 0, 1, 1] and got["sel"][1, 1, 0, 0] == 2
    assert got["reduced"][1, 0, 1, :2].tolist() == [[12.5, 12.0], [14.0, 12.0]]
    assert got["pred"][2, 1, :4].tolist() == [[9.0, 6.0]] * 4 and got["assign"][2, 2, :5].tolist() == [1, 2, 3, 0, 3]


@pytest.mark.parametrize("name", ["map_48x80", "map_5x700"])
def test_maps_that_are_not_square(name):
    """H != W: the index is yi * W + xi and the second plane H * W further; the offsets differ between the planes."""
    _case(name)


@pytest.mark.parametrize("max_sel", [8, 4])
def test_eight_maps(max_sel):
    """K = 8, type_count [1, 3, 1, 2, 8, 1, 4]; at max_sel = 4 the eight-instance type keeps its first four votes and is not reduced;
    max_sel = 1 is among the random batches."""
    case, got = _case(f"eight_maps_max_sel_{max_sel}")
    ran = ~np.isnan(got["reduced"][:, :5, 4, 0, 0])
    assert ran.all() if max_sel == 8 else not ran.any()
    assert (got["sel"][:, :5, 4] >= 0).all()


def test_non_finite_offsets():
    """A NaN or an infinity in the centre map under a peak: no vote (assign -1), pred holds the value, the other peaks are unaffected."""
    case, got = _case("non_finite_offsets")
    assert [int(got["assign"][0, k, j]) for k, j in ((1, 2), (1, 5), (2, 0), (2, 3))] == [-1] * 4 and got["n_votes"][0].sum() == 16


def test_seventy_votes_for_one_object():
    """More than 64 votes for one object: the first 64 are reduced; the compaction of the second batch would pass lane 63."""
    case, got = _case("seventy_votes_for_one_object")
    assert got["n_votes"][0, 0, 0] == 70


def test_three_surplus_objects_one_at_index_63():
    case, got = _case("three_surplus_objects")
    assert np.nonzero(~np.isnan(got["reduced"][0, :, 0, 0, 0]))[0].tolist() == [2, 31, 63]


def test_surplus_across_a_batch_boundary():
    """The surplus object's votes sit in the last lanes of batch 0 and the first of batch 1."""
    _case("surplus_across_a_batch_boundary")


def test_a_launch_without_reduced_leaves_the_other_outputs_as_they_are():
    """reduced == NULL is legal ("no reduction"): the C entry point with a NULL pointer gives the same five other tensors."""
    from object_keypoints_amd import _lib
    case = gc.HAND_MADE["three_surplus_objects"]()
    full = _device(case)
    dev = {k: torch.from_numpy(case[k]).cuda() for k in ("count", "xyc", "centers")}
    N, K, cap, _ = case["xyc"].shape
    H, W = case["centers"].shape[3:]
    out = {k: torch.empty_like(v) for k, v in full.items() if k != "reduced"}
    import ctypes
    tc = (ctypes.c_int32 * (K - 1))(*case["type_count"])
    _lib.check(_lib.lib().okp_group_objects(dev["count"].data_ptr(), dev["xyc"].data_ptr(), dev["centers"].data_ptr(), N, K, cap, H, W, tc, case["max_dist"],
                                            case["max_obj"], case["max_sel"], out["n_obj"].data_ptr(), out["sel"].data_ptr(), out["n_votes"].data_ptr(),
                                            out["assign"].data_ptr(), out["pred"].data_ptr(), None, None), "okp_group_objects")
    torch.cuda.synchronize()
    for key in out:
        assert _bits(out[key], full[key]), key


@pytest.mark.parametrize("n,seed", gc.RANDOM_BATCHES)
def test_random_batch(n, seed, monkeypatch):
    """Seeded batches of 64 frames and of one, over K, cap in {1, 7, 64, 65, 130, 256}, max_sel in {1, 2, 4, 8}, counts from nothing to past
    the capacities: against the specification; the batch equals its frames run one by one (frames are independent); a second launch gives
    the same bits; the ctypes and the torch.ops.okp binding give the same bits."""
    from object_keypoints_amd import _lib, ops
    case = gc.random_batch(n, seed)
    out, want = _against_spec(case, f"random batch n={n} seed={seed}")
    _reduced_within_one_ulp_of_fp64(case, out, want)
    _same_bits(out, _device(case))
    for f in range(n):
        one = _device(case, slice(f, f + 1))
        for key in out:
            assert _bits(one[key], out[key][f:f + 1]), (key, f)
    assert _lib.torch_ops() is not None
    before = ops.COUNTERS["ctypes_launches"]
    monkeypatch.setattr(_lib, "_torch_ops", None)
    via_ctypes = _device(case)
    assert ops.COUNTERS["ctypes_launches"] > before
    _same_bits(out, via_ctypes)
