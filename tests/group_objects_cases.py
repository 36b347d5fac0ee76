"""Inputs for okp_group_objects built directly (count, xyc, centers: no network, no NMS in front), shared by the CPU test that checks their
input conditions (tests/test_group_objects_args.py) and the GPU test that runs them (tests/test_gpu_group_objects.py).

A case is a dict: count [N,K] int32, xyc [N,K,cap,3] fp32, centers [N,K-1,2,H,W] fp32, type_count, max_dist, max_obj, max_sel, and
`exact`: True for the hand-made integer cases, whose every operation is exact with or without a fused multiply-add (they may hold exact
ties; `reduced` is compared bit for bit), False for cases on real-valued coordinates, which must have a decision margin above MARGIN."""
import numpy as np

MARGIN = 1e-9
FAR = ("far",)                     # a vote for nobody: its predicted centre is beyond the gate of every centre


class Frame:
    """One frame under construction.  A peak sits at a pixel of its own, so that its centre-offset value is its own too."""

    def __init__(self, rng, K, cap, H, W, centres, stored=None):
        self.rng, self.K, self.cap, self.H, self.W = rng, K, cap, H, W
        self.count = np.zeros(K, np.int32)
        self.xyc = np.zeros((K, cap, 3), np.float32)
        self.centers = np.zeros((K - 1, 2, H, W), np.float32)
        self.centres = np.asarray(centres, dtype=np.float32).reshape(-1, 2)
        n = len(self.centres) if stored is None else stored
        self.count[0] = len(self.centres)
        self.xyc[0, :n, :2] = self.centres[:n]
        self.xyc[0, :n, 2] = 1.0 + 0.01 * np.arange(n)
        # a background that no test may lean on: offsets that send a stray lookup far away, different in the x and the y plane
        self.centers[:, 0] = 300.0 + rng.uniform(0, 50, (K - 1, H, W)).astype(np.float32)
        self.centers[:, 1] = -400.0 - rng.uniform(0, 50, (K - 1, H, W)).astype(np.float32)
        self.used = [set() for _ in range(K)]

    def _pixel(self, k, near=None, radius=4):
        for _ in range(10000):
            if near is None:
                xi, yi = int(self.rng.integers(0, self.W)), int(self.rng.integers(0, self.H))
            else:
                xi = int(np.clip(round(near[0] + self.rng.uniform(-radius, radius)), 0, self.W - 1))
                yi = int(np.clip(round(near[1] + self.rng.uniform(-radius, radius)), 0, self.H - 1))
            if (xi, yi) not in self.used[k]:
                self.used[k].add((xi, yi))
                return xi, yi
        raise AssertionError("no free pixel")

    def peak(self, k, vote, conf, near=None, spread=6.0, radius=4):
        """Append a peak to map k: vote = object index (its predicted centre falls within `spread` px of that centre), FAR, or an explicit
        (x, y) predicted centre.  near: put the peak's pixel around this position (the k-means clusters peak positions, not predictions)."""
        j = int(self.count[k])
        self.count[k] += 1
        if j >= self.cap:
            return                                                         # found by the NMS, not stored
        xi, yi = self._pixel(k, near, radius)
        fx, fy = self.rng.uniform(-0.45, 0.45, 2)
        self.xyc[k, j] = (xi + fx, yi + fy, conf)
        if vote is FAR:
            tx, ty = -150.0 - self.rng.uniform(0, 20), -150.0 - self.rng.uniform(0, 20)
        elif isinstance(vote, tuple):
            tx, ty = vote
        else:
            r, a = spread * np.sqrt(self.rng.uniform(0.01, 1.0)), self.rng.uniform(0, 2 * np.pi)
            tx, ty = self.centres[vote, 0] + r * np.cos(a), self.centres[vote, 1] + r * np.sin(a)
        self.centers[k - 1, 0, yi, xi] = tx - (xi + 0.5)
        self.centers[k - 1, 1, yi, xi] = ty - (yi + 0.5)
        return j


def pack(frames, type_count, max_obj, max_sel, max_dist=20.0, exact=False):
    return dict(count=np.stack([f.count for f in frames]), xyc=np.stack([f.xyc for f in frames]), centers=np.stack([f.centers for f in frames]),
                type_count=list(type_count), max_dist=max_dist, max_obj=max_obj, max_sel=max_sel, exact=exact)


def grid_centres(rng, n, H, W, pitch=16.0):
    """n centres on a jittered grid of `pitch` px: at least pitch - 2 px apart, so a vote within 6 px of one is nearest to it."""
    cols = int(W // pitch)
    assert n <= cols * int(H // pitch)
    cells = rng.permutation(cols * int(H // pitch))[:n]
    return [((c % cols + 0.5) * pitch + rng.uniform(-1, 1), (c // cols + 0.5) * pitch + rng.uniform(-1, 1)) for c in cells]


def confidences(rng, n):
    """n distinct fp32 confidences in [0.5, 1.5), at least 1 / (2 n) apart."""
    return (rng.permutation(n) / n + 0.5 + rng.uniform(0, 0.4 / n, n)).astype(np.float32)


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------------

def votes_across_lane_batches():
    """cap = 256, four batches of 64 peaks per type.  Object 0 receives votes in batches 0 and 2 only.  Type 1 (count 1): object 1's top
    confidence appears in batch 0 (peak 5) and again, equal, in batch 3 (peak 200): the first wins.  Type 2 (count 1): the batch-3 peak is
    strictly more confident: the later wins.  Type 3 (count 3, max_sel 8): slots are numbered in peak order across the batches."""
    rng = np.random.default_rng(101)
    f = Frame(rng, 4, 256, 64, 64, [(12.0, 12.0), (50.0, 14.0), (30.0, 50.0)])
    conf = confidences(rng, 3 * 256).reshape(3, 256) * np.float32(0.5)                       # all below 0.8
    for k in (1, 2, 3):
        for j in range(256):
            batch = j // 64
            if k < 3 and j in (5, 200):
                f.peak(k, 1, np.float32(0.9) if (k == 1 or j == 5) else np.float32(0.95))
            elif k == 3 and j in (60, 63, 130, 131, 190):
                f.peak(k, 0, conf[k - 1, j], near=[(8, 8), (16, 8), (12, 18)][j % 3], radius=2)
            elif k == 3 and j in (0, 1, 64, 255):
                f.peak(k, 1, conf[k - 1, j], near=[(46, 10), (54, 12), (50, 20)][j % 3], radius=2)
            elif batch in (0, 2) and j % 7 == 3 and k < 3:
                f.peak(k, 0, conf[k - 1, j])
            elif j % 5 == 0:
                f.peak(k, FAR, conf[k - 1, j])
            else:
                f.peak(k, 1 + (j % 2) if k < 3 else FAR, conf[k - 1, j])
    return pack([f], [1, 1, 3], max_obj=4, max_sel=8)


def more_centres_than_max_obj():
    """count[0] = max_obj + 3: only the first max_obj centres exist.  Peak 0 predicts a centre next to dropped centre 5, 12 px from kept
    centre 3: it goes to 3.  Peak 1 predicts one next to dropped centre 6, more than 20 px from every kept centre: it goes to none."""
    rng = np.random.default_rng(102)
    c = [(10.0, 10.0), (40.0, 10.0), (70.0, 10.0), (100.0, 10.0), (10.0, 60.0), (100.0, 22.0), (64.0, 100.0)]
    f = Frame(rng, 3, 16, 128, 128, c)
    for vote in ((100.5, 21.5), (64.5, 99.0), 0, 1, 2, 3, 3, 0):
        f.peak(1, vote, 0.7)
    conf = confidences(rng, 6)
    for j, vote in enumerate(((100.0, 21.0), (63.0, 101.0), 3, 3, 1, (10.5, 59.0))):
        f.peak(2, vote, conf[j])
    return pack([f], [1, 2], max_obj=4, max_sel=4)


def more_peaks_than_cap():
    """count[k] = cap + 5 on a key-point map (and count[0] = cap + 2 with max_obj above cap: n_obj = cap): only the stored peaks vote."""
    rng = np.random.default_rng(103)
    f = Frame(rng, 3, 7, 64, 64, grid_centres(rng, 9, 64, 64), stored=7)
    conf = confidences(rng, 24)
    for j in range(12):
        f.peak(1, j % 7, conf[j])
        f.peak(2, j % 3, conf[12 + j], near=f.centres[j % 3])
    assert f.count.tolist() == [9, 12, 12]
    return pack([f], [1, 2], max_obj=16, max_sel=4)


def no_centre():
    """count[0] = 0 with peaks on the other maps (frame 0), next to an ordinary frame: everything of frame 0 is at its unused value."""
    rng = np.random.default_rng(104)
    empty = Frame(rng, 3, 8, 64, 64, [])
    full = Frame(rng, 3, 8, 64, 64, [(20.0, 20.0), (44.0, 40.0)])
    conf = confidences(rng, 16)
    for fr in (empty, full):
        for j in range(5):
            fr.peak(1, (20.0 + j, 20.0), conf[j])
            fr.peak(2, (44.0, 40.0 - j), conf[8 + j])
    return pack([empty, full], [1, 3], max_obj=4, max_sel=4)


def every_lane_an_object():
    """max_obj = 64 with 64 centres: every lane keeps an object's state; 200 votes per type spread over all of them."""
    rng = np.random.default_rng(105)
    f = Frame(rng, 3, 256, 128, 128, grid_centres(rng, 64, 128, 128))
    conf = confidences(rng, 400)
    for j in range(200):
        f.peak(1, int(rng.integers(0, 64)) if j % 9 else FAR, conf[j])
        o = int(rng.integers(0, 64))
        f.peak(2, o, conf[200 + j], near=f.centres[o], radius=6)
    return pack([f], [1, 2], max_obj=64, max_sel=2)


def one_object_slot():
    """max_obj = 1 with three centre peaks: the first is the only object; votes nearest to the others go to it if within the gate, else to none."""
    rng = np.random.default_rng(106)
    f = Frame(rng, 3, 16, 64, 64, [(20.0, 20.0), (30.0, 26.0), (55.0, 55.0)])
    conf = confidences(rng, 20)
    for j, vote in enumerate((0, 1, 2, 1, 0, 2, FAR, 1)):
        f.peak(1, vote, conf[j])
        f.peak(2, vote, conf[10 + j], near=[(18, 18), (26, 24), (22, 30)][j % 3], radius=2)
    return pack([f], [1, 3], max_obj=1, max_sel=4)


def gate_and_ties_on_integer_geometry():
    """Three frames of exact arithmetic (every coordinate, offset and product a small dyadic number; sqrt of a perfect square).
    Frame 0: one centre at (20, 20).  Peak 0 predicts (32, 36): distance exactly 20 = max_dist, kept.  Peak 1 predicts the same with the next
    fp32 offset above in y: dropped.  Peak 2 is at exactly the centre (distance 0).
    Frame 1: centres (20, 20) and (26, 28).  Peak 0 predicts (23, 24), distance exactly 5 from both: the lower index.  Peak 1 predicts
    (23, 24) from the other side of the map with a lower confidence; type 1 keeps one: peak 0.  Peaks 2, 3 are nearer to centre 1.
    Frame 2: peak coordinates exactly x.5: 10.5 -> pixel 10 and 11.5 -> pixel 12 (half to even), in x and in y; -3.2 and W + 7 (and H + 7)
    are clipped to the border pixels.  Every pixel involved holds an offset of its own, so the vote tells the pixel."""
    K, cap, H, W = 3, 8, 48, 64
    count = np.zeros((3, K), np.int32)
    xyc = np.zeros((3, K, cap, 3), np.float32)
    centers = np.full((3, K - 1, 2, H, W), 500.0, np.float32)

    def aim(f, k, pixel, target):
        centers[f, k - 1, 0, pixel[1], pixel[0]] = np.float32(target[0] - (pixel[0] + 0.5))
        centers[f, k - 1, 1, pixel[1], pixel[0]] = np.float32(target[1] - (pixel[1] + 0.5))

    def put(f, k, j, x, y, conf, target, pixel):
        xyc[f, k, j] = (x, y, conf)
        count[f, k] = max(count[f, k], j + 1)
        aim(f, k, pixel, target)

    # frame 0: the gate
    count[0, 0] = 1
    xyc[0, 0, 0] = (20.0, 20.0, 1.0)
    put(0, 1, 0, 30.0, 30.0, 0.5, (32.0, 36.0), (30, 30))
    put(0, 1, 1, 40.0, 30.25, 0.75, (32.0, 36.0), (40, 30))
    centers[0, 0, 1, 30, 40] = np.nextafter(np.float32(5.5), np.float32(np.inf))
    put(0, 1, 2, 20.25, 19.75, 0.25, (20.0, 20.0), (20, 20))
    put(0, 2, 0, 5.0, 5.0, 0.5, (8.0, 4.0), (5, 5))                      # (-12, -16) from the centre: 20 again
    put(0, 2, 1, 6.0, 6.0, 0.5, (20.0, 40.0), (6, 6))                    # (0, 20): kept
    put(0, 2, 2, 7.0, 7.0, 0.5, (20.0, 40.5), (7, 7))                    # 20.5: dropped
    # frame 1: the bisector
    count[1, 0] = 2
    xyc[1, 0, 0] = (20.0, 20.0, 1.0)
    xyc[1, 0, 1] = (26.0, 28.0, 0.9)
    put(1, 1, 0, 3.0, 3.0, 0.75, (23.0, 24.0), (3, 3))
    put(1, 1, 1, 60.0, 40.0, 0.5, (23.0, 24.0), (60, 40))
    put(1, 1, 2, 33.0, 9.0, 0.875, (24.0, 25.0), (33, 9))
    put(1, 1, 3, 34.0, 9.0, 0.875, (26.0, 28.0), (34, 9))               # the same confidence as peak 2: the first of the two is kept
    put(1, 2, 0, 12.0, 12.0, 0.5, (23.0, 24.0), (12, 12))
    put(1, 2, 1, 13.0, 12.0, 0.5, (23.0, 24.0), (13, 12))
    put(1, 2, 2, 14.0, 12.0, 0.5, (23.0, 24.0), (14, 12))
    # frame 2: rounding and clipping; centres 0 .. 3 far apart, each pixel votes for a centre of its own
    count[2, 0] = 4
    cs = [(8.0, 8.0), (56.0, 8.0), (8.0, 40.0), (56.0, 40.0)]
    for o, c in enumerate(cs):
        xyc[2, 0, o] = (c[0], c[1], 1.0)
    for x in (10, 11, 12):
        for y in (10, 11, 12):
            o = (x == 11) + 2 * (y == 11)                                 # pixel column 11 or row 11: another centre
            aim(2, 1, (x, y), (cs[o][0] + 1.0, cs[o][1] - 2.0))
    put(2, 1, 0, 10.5, 10.5, 0.5, (9.0, 6.0), (10, 10))
    put(2, 1, 1, 11.5, 10.5, 0.625, (9.0, 6.0), (12, 10))
    put(2, 1, 2, 10.5, 11.5, 0.75, (9.0, 6.0), (10, 12))
    put(2, 1, 3, 11.5, 11.5, 0.875, (9.0, 6.0), (12, 12))
    put(2, 2, 0, -3.2, 20.0, 0.5, (56.0, 10.0), (0, 20))
    put(2, 2, 1, W + 7.0, 20.0, 0.5, (8.0, 42.0), (W - 1, 20))
    put(2, 2, 2, 30.0, -3.2, 0.5, (58.0, 40.0), (30, 0))
    put(2, 2, 3, 30.0, H + 7.0, 0.5, (8.0, 10.0), (30, H - 1))
    put(2, 2, 4, -3.2, H + 7.0, 0.5, (56.0, 38.0), (0, H - 1))
    return dict(count=count, xyc=xyc, centers=centers, type_count=[1, 2], max_dist=20.0, max_obj=4, max_sel=4, exact=True)


def maps_that_are_not_square(H, W):
    """H != W, offsets that differ between the x and the y plane: a swapped plane or pitch changes every vote."""
    rng = np.random.default_rng(H * 1000 + W)
    frames = []
    for _ in range(3):
        n = 3
        cs = [(W * (o + 0.5) / n + rng.uniform(-2, 2), H / 2 + rng.uniform(-1, 1)) for o in range(n)] if H < 16 else grid_centres(rng, n, H, W)
        f = Frame(rng, 3, 64, H, W, cs)
        conf = confidences(rng, 100)
        for j in range(40):
            f.peak(1, j % n if j % 6 else FAR, conf[j])
            f.peak(2, j % n, conf[50 + j], near=f.centres[j % n], radius=5)
        frames.append(f)
    return pack(frames, [1, 3], max_obj=8, max_sel=4)


def eight_maps(max_sel):
    """K = 8 with type_count [1, 3, 1, 2, 8, 1, 4]: at max_sel = 8 every multi-instance type with surplus votes is reduced; at max_sel = 4 the
    type with eight instances keeps its first four votes and gets no reduction."""
    rng = np.random.default_rng(108)
    tc = [1, 3, 1, 2, 8, 1, 4]
    frames = []
    for _ in range(2):
        f = Frame(rng, 8, 64, 96, 96, grid_centres(rng, 5, 96, 96))
        for k in range(1, 8):
            conf = confidences(rng, 64)
            for j in range(30 + 4 * k):
                o = j % 5 if j % 11 else FAR
                f.peak(k, o, conf[j], near=None if o is FAR else f.centres[o], radius=6)
        frames.append(f)
    return pack(frames, tc, max_obj=8, max_sel=max_sel)


def non_finite_offsets():
    """A NaN, a +inf and a -inf in the centre map under three peaks (in the x plane, the y plane, and both): assign -1, pred holds the value;
    the other peaks of the frame vote as if those were not there."""
    rng = np.random.default_rng(109)
    f = Frame(rng, 3, 16, 64, 64, [(20.0, 20.0), (44.0, 40.0)])
    conf = confidences(rng, 32)
    for j in range(10):
        f.peak(1, j % 2, conf[j])
        f.peak(2, j % 2, conf[16 + j], near=f.centres[j % 2])
    for k, j, plane, v in ((1, 2, 0, np.nan), (1, 5, 1, np.inf), (2, 0, 0, -np.inf), (2, 3, 1, np.nan), (2, 3, 0, np.inf)):
        xi, yi = int(np.rint(f.xyc[k, j, 0])), int(np.rint(f.xyc[k, j, 1]))
        f.centers[k - 1, plane, yi, xi] = v
    return pack([f], [1, 3], max_obj=4, max_sel=4)


def seventy_votes_for_one_object():
    """One object with 70 votes for a 3-instance type: the first 64 in peak order are reduced.  60 of them sit in batch 0 and 10 in batch 1
    (peaks 64 .. 73), so the compaction of batch 1 would pass lane 63; the six votes past the 64th are in a cluster of their own corner,
    which would move a centre if they were counted."""
    rng = np.random.default_rng(110)
    f = Frame(rng, 2, 128, 64, 64, [(32.0, 32.0)])
    conf = confidences(rng, 100)
    blobs = [(20, 22), (44, 24), (30, 46)]
    for j in range(100):
        if j < 60 or 64 <= j < 74:
            nth = j if j < 60 else j - 4
            f.peak(1, 0, conf[j], near=blobs[j % 3] if nth < 64 else (58, 58), radius=5 if nth < 64 else 3)
        else:
            f.peak(1, FAR, conf[j])
    return pack([f], [3], max_obj=2, max_sel=4)


def three_surplus_objects():
    """64 objects; objects 2, 31 and 63 each receive more votes than the type has instances (the others at most as many)."""
    rng = np.random.default_rng(111)
    f = Frame(rng, 3, 256, 128, 128, grid_centres(rng, 64, 128, 128))
    conf = confidences(rng, 512)
    plan = [o for o in range(64) for _ in range(2)] + [2] * 5 + [31] * 9 + [63] * 4
    for j, o in enumerate(rng.permutation(plan)):
        f.peak(1, int(o), conf[j], near=f.centres[o] + [(-4, -3), (4, -2), (0, 5)][j % 3], radius=2)
    for j in range(70):
        f.peak(2, int(rng.integers(0, 64)), conf[256 + j])
    return pack([f], [3, 1], max_obj=64, max_sel=4)


def surplus_across_a_batch_boundary():
    """A surplus object whose six votes are peaks 61 .. 66: the last three lanes of batch 0 and the first three of batch 1."""
    rng = np.random.default_rng(112)
    f = Frame(rng, 2, 128, 64, 64, [(20.0, 20.0), (44.0, 44.0)])
    conf = confidences(rng, 100)
    for j in range(90):
        if 61 <= j <= 66:
            f.peak(1, 1, conf[j], near=[(40, 40), (50, 42), (44, 52)][j % 3], radius=2)
        else:
            f.peak(1, 0 if j % 30 == 7 else FAR, conf[j])
    return pack([f], [3], max_obj=4, max_sel=4)


HAND_MADE = {
    "votes_across_lane_batches": votes_across_lane_batches,
    "more_centres_than_max_obj": more_centres_than_max_obj,
    "more_peaks_than_cap": more_peaks_than_cap,
    "no_centre": no_centre,
    "every_lane_an_object": every_lane_an_object,
    "one_object_slot": one_object_slot,
    "gate_and_ties_on_integer_geometry": gate_and_ties_on_integer_geometry,
    "map_48x80": lambda: maps_that_are_not_square(48, 80),
    "map_5x700": lambda: maps_that_are_not_square(5, 700),
    "eight_maps_max_sel_8": lambda: eight_maps(8),
    "eight_maps_max_sel_4": lambda: eight_maps(4),
    "non_finite_offsets": non_finite_offsets,
    "seventy_votes_for_one_object": seventy_votes_for_one_object,
    "three_surplus_objects": three_surplus_objects,
    "surplus_across_a_batch_boundary": surplus_across_a_batch_boundary,
}


# ---- seeded random batches --------------------------------------------------------------------------------------------------------------

CAPS = (1, 7, 64, 65, 130, 256)
# (frames, seed); cap = CAPS[seed % 6].  Every seed listed passes the margin condition (tests/test_group_objects_args.py); seed 5 is the
# cap-256 batch with max_sel = 1, seed 23 the one with max_sel = 4 and several hundred reductions.
RANDOM_BATCHES = [(64, seed) for seed in (0, 1, 2, 3, 4, 5, 23)] + [(1, seed) for seed in (6, 7, 8, 9, 10, 29)]


def random_batch(n, seed):
    """n frames that share K, cap, type_count, max_obj and max_sel (one launch), each with counts of its own: between nothing and a few more
    than cap peaks per map, between no and a few more than max_obj centres."""
    rng = np.random.default_rng(7000 + seed)
    cap = CAPS[seed % 6]
    K = int(rng.integers(2, 9))
    max_sel = int(rng.choice([1, 2, 4, 8]))
    max_obj = int(rng.choice([1, 3, 16, 64]))
    type_count = [int(rng.choice([1, 1, 2, 3, 5])) for _ in range(K - 1)]
    if max_sel >= 2:
        type_count[-1] = min(int(rng.choice([2, 3])), max_sel)               # (one type at least that the reduction can serve)
    H, W = (64, 64) if max_obj <= 16 else (128, 128)
    frames = []
    for _ in range(n):
        n_c = int(rng.integers(0, min(max_obj, 12) + 3))
        f = Frame(rng, K, cap, H, W, grid_centres(rng, n_c, H, W), stored=min(n_c, cap))
        live = min(n_c, cap, max_obj)
        for k in range(1, K):
            npk = int((cap + 4) * rng.uniform(0, 1) ** 2)
            conf = confidences(rng, max(npk, 1))
            for j in range(npk):
                if n_c == 0 or rng.uniform() < 0.15:
                    f.peak(k, FAR, conf[j])
                else:
                    o = int(rng.integers(0, n_c))                            # (a centre beyond max_obj / cap: its votes go to a neighbour or to none)
                    f.peak(k, o, conf[j], near=f.centres[o] if o < live and npk < 40 * n_c else None, radius=7)
        frames.append(f)
    return pack(frames, type_count, max_obj=max_obj, max_sel=max_sel)
