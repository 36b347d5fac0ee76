"""NumPy / fp64 statement of okp_group_objects, written from the comment in include/okp.h and the reference's ObjectExtraction.__call__ as
oracle/pipeline.py:136-175 restates it - not from the kernel: plain loops, one frame, one peak, one object at a time.  The tests compare
whole output tensors of the device stage with it (tests/test_gpu_group_objects.py) and pin it to the oracle (tests/test_group_objects_args.py).

Besides the six tensors it returns its SMALLEST DECISION MARGIN: the smallest relative gap seen in any comparison that decides an outcome
(nearest centre, the distance gate, the farthest point of the initialisation, the nearest cluster of a Lloyd step, the inertia of two
restarts, the confidence rank that picks the seeds).  A case whose margin is well above the rounding of fp64 has one answer whatever the
order of the sums and whether or not a multiply-add is fused; a case with margin 0 holds an exact tie, which the rules below decide."""
import math

import numpy as np

KM_RESTARTS = 4          # include/okp.h: "seeded by each of the four most confident votes in turn"
KM_ITERS = 32            # include/okp.h: "or after 32 iterations"
KM_VOTES = 64            # include/okp.h: "one lane per vote (the object's first 64)"


class _Margin:
    def __init__(self):
        self.value = math.inf

    def gap(self, a, b):
        """a, b: the two quantities a decision compares (non-negative)."""
        scale = max(abs(a), abs(b))
        self.value = min(self.value, abs(a - b) / scale if scale > 0.0 else 0.0)


def _sq_dist(px, py, cx, cy):
    dx, dy = px - cx, py - cy
    return dx * dx + dy * dy


def reduce_votes(points, conf, want, margin=None):
    """The deterministic k-means of the header: points [(x, y)] fp64 and conf [fp32] of one object's votes for one type in peak order (at
    most KM_VOTES of them), want clusters -> [want][2] fp64 centres (the caller rounds to fp32)."""
    margin = margin or _Margin()
    n = len(points)
    px = [float(p[0]) for p in points]
    py = [float(p[1]) for p in points]
    ranked = sorted(range(n), key=lambda i: (-float(conf[i]), i))            # confidence descending, then peak order
    restarts = min(KM_RESTARTS, n)
    for r in range(restarts):                                                # the ranks that pick the seeds, and the first one left out
        if r + 1 < n:
            margin.gap(float(conf[ranked[r]]), float(conf[ranked[r + 1]]))
    best = None
    for r in range(restarts):
        seed = ranked[r]
        cx, cy = [px[seed]], [py[seed]]
        dmin = [_sq_dist(px[i], py[i], cx[0], cy[0]) for i in range(n)]
        for t in range(1, want):                                             # farthest point from the centres chosen so far, lowest index on a tie
            far = max(range(n), key=lambda i: (dmin[i], -i))
            second = max((dmin[i] for i in range(n) if i != far), default=None)
            if second is not None:
                margin.gap(dmin[far], second)
            cx.append(px[far]); cy.append(py[far])
            dmin = [min(dmin[i], _sq_dist(px[i], py[i], cx[t], cy[t])) for i in range(n)]
        inertia = 0.0
        ax, ay = np.array(px), np.array(py)
        for _ in range(KM_ITERS):
            d = np.stack([_sq_dist(ax, ay, cx[t], cy[t]) for t in range(want)], axis=1)      # [vote][cluster], each entry one fp64 expression
            member = [min(range(want), key=lambda t: (d[i, t], t)) for i in range(n)]         # the nearest centre, the lower cluster on a tie
            nearest = [float(d[i, member[i]]) for i in range(n)]
            if want > 1:
                for i in range(n):
                    margin.gap(nearest[i], float(np.delete(d[i], member[i]).min()))
            inertia = math.fsum(nearest)
            moved = False
            for t in range(want):
                mine = [i for i in range(n) if member[i] == t]
                if not mine:
                    continue                                                 # an empty cluster keeps its centre
                nx, ny = math.fsum(px[i] for i in mine) / len(mine), math.fsum(py[i] for i in mine) / len(mine)
                moved = moved or nx != cx[t] or ny != cy[t]
                cx[t], cy[t] = nx, ny
            if not moved:
                break
        run = (inertia, list(zip(cx, cy)))
        if best is None:
            best = run
        else:
            if sorted(run[1]) != sorted(best[1]):                            # (two runs that end in the same clusters: nothing is decided)
                margin.gap(run[0], best[0])
            if run[0] < best[0]:                                             # the least inertia, the earlier seed on a tie
                best = run
    return np.array(best[1], dtype=np.float64)


def group_objects(count, xyc, centers, type_count, max_dist, max_obj, max_sel):
    """count [N,K] int32, xyc [N,K,cap,3] fp32, centers [N,K-1,2,H,W] fp32 -> dict of n_obj [N], sel [N,max_obj,K-1,max_sel], n_votes
    [N,max_obj,K-1], assign [N,K,cap] (int32), pred [N,K,cap,2] (fp64), reduced [N,max_obj,K-1,max_sel,2] (fp32), and "margin"."""
    count = np.asarray(count, dtype=np.int32)
    xyc = np.asarray(xyc, dtype=np.float32)
    centers = np.asarray(centers, dtype=np.float32)
    N, K, cap, _ = xyc.shape
    H, W = centers.shape[3:]
    assert count.shape == (N, K) and centers.shape[:3] == (N, K - 1, 2) and len(type_count) == K - 1
    gate = float(np.float32(max_dist))
    n_obj = np.zeros(N, np.int32)
    sel = np.full((N, max_obj, K - 1, max_sel), -1, np.int32)
    n_votes = np.zeros((N, max_obj, K - 1), np.int32)
    assign = np.full((N, K, cap), -1, np.int32)
    pred = np.zeros((N, K, cap, 2), np.float64)
    reduced = np.full((N, max_obj, K - 1, max_sel, 2), np.nan, np.float32)
    margin = _Margin()
    for f in range(N):
        nobj = min(int(count[f, 0]), cap, max_obj)
        n_obj[f] = nobj
        if nobj == 0:
            continue                                                         # no centre, no vote: every output keeps its unused value
        ox = xyc[f, 0, :nobj, 0].astype(np.float64)
        oy = xyc[f, 0, :nobj, 1].astype(np.float64)
        for k in range(1, K):
            want = int(type_count[k - 1])
            votes = [[] for _ in range(nobj)]                                # per object: peak indices in peak order
            for j in range(min(int(count[f, k]), cap)):
                x, y, c = xyc[f, k, j]
                xi = min(max(int(np.rint(x)), 0), W - 1)                     # round half to even, then clip
                yi = min(max(int(np.rint(y)), 0), H - 1)
                cx = (xi + 0.5) + float(centers[f, k - 1, 0, yi, xi])
                cy = (yi + 0.5) + float(centers[f, k - 1, 1, yi, xi])
                pred[f, k, j] = (cx, cy)
                if not (math.isfinite(cx) and math.isfinite(cy)):
                    continue                                                 # votes for no object
                d = np.sqrt((ox - cx) * (ox - cx) + (oy - cy) * (oy - cy))
                o = int(np.argmin(d))                                        # the nearest centre, the lower index on a tie
                if d[o] > gate:
                    if math.isfinite(d[o]):
                        margin.gap(d[o], gate)
                    continue
                margin.gap(d[o], gate)
                if nobj > 1:
                    margin.gap(d[o], float(np.delete(d, o).min()))
                assign[f, k, j] = o
                votes[o].append(j)
            for o in range(nobj):
                v = votes[o]
                n_votes[f, o, k - 1] = len(v)
                if not v:
                    continue
                if want == 1:
                    sel[f, o, k - 1, 0] = max(v, key=lambda j: (xyc[f, k, j, 2], -j))      # the most confident, the first on a tie
                    continue
                sel[f, o, k - 1, :min(len(v), max_sel)] = v[:max_sel]
                if len(v) > want and want <= max_sel:
                    first = v[:KM_VOTES]
                    c = reduce_votes([xyc[f, k, j, :2].astype(np.float64) for j in first], [xyc[f, k, j, 2] for j in first], want, margin)
                    reduced[f, o, k - 1, :want] = c.astype(np.float32)
    return {"n_obj": n_obj, "sel": sel, "n_votes": n_votes, "assign": assign, "pred": pred, "reduced": reduced, "margin": margin.value}
