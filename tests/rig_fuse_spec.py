"""NumPy statement of okp_rig_fuse, written from the specification in include/okp.h (transform, cluster each type across the pairs, fuse,
group around the centres), not from the kernel: plain loops, one candidate at a time.  The tests compare the device stage with it."""
import numpy as np

FUSE_OVERFLOW = 4


def rig_fuse(points, poses, type_count, merge_radius, object_radius, cap_f, overflow_in=0):
    """points [P,K,cap,4] float64 (NaN confidence = empty slot), poses [P,12] float64 (T_BL[p][:3] row-major), type_count: K-1 ints
    -> dict of fused [K,cap_f,4], n_fused [K], views [K,cap_f], object [K,cap_f], member [P,K,cap], n_obj, overflow."""
    points = np.asarray(points, dtype=np.float64)
    P, K, cap, _ = points.shape
    T = np.asarray(poses, dtype=np.float64).reshape(P, 3, 4)
    fused = np.full((K, cap_f, 4), np.nan)
    n_fused = np.zeros(K, np.int32)
    views = np.zeros((K, cap_f), np.int32)
    obj = np.full((K, cap_f), -1, np.int32)
    member = np.full((P, K, cap), -1, np.int32)
    overflow = int(overflow_in)
    for k in range(K):
        # 1. transform every candidate; 2. order: confidence descending, then pair, then slot
        cand = [(-points[p, k, s, 3], p, s) for p in range(P) for s in range(cap) if not np.isnan(points[p, k, s, 3])]
        cand.sort()
        clusters = []                                  # [seed, pairs, sum c, sum c X, seed confidence]
        for neg_c, p, s in cand:
            c = -neg_c
            X = T[p, :, :3] @ points[p, k, s, :3] + T[p, :, 3]
            for j, cl in enumerate(clusters):
                d = X - cl["seed"]
                if p not in cl["pairs"] and d @ d <= merge_radius * merge_radius:
                    break
            else:
                if len(clusters) == cap_f:
                    overflow |= FUSE_OVERFLOW
                    continue
                j = len(clusters)
                clusters.append({"seed": X, "pairs": [], "w": 0.0, "wx": np.zeros(3), "c": c})
            cl = clusters[j]
            cl["pairs"].append(p)
            cl["w"] = cl["w"] + c                      # 3. sums in join order
            cl["wx"] = cl["wx"] + c * X
            member[p, k, s] = j
        n_fused[k] = len(clusters)
        for j, cl in enumerate(clusters):
            fused[k, j, :3] = cl["wx"] / cl["w"]
            fused[k, j, 3] = cl["c"]
            views[k, j] = np.array(sum(1 << p for p in cl["pairs"]), dtype=np.uint32).astype(np.int32)
    # 4. group
    n_obj = int(n_fused[0])
    obj[0, :n_obj] = np.arange(n_obj)
    for k in range(1, K):
        nearest = np.full(n_fused[k], -1)
        for j in range(n_fused[k]):
            best = None
            for o in range(n_obj):
                d = fused[k, j, :3] - fused[0, o, :3]
                d2 = d @ d
                if best is None or d2 < best:          # a tie stays with the lower index
                    best, nearest[j] = d2, o
            if best is None or not best <= object_radius * object_radius:
                nearest[j] = -1
        for o in range(n_obj):
            mine = [j for j in range(n_fused[k]) if nearest[j] == o]
            mine.sort(key=lambda j: (-bin(int(views[k, j]) & 0xffffffff).count("1"), -fused[k, j, 3], j))
            for j in mine[:type_count[k - 1]]:
                obj[k, j] = o
    return {"fused": fused, "n_fused": n_fused, "views": views, "object": obj, "member": member, "n_obj": n_obj, "overflow": overflow}


def rounding_bound(points, poses, n_terms):
    """Bound on |device - spec| for a fused coordinate, from the formats alone (u = 2^-53).  A transformed coordinate is a sum of four
    terms (three products and t): computed with or without fused multiply-adds its error is at most 4 u M (to first order), with
    M = max over candidates and axes of sum_j |R_ij| |X_j| + |t_i|, which also bounds |X_B|.  The weighted mean of n members with
    positive weights: each product c_i X_i adds u, the n-term sums n u each in numerator and denominator, the division u; numerator
    errors are relative to sum c_i |X_B,i| <= (sum c_i) M, so the quotient is within (4 + 1 + 2 n + 1) u M of the exact mean of the exact
    transforms.  Device and spec each stay within that of the exact value, hence twice it between them; a factor 2 covers the
    second-order terms."""
    points = np.asarray(points, dtype=np.float64)
    P = points.shape[0]
    T = np.abs(np.asarray(poses, dtype=np.float64).reshape(P, 3, 4))
    X = np.abs(np.nan_to_num(points[..., :3], nan=0.0))                        # [P,K,cap,3]
    M = (np.einsum("pij,pkcj->pkci", T[:, :, :3], X) + T[:, None, None, :, 3]).max()
    return 2.0 * 2.0 * (2 * n_terms + 6) * 2.0 ** -53 * M
