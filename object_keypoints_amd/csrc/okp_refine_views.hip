// Pose refinement of a rig's objects against every camera's bearings (okp_rig_bearings, okp_refine_pose_views; contract in include/okp.h).
// okp_object_pose fits a rig's pose to FUSED points, confidence-weighted means of two-view triangulations that carry the depth noise of a
// short baseline; the peaks those points came from do not.  okp_rig_bearings collects them, per object and table slot, as one bearing per
// camera; okp_refine_pose_views minimises the reprojection error of the object model in all cameras at once, from the fitted pose.
//
//   okp_rig_bearings_kernel        one workgroup of 1024 per object (a rig of 32 pairs has 16 x 32 (slot, pair) items: 32 per wave).  Phase 1, a
//                                  wave per (slot, pair): the slot's cluster is the j-th set bit
//                                  of a ballot over the type's clusters, the pair's member of it a ballot over the pair's left peaks; the two
//                                  peak indices go to LDS.  Phase 2, a lane per (slot, camera): undistort the peak, store the bearing - or
//                                  NaN, so every word of the table is written, once, with no atomics.
//   okp_refine_pose_views_kernel   one wave per object.  With Vp the power of two that holds the V views the wave is G = 64 / Vp groups of Vp
//                                  lanes: lane (g, v) is camera v and takes the slots g, g + G, g + 2 G, ... - a rig of 4 pairs (Vp = 8) has
//                                  eight groups and walks a five-point model in ONE pass, a table of 64 views has one group and walks it
//                                  slot by slot.  The lane keeps its row of `views`, its bearings and their model rows in registers over the
//                                  whole iteration.  Per iterate it adds the terms of its own slots in ascending order, then one
//                                  xor-butterfly over the 64 lanes makes the sums of H, g and the cost - after it every lane holds the
//                                  same bits - and every lane solves the same 6 x 6 system (refine_step), so nothing is broadcast.  The
//                                  loop over a lane's slots is unrolled to the 16 a model can have; a pass in which no lane's slot has a
//                                  model row is skipped on a scalar branch.  A template on where the lane's row of `views` lies: one
//                                  table for every object (okp_refine_pose_views), or one per object (okp_refine_pose_views_each: the
//                                  sliding window of csrc/okp_window.hip, whose views are the ticks of each track's own ring).
//   okp_refine_pose_views_robust_kernel   the same wave, lanes, registers, butterfly and solve under a Huber loss (okp_refine_pose_views_robust):
//                                  a weight per observation from the current iterate's residuals, the robust cost where the plain kernel has
//                                  its cost and the plain cost in a sum of its own, the inliers counted by ballot, and after the status is
//                                  known a pass in which every lane writes the weights of its own (slot, view) entries.  A sibling, not a
//                                  further template flag: the two plain instances stay the code they are.  Two bodies, because a merged
//                                  one, or bodies built from more shared blocks than csrc/okp_pose_math.h's pose load (plain kernel) and
//                                  `information` writer (both), changed the instances' instructions and their time (docs/EXPERIMENTS.md);
//                                  the launch parameters, the argument checks and the launcher of the four entry points of this file are shared.
//   PRIOR instances (okp_refine_pose_views_weighted, okp_rig_bearings_weighted; contract in include/okp.h): a template flag on the two
//                                  refinement kernels - the lane keeps the priors of its observations in registers, 1.0 where it has none,
//                                  and the factor scales the first j of every product (plain) or the Huber weight, so with all priors
//                                  1.0 the bits are the instance's without the flag - and on the bearings kernel, whose phase 2 then also
//                                  writes every entry's prior.  Under `if constexpr`: the instances without the flag are the code they were.
// fp64, no atomics, no host wait; the summation order is fixed, so the bits are the same on every run.
#include "okp_pose_math.h"           // PoseTypes, pose_types, ViewsParams, load_pose, refine_step, view_term, huber_weight, write_information

#pragma clang fp contract(off)

namespace {

#define OKP_BEARINGS_THREADS 1024

struct BearingsParams {
  const int32_t* count; const float* xyc; const int32_t* match; const int32_t* member; const int32_t* object; const int32_t* n_fused;
  const okp_stereo_pair* table; int32_t n_table;
  int32_t n_pairs, cap, cap_f;
  PoseTypes types;
  double* obs;
  double* prior; double conf_ref, conf_floor;    // the PRIOR instance's (okp_rig_bearings_weighted); last, so the other offsets stay
};

// PRIOR: phase 2 also writes every entry's prior from the peak's confidence (okp_rig_bearings_weighted); the plain instance is the code it was
template <bool PRIOR>
__global__ __launch_bounds__(OKP_BEARINGS_THREADS) void okp_rig_bearings_kernel(const BearingsParams p) {
  __shared__ int32_t peak[OKP_POSE_MAX_POINTS][2 * OKP_RIG_MAX_PAIRS];      // [s][v]: the peak of camera v that slot s saw, or -1
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = p.types.S, K = p.types.K, P = p.n_pairs, V = 2 * P, cap = p.cap, cap_f = p.cap_f;
  const bool live = o < min(p.n_fused[0], cap_f);
  for (int e = tid; e < S * V; e += OKP_BEARINGS_THREADS) peak[e / V][e - (e / V) * V] = -1;
  __syncthreads();
  if (live) {                                                     // (block-uniform)
    for (int item = wave; item < S * P; item += OKP_BEARINGS_THREADS / 64) {              // (wave-uniform)
      const int s = item / P, pair = item - s * P;
      int k = 0;
      while (k + 1 < K && s >= p.types.base[k + 1]) ++k;
      const int j = s - p.types.base[k];
      int cluster = o;                                            // type 0: the object's own centre cluster
      if (k >= 1) {
        const int n = min(p.n_fused[k], cap_f);
        unsigned long long mine = __ballot(lane < n && p.object[k * cap_f + lane] == o);
        for (int q = 0; q < j; ++q) mine &= mine - 1ull;          // the j-th cluster of the object, in cluster order
        cluster = mine ? __ffsll((long long)mine) - 1 : -1;
      }
      if (cluster < 0) continue;
      const int ml = 2 * pair * K + k, mr = ml + K;
      const int nl = min(p.count[ml], cap), nr = min(p.count[mr], cap);
      const int32_t* mem = p.member + ((size_t)pair * K + k) * cap;
      int found = -1;
      for (int i0 = 0; i0 < nl && found < 0; i0 += 64) {
        const int i = i0 + lane;
        const unsigned long long hit = __ballot(i < nl && mem[i] == cluster);
        if (hit) found = i0 + __ffsll((long long)hit) - 1;
      }
      if (found < 0) continue;
      const int right = p.match[((size_t)pair * K + k) * cap + found];
      if (right < 0 || right >= nr) continue;                     // (no member of a cluster is unmatched: a table the fusion did not write)
      if (lane == 0) { peak[s][2 * pair] = found; peak[s][2 * pair + 1] = right; }
    }
  }
  __syncthreads();
  const double nan = __builtin_nan("");
  for (int e = tid; e < S * V; e += OKP_BEARINGS_THREADS) {
    const int s = e / V, v = e - s * V;
    const int idx = peak[s][v];
    double bx = nan, by = nan;
    [[maybe_unused]] double a = nan;
    if (idx >= 0) {
      int k = 0;
      while (k + 1 < K && s >= p.types.base[k + 1]) ++k;
      const okp_stereo_pair& entry = p.table[p.n_table == 1 ? 0 : (v >> 1)];
      const okp_camera cam = (v & 1) ? entry.right : entry.left;
      const float* src = p.xyc + (((size_t)v * K + k) * cap + idx) * 3;
      double xu, yu;
      okp_undistort_point(cam, (double)src[0], (double)src[1], xu, yu);
      bx = (xu - cam.cx) / cam.fx;
      by = (yu - cam.cy) / cam.fy;
      if constexpr (PRIOR) {                                      // comparisons and one division; a NaN confidence falls to the floor
        const double c = (double)src[2];
        a = c >= p.conf_ref ? 1.0 : ((c > p.conf_floor ? c : p.conf_floor) / p.conf_ref);
        if (bx != bx && by != by) a = nan;
      }
    }
    double* dst = p.obs + ((size_t)o * S * V + e) * 2;
    dst[0] = bx; dst[1] = by;
    if constexpr (PRIOR) p.prior[(size_t)o * S * V + e] = a;
  }
}

// The sums over the wave's 64 lanes (H, g and the cost: the depth sums of the layout are not used here)
__device__ __forceinline__ void views_butterfly(double (&acc)[OKP_REFINE_SUMS]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] += __shfl_xor(acc[i], off);
}

// EACH: `views` holds one table of V rows per object (okp_refine_pose_views_each) instead of one for all; the only line that differs is the
// address of the lane's row, so the shared-table instance is the code it was
// PRIOR: every observation's squared residual is scaled by its prior (okp_refine_pose_views_weighted): the lane keeps the priors of its slots
// in registers and scales its Jacobian rows by them; under `if constexpr`, so the instances without it are the code they were
template <bool EACH, bool PRIOR>
__global__ __launch_bounds__(64) void okp_refine_pose_views_kernel(const ViewsParams P) {
  const int lane = threadIdx.x;
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];                               // (wave-uniform, like everything that is not a lane's own view)
  const int S = P.S, V = P.V;
  const int G = 64 >> P.vshift, grp = lane >> P.vshift, cam = lane & ((1 << P.vshift) - 1);
  const int passes = (S + G - 1) / G;                             // slots per lane: slot grp + G i in pass i
  const bool view = cam < V;
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  double R[9], t[3];
  const bool pose_finite = load_pose(P.pose, oi, R, t);
  // this lane's camera: [R_v | t_v] and k_v = (fx_v, fy_v) / sigma_px (the lanes past V: an identity that observes nothing)
  double rv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tv[3] = {0.0, 0.0, 0.0}, kx = 1.0, ky = 1.0;
  if (view) {
    const double* row = P.views + (EACH ? oi * (size_t)V * 14 : (size_t)0) + (size_t)cam * 14;
#pragma unroll
    for (int i = 0; i < 3; ++i) { rv[3 * i + 0] = row[4 * i + 0]; rv[3 * i + 1] = row[4 * i + 1]; rv[3 * i + 2] = row[4 * i + 2]; tv[i] = row[4 * i + 3]; }
    kx = row[12] / P.sigma_px; ky = row[13] / P.sigma_px;
  }
  // the object's bearings and model rows, slot by slot
  double ou[OKP_POSE_MAX_POINTS], ov[OKP_POSE_MAX_POINTS], m[OKP_POSE_MAX_POINTS][3];
  [[maybe_unused]] double pr[PRIOR ? OKP_POSE_MAX_POINTS : 1];    // the priors of this lane's observations (1.0 where it has none)
  unsigned seen = 0u, rows = 0u;                                  // bit i: this lane observed its slot of pass i; some lane's slot of pass i has a model row
  int n_obs = 0, n_rows = 0;
  bool bad = false;
  unsigned long long first = 0ull;                                // the first lane of every group
  for (int g = 0; g < G; ++g) first |= 1ull << (g << P.vshift);
#pragma unroll
  for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
    ou[i] = 0.0; ov[i] = 0.0; m[i][0] = 0.0; m[i][1] = 0.0; m[i][2] = 0.0;
    if constexpr (PRIOR) pr[i] = 1.0;
    if (i < passes) {                                             // (wave-uniform)
      const int s = grp + G * i;
      const bool slot = live && s < S;
      const int a = slot ? P.assignment[oi * S + s] : -1;
      const bool row = a >= 0 && a < S;
      double u = nan, v = nan;
      if (slot && view) {
        const double* e = P.obs + ((oi * S + s) * V + cam) * 2;
        u = e[0]; v = e[1];
      }
      bad = bad || ((u != u) != (v != v)) || fabs(u) == inf || fabs(v) == inf;
      const bool mine = row && finite64(u) && finite64(v);
      if constexpr (PRIOR) {
        if (mine) {                                               // (a prior is read, and judged, only where there is an observation)
          const double a = P.prior[(oi * S + s) * V + cam];
          bad = bad || !(a > 0.0 && a < inf);
          pr[i] = a;
        }
      }
      unsigned long long who = __ballot(mine);
      n_obs += __popcll(who);
      for (int sh = 1; sh < (1 << P.vshift); sh <<= 1) who |= who >> sh;          // a group's first lane: some lane of the group observed the slot
      n_rows += __popcll(who & first);
      if (mine) { ou[i] = u; ov[i] = v; seen |= 1u << i; }
      if (row) { m[i][0] = P.model[a * 3 + 0]; m[i][1] = P.model[a * 3 + 1]; m[i][2] = P.model[a * 3 + 2]; }
      if (__ballot(row) != 0ull) rows |= 1u << i;
    }
  }
  const bool any_bad = __ballot(bad) != 0ull;
  int status = (!live || !pose_finite || any_bad || n_rows < 3) ? OKP_REFINE_SKIPPED : 0;

  double acc[OKP_REFINE_SUMS];
  double J0 = nan;
  if (status == 0) {                                              // (a skipped object has nothing to iterate on; its outputs do not depend on it)
    for (int k = 0;; ++k) {
#pragma unroll
      for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] = 0.0;
      bool behind = false;
#pragma unroll
      for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {             // (s: the pass; the lane's slot of it)
        if (!((rows >> s) & 1u)) continue;                        // (wave-uniform)
        const bool mine = (seen >> s) & 1u;
        const double p0 = (R[0] * m[s][0] + R[1] * m[s][1]) + R[2] * m[s][2], p1 = (R[3] * m[s][0] + R[4] * m[s][1]) + R[5] * m[s][2],
                     p2 = (R[6] * m[s][0] + R[7] * m[s][1]) + R[8] * m[s][2];
        const double X0 = p0 + t[0], X1 = p1 + t[1], X2 = p2 + t[2];
        const double q0 = ((rv[0] * X0 + rv[1] * X1) + rv[2] * X2) + tv[0], q1 = ((rv[3] * X0 + rv[4] * X1) + rv[5] * X2) + tv[1],
                     q2 = ((rv[6] * X0 + rv[7] * X1) + rv[8] * X2) + tv[2];
        behind = behind || (mine && q2 <= 0.0);
        const double iz = 1.0 / q2, xn = q0 * iz, yn = q1 * iz;
        const double au0 = kx * iz, au2 = -(au0 * xn), av1 = ky * iz, av2 = -(av1 * yn);
        // b = R_v^T a, the gradient in the table's frame; a Jacobian row is (p x b, b)
        const double bu0 = rv[0] * au0 + rv[6] * au2, bu1 = rv[1] * au0 + rv[7] * au2, bu2 = rv[2] * au0 + rv[8] * au2;
        const double bv0 = rv[3] * av1 + rv[6] * av2, bv1 = rv[4] * av1 + rv[7] * av2, bv2 = rv[5] * av1 + rv[8] * av2;
        double e[2] = {kx * (xn - ou[s]), ky * (yn - ov[s])};
        double j[2][6] = {{p1 * bu2 - p2 * bu1, p2 * bu0 - p0 * bu2, p0 * bu1 - p1 * bu0, bu0, bu1, bu2},
                          {p1 * bv2 - p2 * bv1, p2 * bv0 - p0 * bv2, p0 * bv1 - p1 * bv0, bv0, bv1, bv2}};
        if (!mine) {
          e[0] = 0.0; e[1] = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) { j[0][c] = 0.0; j[1][c] = 0.0; }
        }
        if constexpr (PRIOR) {                                    // a j in the place of the first j of every product: 1.0 gives the bits below
          const double a = pr[s];
          double aj[2][6];
#pragma unroll
          for (int c = 0; c < 6; ++c) { aj[0][c] = a * j[0][c]; aj[1][c] = a * j[1][c]; }
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { acc[idx] += aj[0][r] * j[0][c] + aj[1][r] * j[1][c]; ++idx; }
#pragma unroll
          for (int r = 0; r < 6; ++r) acc[21 + r] += aj[0][r] * e[0] + aj[1][r] * e[1];
          acc[27] += a * (e[0] * e[0] + e[1] * e[1]);
        } else {
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { acc[idx] += j[0][r] * j[0][c] + j[1][r] * j[1][c]; ++idx; }
#pragma unroll
          for (int r = 0; r < 6; ++r) acc[21 + r] += j[0][r] * e[0] + j[1][r] * e[1];
          acc[27] += e[0] * e[0] + e[1] * e[1];
        }
      }
      if (status == 0 && __ballot(behind) != 0ull) status = OKP_REFINE_BEHIND;
      views_butterfly(acc);
      if (k == 0) J0 = acc[27];
      if (k == P.iters) break;                                    // acc holds the sums at the final iterate
      const bool singular = refine_step(acc, P.damping, R, t);
      if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
    }
    const double J1 = acc[27];
    if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_obs)) status = OKP_REFINE_REJECTED;
  }

  // outputs: every word is written by every call, by the object's first lane
  if (lane != 0) return;
  double* pose_out = P.pose_out + oi * 12;
  double* fit = P.fit + oi * 2;
  double* info = P.information + oi * 36;
  const bool ok = status == 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = R[3 * i + 0]; pose_out[4 * i + 1] = R[3 * i + 1]; pose_out[4 * i + 2] = R[3 * i + 2]; pose_out[4 * i + 3] = t[i]; }
  } else if (live) {                                              // the input pose, bit for bit (NaN payloads included)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pose_out);
    unsigned long long bits[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) bits[i] = src[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = bits[i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_out[i] = nan;
  }
  fit[0] = ok ? sqrt(J0 / n_obs) * P.sigma_px : nan;
  fit[1] = ok ? sqrt(acc[27] / n_obs) * P.sigma_px : nan;
  write_information(acc, ok, info);
  P.n_obs[oi] = n_obs;
  P.status[oi] = status;
}

// ---- the robust sibling (okp_refine_pose_views_robust): the same wave, lanes and sums with a Huber weight per observation (IRLS) ----

// H, g, the robust cost (slot 27, where the plain kernel keeps its cost) and the plain cost (slot 28)
__device__ __forceinline__ void robust_butterfly(double (&acc)[OKP_REFINE_SUMS]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < 29; ++i) acc[i] += __shfl_xor(acc[i], off);
}

template <bool EACH, bool PRIOR>
__global__ __launch_bounds__(64) void okp_refine_pose_views_robust_kernel(const ViewsParams P) {
  const int lane = threadIdx.x;
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];
  const int S = P.S, V = P.V;
  const int G = 64 >> P.vshift, grp = lane >> P.vshift, cam = lane & ((1 << P.vshift) - 1);
  const int passes = (S + G - 1) / G;
  const bool view = cam < V;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const double c = P.c, c2 = P.c2, two_c = 2.0 * P.c;

  double R[9], t[3];
  bool pose_finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* row = P.pose + oi * 12 + 4 * i;
    R[3 * i + 0] = row[0]; R[3 * i + 1] = row[1]; R[3 * i + 2] = row[2]; t[i] = row[3];
    pose_finite = pose_finite && finite64(row[0]) && finite64(row[1]) && finite64(row[2]) && finite64(row[3]);
  }
  double rv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tv[3] = {0.0, 0.0, 0.0}, kx = 1.0, ky = 1.0;
  if (view) {
    const double* row = P.views + (EACH ? oi * (size_t)V * 14 : (size_t)0) + (size_t)cam * 14;
#pragma unroll
    for (int i = 0; i < 3; ++i) { rv[3 * i + 0] = row[4 * i + 0]; rv[3 * i + 1] = row[4 * i + 1]; rv[3 * i + 2] = row[4 * i + 2]; tv[i] = row[4 * i + 3]; }
    kx = row[12] / P.sigma_px; ky = row[13] / P.sigma_px;
  }
  double ou[OKP_POSE_MAX_POINTS], ov[OKP_POSE_MAX_POINTS], m[OKP_POSE_MAX_POINTS][3];
  [[maybe_unused]] double pr[PRIOR ? OKP_POSE_MAX_POINTS : 1];    // the priors of this lane's observations (1.0 where it has none)
  unsigned seen = 0u, rows = 0u;
  int n_obs = 0, n_rows = 0;
  bool bad = false;
  unsigned long long first = 0ull;
  for (int g = 0; g < G; ++g) first |= 1ull << (g << P.vshift);
#pragma unroll
  for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
    ou[i] = 0.0; ov[i] = 0.0; m[i][0] = 0.0; m[i][1] = 0.0; m[i][2] = 0.0;
    if constexpr (PRIOR) pr[i] = 1.0;
    if (i < passes) {
      const int s = grp + G * i;
      const bool slot = live && s < S;
      const int a = slot ? P.assignment[oi * S + s] : -1;
      const bool row = a >= 0 && a < S;
      double u = nan, v = nan;
      if (slot && view) {
        const double* e = P.obs + ((oi * S + s) * V + cam) * 2;
        u = e[0]; v = e[1];
      }
      bad = bad || ((u != u) != (v != v)) || fabs(u) == inf || fabs(v) == inf;
      const bool mine = row && finite64(u) && finite64(v);
      if constexpr (PRIOR) {
        if (mine) {                                               // (a prior is read, and judged, only where there is an observation)
          const double a = P.prior[(oi * S + s) * V + cam];
          bad = bad || !(a > 0.0 && a < inf);
          pr[i] = a;
        }
      }
      unsigned long long who = __ballot(mine);
      n_obs += __popcll(who);
      for (int sh = 1; sh < (1 << P.vshift); sh <<= 1) who |= who >> sh;
      n_rows += __popcll(who & first);
      if (mine) { ou[i] = u; ov[i] = v; seen |= 1u << i; }
      if (row) { m[i][0] = P.model[a * 3 + 0]; m[i][1] = P.model[a * 3 + 1]; m[i][2] = P.model[a * 3 + 2]; }
      if (__ballot(row) != 0ull) rows |= 1u << i;
    }
  }
  const bool any_bad = __ballot(bad) != 0ull;
  int status = (!live || !pose_finite || any_bad || n_rows < 3) ? OKP_REFINE_SKIPPED : 0;

  double acc[OKP_REFINE_SUMS];
  double J0 = nan, Pl0 = nan;
  int n_inlier = 0;
  if (status == 0) {
    for (int k = 0;; ++k) {
#pragma unroll
      for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] = 0.0;
      bool behind = false;
      n_inlier = 0;
#pragma unroll
      for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {
        if (!((rows >> s) & 1u)) continue;                        // (wave-uniform)
        const bool mine = (seen >> s) & 1u;
        const ViewTerm T = view_term(R, t, rv, tv, kx, ky, m[s][0], m[s][1], m[s][2], ou[s], ov[s]);
        behind = behind || (mine && T.qz <= 0.0);
        double e[2] = {T.e0, T.e1};
        double j[2][6] = {{T.p1 * T.bu2 - T.p2 * T.bu1, T.p2 * T.bu0 - T.p0 * T.bu2, T.p0 * T.bu1 - T.p1 * T.bu0, T.bu0, T.bu1, T.bu2},
                          {T.p1 * T.bv2 - T.p2 * T.bv1, T.p2 * T.bv0 - T.p0 * T.bv2, T.p0 * T.bv1 - T.p1 * T.bv0, T.bv0, T.bv1, T.bv2}};
        if (!mine) {
          e[0] = 0.0; e[1] = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) { j[0][q] = 0.0; j[1][q] = 0.0; }
        }
        double sq = e[0] * e[0] + e[1] * e[1];                   // (0 for a lane without the observation: an inlier that adds nothing)
        if constexpr (PRIOR) sq = pr[s] * sq;                     // the whitened residual: the Huber rule is applied to it
        const bool inlier = sq <= c2;
        double w = huber_weight(sq, c, c2);
        const double rho = inlier ? sq : two_c * sqrt(sq) - c2;
        n_inlier += __popcll(__ballot(mine && inlier));
        if constexpr (PRIOR) w = pr[s] * w;                       // the terms' weight is a w_h (the weight OUTPUT stays w_h)
        double wj[2][6];
#pragma unroll
        for (int q = 0; q < 6; ++q) { wj[0][q] = w * j[0][q]; wj[1][q] = w * j[1][q]; }
        int idx = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int q = r; q < 6; ++q) { acc[idx] += wj[0][r] * j[0][q] + wj[1][r] * j[1][q]; ++idx; }
#pragma unroll
        for (int r = 0; r < 6; ++r) acc[21 + r] += wj[0][r] * e[0] + wj[1][r] * e[1];
        acc[27] += rho;
        acc[28] += sq;
      }
      if (status == 0 && __ballot(behind) != 0ull) status = OKP_REFINE_BEHIND;
      robust_butterfly(acc);
      if (k == 0) { J0 = acc[27]; Pl0 = acc[28]; }
      if (k == P.iters) break;
      const bool singular = refine_step(acc, P.damping, R, t);
      if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
    }
    const double J1 = acc[27];
    if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_obs)) status = OKP_REFINE_REJECTED;
  }
  const bool ok = status == 0;

  // the weights: a lane writes the words of its own (slot, view) entries - the lanes with cam < V and the passes cover the table - from the
  // final iterate (R, t), after the status is known
  if (view) {
    double* wrow = P.weight + oi * (size_t)S * V + cam;
#pragma unroll
    for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
      const int s = grp + G * i;
      if (i < passes && s < S) {
        double w = nan;
        if (ok && ((seen >> i) & 1u)) {
          const ViewTerm T = view_term(R, t, rv, tv, kx, ky, m[i][0], m[i][1], m[i][2], ou[i], ov[i]);
          double sq = T.e0 * T.e0 + T.e1 * T.e1;
          if constexpr (PRIOR) sq = pr[i] * sq;
          w = huber_weight(sq, c, c2);
        }
        wrow[(size_t)s * V] = w;
      }
    }
  }

  // the other outputs: every word is written by every call, by the object's first lane
  if (lane != 0) return;
  double* pose_out = P.pose_out + oi * 12;
  double* fit = P.fit + oi * 4;
  double* info = P.information + oi * 36;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = R[3 * i + 0]; pose_out[4 * i + 1] = R[3 * i + 1]; pose_out[4 * i + 2] = R[3 * i + 2]; pose_out[4 * i + 3] = t[i]; }
  } else if (live) {                                              // the input pose, bit for bit (NaN payloads included)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pose_out);
    unsigned long long bits[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) bits[i] = src[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = bits[i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose_out[i] = nan;
  }
  fit[0] = ok ? sqrt(Pl0 / n_obs) * P.sigma_px : nan;
  fit[1] = ok ? sqrt(acc[28] / n_obs) * P.sigma_px : nan;
  fit[2] = ok ? sqrt(J0 / n_obs) * P.sigma_px : nan;
  fit[3] = ok ? sqrt(acc[27] / n_obs) * P.sigma_px : nan;
  write_information(acc, ok, info);
  P.n_obs[oi] = n_obs;
  P.n_inlier[oi] = ok ? n_inlier : 0;
  P.status[oi] = status;
}

}  // namespace

// okp_rig_bearings and okp_rig_bearings_weighted: one kernel, the second instance also writes the priors
static int rig_bearings_launch(const char* fn, const char* what, const int32_t* count, const float* xyc, const int32_t* match, const int32_t* member,
                               const int32_t* object, const int32_t* n_fused, const okp_stereo_pair* table, int32_t n_table, int32_t n_pairs, int32_t K,
                               int32_t cap, int32_t cap_f, const int32_t* type_count, bool weighted, double conf_ref, double conf_floor, double* obs,
                               double* prior, void* stream) {
  BearingsParams p = {};
  if (n_pairs < 1 || n_pairs > OKP_RIG_MAX_PAIRS) { okp_set_error("%s: n_pairs = %d outside [1, %d]", fn, n_pairs, OKP_RIG_MAX_PAIRS); return OKP_EINVAL; }
  int rc = pose_types(fn, type_count, K, OKP_RIG_MAX_TYPES, p.types, nullptr);
  if (rc) return rc;
  if (cap < 1 || cap > 256) { okp_set_error("%s: cap = %d outside [1, 256]", fn, cap); return OKP_EINVAL; }
  if (cap_f < 1 || cap_f > OKP_RIG_MAX_FUSED) { okp_set_error("%s: cap_f = %d outside [1, %d]", fn, cap_f, OKP_RIG_MAX_FUSED); return OKP_EINVAL; }
  if (n_table < 1) { okp_set_error("%s: n_table = %d; a calibration table holds at least one stereo pair", fn, n_table); return OKP_EINVAL; }
  if (n_table > 1 && n_table < n_pairs) { okp_set_error("%s: n_table = %d calibrations for n_pairs = %d pairs (one entry serves every pair)", fn, n_table, n_pairs); return OKP_EINVAL; }
  if (weighted && !(conf_ref > 0.0 && conf_ref < __builtin_inf())) {
    okp_set_error("%s: conf_ref = %g must be positive and finite (the confidence from which a peak has the full weight)", fn, conf_ref);
    return OKP_EINVAL;
  }
  if (weighted && !(conf_floor > 0.0 && conf_floor <= conf_ref)) {
    okp_set_error("%s: conf_floor = %g outside (0, conf_ref = %g]", fn, conf_floor, conf_ref);
    return OKP_EINVAL;
  }
  const struct { const void* ptr; const char* name; } required[] = {
      {count, "count"}, {xyc, "xyc"}, {match, "match"}, {member, "member"}, {object, "object"}, {n_fused, "n_fused"}, {table, "table"}, {obs, "obs"}};
  for (const auto& r : required)
    if (!r.ptr) { okp_set_error("%s: null %s", fn, r.name); return OKP_EINVAL; }
  if (weighted && !prior) { okp_set_error("%s: null prior", fn); return OKP_EINVAL; }
  p.count = count; p.xyc = xyc; p.match = match; p.member = member; p.object = object; p.n_fused = n_fused;
  p.table = table; p.n_table = n_table; p.n_pairs = n_pairs; p.cap = cap; p.cap_f = cap_f; p.obs = obs;
  p.prior = prior; p.conf_ref = conf_ref; p.conf_floor = conf_floor;
  if (weighted) hipLaunchKernelGGL(okp_rig_bearings_kernel<true>, dim3(cap_f), dim3(OKP_BEARINGS_THREADS), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(okp_rig_bearings_kernel<false>, dim3(cap_f), dim3(OKP_BEARINGS_THREADS), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), what);
}

extern "C" int okp_rig_bearings(const int32_t* count, const float* xyc, const int32_t* match, const int32_t* member, const int32_t* object,
                                const int32_t* n_fused, const okp_stereo_pair* table, int32_t n_table, int32_t n_pairs, int32_t K, int32_t cap,
                                int32_t cap_f, const int32_t* type_count, double* obs, void* stream) {
  return rig_bearings_launch("okp_rig_bearings", "okp_rig_bearings launch", count, xyc, match, member, object, n_fused, table, n_table, n_pairs, K, cap, cap_f,
                             type_count, false, 0.0, 0.0, obs, nullptr, stream);
}

extern "C" int okp_rig_bearings_weighted(const int32_t* count, const float* xyc, const int32_t* match, const int32_t* member, const int32_t* object,
                                         const int32_t* n_fused, const okp_stereo_pair* table, int32_t n_table, int32_t n_pairs, int32_t K, int32_t cap,
                                         int32_t cap_f, const int32_t* type_count, double conf_ref, double conf_floor, double* obs, double* prior,
                                         void* stream) {
  return rig_bearings_launch("okp_rig_bearings_weighted", "okp_rig_bearings_weighted launch", count, xyc, match, member, object, n_fused, table, n_table, n_pairs,
                             K, cap, cap_f, type_count, true, conf_ref, conf_floor, obs, prior, stream);
}

// The four one-wave entry points behind one launcher: plain or Huber, one views table for every object or one per object, with priors or without.
// huber_px and views_each are null for the entry points that have none; weighted: okp_refine_pose_views_weighted's - prior is required, V may
// be refused only beyond the wide limit (above one wave the entry point has handed off already) and huber_px = 0 selects the plain cost
static int refine_views_launch(const char* fn, const char* what, bool weighted, const double* obs, const double* prior, const double* views, const int32_t* views_each,
                               bool each, const double* pose, const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, const double* huber_px,
                               int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs,
                               int32_t* n_inlier, double* weight, double* information, int32_t* status, void* stream) {
  ViewsParams p;
  const int rc = refine_views_params(fn, obs, views, pose, assignment, n_obj, model, sigma_px, huber_px, weighted, views_each, iters, damping, B, max_obj, S, V,
                                     weighted ? OKP_REFINE_WIDE_MAX_VIEWS : OKP_REFINE_MAX_VIEWS, pose_out, fit, n_obs, n_inlier, weight, information, status, p);
  if (rc) return rc;
  if (weighted && !prior) { okp_set_error("%s: null prior", fn); return OKP_EINVAL; }
  p.prior = prior;
  using Kernel = void (*)(const ViewsParams);
  static const Kernel instance[2][2][2] = {          // [PRIOR][Huber][!EACH]: named in the order the file has always emitted them, so its device code stays the same bytes
      {{okp_refine_pose_views_kernel<true, false>, okp_refine_pose_views_kernel<false, false>},
       {okp_refine_pose_views_robust_kernel<true, false>, okp_refine_pose_views_robust_kernel<false, false>}},
      {{okp_refine_pose_views_kernel<true, true>, okp_refine_pose_views_kernel<false, true>},
       {okp_refine_pose_views_robust_kernel<true, true>, okp_refine_pose_views_robust_kernel<false, true>}}};
  const bool robust = huber_px && *huber_px > 0.0;                // (an entry point that does not take 0 as the plain cost has refused it)
  hipLaunchKernelGGL(instance[weighted][robust][!each], dim3((unsigned)((size_t)B * max_obj)), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), what);
}

extern "C" int okp_refine_pose_views(const double* obs, const double* views, const double* pose, const int32_t* assignment, const int32_t* n_obj,
                                     const double* model, double sigma_px, int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S,
                                     int32_t V, double* pose_out, double* fit, int32_t* n_obs, double* information, int32_t* status, void* stream) {
  return refine_views_launch("okp_refine_pose_views", "okp_refine_pose_views launch", false, obs, nullptr, views, nullptr, false, pose, assignment, n_obj, model, sigma_px, nullptr,
                             iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, nullptr, nullptr, information, status, stream);
}

extern "C" int okp_refine_pose_views_each(const double* obs, const double* views, const double* pose, const int32_t* assignment, const int32_t* n_obj,
                                          const double* model, double sigma_px, int32_t iters, double damping, int32_t B, int32_t max_obj, int32_t S,
                                          int32_t V, double* pose_out, double* fit, int32_t* n_obs, double* information, int32_t* status, void* stream) {
  return refine_views_launch("okp_refine_pose_views_each", "okp_refine_pose_views_each launch", false, obs, nullptr, views, nullptr, true, pose, assignment, n_obj, model, sigma_px,
                             nullptr, iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, nullptr, nullptr, information, status, stream);
}

extern "C" int okp_refine_pose_views_robust(const double* obs, const double* views, int32_t views_each, const double* pose, const int32_t* assignment,
                                            const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters, double damping, int32_t B,
                                            int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs, int32_t* n_inlier, double* weight,
                                            double* information, int32_t* status, void* stream) {
  return refine_views_launch("okp_refine_pose_views_robust", "okp_refine_pose_views_robust launch", false, obs, nullptr, views, &views_each, views_each != 0, pose, assignment, n_obj,
                             model, sigma_px, &huber_px, iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
}

// The weighted refinement: up to one wave of views the PRIOR instances of the kernels above, beyond it the wide kernel's (csrc/okp_refine_views_wide.hip)
extern "C" int okp_refine_pose_views_weighted(const double* obs, const double* prior, const double* views, int32_t views_each, const double* pose,
                                              const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters,
                                              double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs,
                                              int32_t* n_inlier, double* weight, double* information, int32_t* status, void* stream) {
  const char* fn = "okp_refine_pose_views_weighted";
  if (V > OKP_REFINE_MAX_VIEWS)
    return okp_refine_views_weighted_wide(fn, obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters, damping, B, max_obj, S, V,
                                          pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
  return refine_views_launch(fn, "okp_refine_pose_views_weighted launch", true, obs, prior, views, &views_each, views_each != 0, pose, assignment, n_obj, model, sigma_px,
                             &huber_px, iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
}
