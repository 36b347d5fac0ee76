// The views refinement beyond one wave (okp_refine_pose_views_wide; contract in include/okp.h).  okp_refine_pose_views and its siblings
// (csrc/okp_refine_views.hip) give every view a lane of ONE wave, so a table holds at most 64 views; the window of a rig - 2 P cameras x W
// ticks - has up to 512.  Here an object is a WORKGROUP of ceil(V / 64) waves.
//
//   okp_refine_pose_views_wide_kernel   lane l of wave w is view 64 w + l and walks the S slots one per pass, as the one-wave kernel does at
//                                  64 views.  Its row of `views` and its bearings stay in registers over the iteration; the model rows are
//                                  the same for every lane and lie in LDS, and the iterate (R, t) - the same bits in every lane - in scalar
//                                  registers: at 512 threads a lane has 256 registers, and neither instance uses scratch.  Per iterate a lane adds its own slots' terms in ascending order,
//                                  the xor-butterfly makes the wave's sums, lane 0 of each wave stores them to LDS, and after a barrier every
//                                  lane adds the waves' partials in ascending wave order, starting from wave 0's - so every lane of the
//                                  workgroup holds the same bits and solves the same 6 x 6 system (refine_step); nothing is broadcast.  With
//                                  one wave (V <= 64) the sums are that wave's butterfly: at 32 < V <= 64 the bits are the one-wave kernels'.
//                                  A template on the loss: plain (okp_refine_pose_views' cost) or Huber (okp_refine_pose_views_robust's).
//                                  Of the blocks csrc/okp_pose_math.h shares, the kernel takes the writer of `information`; the others
//                                  changed its instructions, and built from them the plain instance took 2 % longer at 512 views
//                                  (docs/EXPERIMENTS.md).  The argument checks are the shared ones (refine_views_params).
//
// Barriers.  A barrier under a branch that two waves of a workgroup decide differently hangs the device, so every word that decides control
// flow around a barrier is workgroup-wide BEFORE it is used: whether the object is live, its pose finite and its bearings well-formed, the
// set of observed slots (an OR of per-wave bit masks, not a sum of counts: two waves that see the same slot see ONE row), n_obs, a point
// behind a camera and n_inlier all go through LDS; `singular` comes from refine_step on sums that are the same bits in every lane.  The only
// branch that encloses a barrier is `status == 0` before the loop, made of such words; the loop runs `iters` steps (a kernel argument) in
// every wave, and no thread returns before the last barrier.
// fp64, no atomics, no host wait, contraction off; the summation order is fixed, so the bits are the same on every run.
#include "okp_pose_math.h"           // finite64, view_term, huber_weight, refine_step, write_information, refine_views_params

#pragma clang fp contract(off)

namespace {

#define OKP_WIDE_WAVES (OKP_REFINE_WIDE_MAX_VIEWS / 64)
static_assert(OKP_REFINE_WIDE_MAX_VIEWS % 64 == 0 && OKP_WIDE_WAVES * 64 <= 1024, "whole waves, one workgroup");

// (the kernel's own order of the launch parameters: its scalar loads and spills follow the layout; refine_views_params fills the shared
// ViewsParams and the entry point copies)
struct WideParams {
  const double* obs; const double* views; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, S, V, iters, each;             // each: views holds one table of V rows per object
  double sigma_px, damping;
  double c, c2;                                   // huber_px / sigma_px and its square, formed on the host (the Huber instance)
  double* pose_out; double* fit; int32_t* n_obs; int32_t* n_inlier; double* weight; double* information; int32_t* status;
  const double* prior;                            // [B][max_obj][S][V], the PRIOR instances' (last: the other offsets stay)
};

// x as a scalar: every lane of the workgroup holds the same bits of the iterate (R, t), so the wave's copy can live in scalar registers - the
// 24 vector registers it frees are what keeps the Huber instance out of scratch memory at 256 registers a lane
__device__ __forceinline__ double wave_uniform(double x) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)bits), hi = __builtin_amdgcn_readfirstlane((unsigned)(bits >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// PRIOR: every observation's squared residual is scaled by its prior (okp_refine_pose_views_weighted).  Sixteen more fp64 values a lane do not
// fit its 256 registers, so the object's priors are staged in LDS once, [slot][thread] (64 KB): a lane writes and reads only its own view's
// entries, so they need no barrier, and the address is one register with the slot in the instruction's offset.  The precheck of the priors
// joins the workgroup-wide OR of the bearings' precheck; nothing else that decides control flow depends on them.  Under `if constexpr`: the
// other instances are the code they were
template <bool ROBUST, bool PRIOR>
__global__ __launch_bounds__(OKP_REFINE_WIDE_MAX_VIEWS) void okp_refine_pose_views_wide_kernel(const WideParams P) {
  constexpr int NS = ROBUST ? 29 : 28;            // H, g, the cost (and the plain cost next to the robust one)
  __shared__ double mdl[OKP_POSE_MAX_POINTS][3];  // the model row of every slot (zeros without one)
  __shared__ double part[OKP_WIDE_WAVES][NS];     // the waves' sums of one iterate
  __shared__ unsigned w_seen[OKP_WIDE_WAVES];     // before the loop: bit s - some lane of the wave observed slot s
  __shared__ int w_obs[OKP_WIDE_WAVES], w_skip[OKP_WIDE_WAVES];
  __shared__ int w_behind[OKP_WIDE_WAVES], w_inlier[OKP_WIDE_WAVES];          // per iterate
  [[maybe_unused]] __shared__ double pri[PRIOR ? OKP_POSE_MAX_POINTS : 1][PRIOR ? OKP_REFINE_WIDE_MAX_VIEWS : 1];     // (PRIOR) [s][tid]: 1.0 without an observation
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];
  const int S = P.S, V = P.V;
  const bool view = tid < V;                      // (the lanes past V: an identity that observes nothing)
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
    const double* row = P.views + (P.each ? oi * (size_t)V * 14 : (size_t)0) + (size_t)tid * 14;
#pragma unroll
    for (int i = 0; i < 3; ++i) { rv[3 * i + 0] = row[4 * i + 0]; rv[3 * i + 1] = row[4 * i + 1]; rv[3 * i + 2] = row[4 * i + 2]; tv[i] = row[4 * i + 3]; }
    kx = row[12] / P.sigma_px; ky = row[13] / P.sigma_px;
  }
  // the slots with a model row: the same words for every lane of the workgroup
  unsigned rows = 0u;
#pragma unroll
  for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {
    if (s < S) {
      const int a = live ? P.assignment[oi * S + s] : -1;
      if (a >= 0 && a < S) rows |= 1u << s;
    }
  }
  if (tid < S) {
    const int a = live ? P.assignment[oi * S + tid] : -1;
    const bool row = a >= 0 && a < S;
    mdl[tid][0] = row ? P.model[a * 3 + 0] : 0.0; mdl[tid][1] = row ? P.model[a * 3 + 1] : 0.0; mdl[tid][2] = row ? P.model[a * 3 + 2] : 0.0;
  }
  // this view's bearings, slot by slot
  double ou[OKP_POSE_MAX_POINTS], ov[OKP_POSE_MAX_POINTS];
  unsigned seen = 0u, seen_w = 0u;                // bit s: this lane / some lane of this wave observed slot s
  int n_obs_w = 0;
  bool bad = false;
#pragma unroll
  for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {
    ou[s] = 0.0; ov[s] = 0.0;
    if (s < S) {                                  // (a kernel argument)
      double u = nan, v = nan;
      if (live && view) {
        const double* e = P.obs + ((oi * S + s) * V + tid) * 2;
        u = e[0]; v = e[1];
      }
      bad = bad || ((u != u) != (v != v)) || fabs(u) == inf || fabs(v) == inf;
      const bool mine = ((rows >> s) & 1u) && finite64(u) && finite64(v);
      if constexpr (PRIOR) {
        double a = 1.0;
        if (mine) {                               // (a prior is read, and judged, only where there is an observation)
          a = P.prior[(oi * S + s) * V + tid];
          bad = bad || !(a > 0.0 && a < inf);
        }
        pri[s][tid] = a;
      }
      const unsigned long long who = __ballot(mine);
      n_obs_w += __popcll(who);
      if (who != 0ull) seen_w |= 1u << s;
      if (mine) { ou[s] = u; ov[s] = v; seen |= 1u << s; }
    }
  }
  const bool skip_w = !live || !pose_finite || __ballot(bad) != 0ull;
  if (lane == 0) { w_seen[wave] = seen_w; w_obs[wave] = n_obs_w; w_skip[wave] = skip_w ? 1 : 0; }
  __syncthreads();                                // (the model rows, too)
  unsigned seen_all = 0u;
  int n_obs = 0, skip = 0;
  for (int w = 0; w < nw; ++w) { seen_all |= w_seen[w]; n_obs += w_obs[w]; skip |= w_skip[w]; }
  int status = (skip != 0 || __popc(seen_all) < 3) ? OKP_REFINE_SKIPPED : 0;      // (the same words in every lane of the workgroup)

  double acc[OKP_REFINE_SUMS];
  double J0 = nan, Pl0 = nan;
  int n_inlier = 0;
  if (status == 0) {                              // (workgroup-uniform: the barriers below are reached by every wave or by none)
    for (int k = 0;; ++k) {
#pragma unroll
      for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] = 0.0;
      bool behind = false;
      int inlier_w = 0;
#pragma unroll
      for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {
        if (!((rows >> s) & 1u)) continue;        // (workgroup-uniform)
        const bool mine = (seen >> s) & 1u;
        const ViewTerm T = view_term(R, t, rv, tv, kx, ky, mdl[s][0], mdl[s][1], mdl[s][2], ou[s], ov[s]);
        behind = behind || (mine && T.qz <= 0.0);
        double e[2] = {T.e0, T.e1};
        double j[2][6] = {{T.p1 * T.bu2 - T.p2 * T.bu1, T.p2 * T.bu0 - T.p0 * T.bu2, T.p0 * T.bu1 - T.p1 * T.bu0, T.bu0, T.bu1, T.bu2},
                          {T.p1 * T.bv2 - T.p2 * T.bv1, T.p2 * T.bv0 - T.p0 * T.bv2, T.p0 * T.bv1 - T.p1 * T.bv0, T.bv0, T.bv1, T.bv2}};
        if (!mine) {
          e[0] = 0.0; e[1] = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) { j[0][q] = 0.0; j[1][q] = 0.0; }
        }
        [[maybe_unused]] double a = 1.0;
        if constexpr (PRIOR) a = pri[s][tid];     // (1.0 for a lane without the observation: its terms are zeros)
        if constexpr (ROBUST) {
          double sq = e[0] * e[0] + e[1] * e[1];                 // (0 for a lane without the observation: an inlier that adds nothing)
          if constexpr (PRIOR) sq = a * sq;                      // the whitened residual: the Huber rule is applied to it
          const bool inlier = sq <= c2;
          double w = huber_weight(sq, c, c2);
          const double rho = inlier ? sq : two_c * sqrt(sq) - c2;
          inlier_w += __popcll(__ballot(mine && inlier));
          if constexpr (PRIOR) {                                 // the terms' weight is a w_h (the weight OUTPUT stays w_h); the prior is read
            __asm__ volatile("" ::: "memory");                   // again, not held over the square root and the division: three registers
            w = pri[s][tid] * w;                                 // that this instance does not have (tests/test_refine_weighted_args.py holds the build's report to no scratch)
          }
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {           // (w j of one row at a time: the products of the one-wave kernel, fewer live registers)
            const double wj0 = w * j[0][r], wj1 = w * j[1][r];
#pragma unroll
            for (int q = r; q < 6; ++q) { acc[idx] += wj0 * j[0][q] + wj1 * j[1][q]; ++idx; }
            acc[21 + r] += wj0 * e[0] + wj1 * e[1];
          }
          acc[27] += rho;
          acc[28] += sq;
        } else if constexpr (PRIOR) {             // a j in the place of the first j of every product: 1.0 gives the bits of the plain instance
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            const double aj0 = a * j[0][r], aj1 = a * j[1][r];
#pragma unroll
            for (int q = r; q < 6; ++q) { acc[idx] += aj0 * j[0][q] + aj1 * j[1][q]; ++idx; }
            acc[21 + r] += aj0 * e[0] + aj1 * e[1];
          }
          acc[27] += a * (e[0] * e[0] + e[1] * e[1]);
        } else {
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = r; q < 6; ++q) { acc[idx] += j[0][r] * j[0][q] + j[1][r] * j[1][q]; ++idx; }
#pragma unroll
          for (int r = 0; r < 6; ++r) acc[21 + r] += j[0][r] * e[0] + j[1][r] * e[1];
          acc[27] += e[0] * e[0] + e[1] * e[1];
        }
      }
      const bool behind_w = __ballot(behind) != 0ull;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] += __shfl_xor(acc[i], off);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) part[wave][i] = acc[i];
        w_behind[wave] = behind_w ? 1 : 0;
        w_inlier[wave] = inlier_w;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NS; ++i) acc[i] = part[0][i];
      int any_behind = w_behind[0];
      n_inlier = w_inlier[0];
      for (int w = 1; w < nw; ++w) {              // ascending waves, from wave 0's sums: the same bits in every lane
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] += part[w][i];
        any_behind |= w_behind[w];
        n_inlier += w_inlier[w];
      }
      __syncthreads();                            // (the next iterate overwrites the partials)
      if (status == 0 && any_behind != 0) status = OKP_REFINE_BEHIND;
      if (k == 0) { J0 = acc[27]; Pl0 = acc[28]; }
      if (k == P.iters) break;                    // acc holds the sums at the final iterate
      const bool singular = refine_step(acc, P.damping, R, t);
      if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = wave_uniform(R[i]);
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = wave_uniform(t[i]);
    }
    const double J1 = acc[27];
    if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_obs)) status = OKP_REFINE_REJECTED;
  }
  const bool ok = status == 0;

  // the weights: a lane writes the words of its own view, from the final iterate, after the status is known
  if constexpr (ROBUST) {
    if (view) {
      double* wrow = P.weight + oi * (size_t)S * V + tid;
#pragma unroll
      for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {
        if (s < S) {
          double w = nan;
          if (ok && ((seen >> s) & 1u)) {
            const ViewTerm T = view_term(R, t, rv, tv, kx, ky, mdl[s][0], mdl[s][1], mdl[s][2], ou[s], ov[s]);
            double sq = T.e0 * T.e0 + T.e1 * T.e1;
            if constexpr (PRIOR) sq = pri[s][tid] * sq;
            w = huber_weight(sq, c, c2);
          }
          wrow[(size_t)s * V] = w;
        }
      }
    }
  }

  // the other outputs: every word is written by every call, by the object's first lane
  if (tid != 0) return;
  double* pose_out = P.pose_out + oi * 12;
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
  if constexpr (ROBUST) {
    double* fit = P.fit + oi * 4;
    fit[0] = ok ? sqrt(Pl0 / n_obs) * P.sigma_px : nan;
    fit[1] = ok ? sqrt(acc[28] / n_obs) * P.sigma_px : nan;
    fit[2] = ok ? sqrt(J0 / n_obs) * P.sigma_px : nan;
    fit[3] = ok ? sqrt(acc[27] / n_obs) * P.sigma_px : nan;
    P.n_inlier[oi] = ok ? n_inlier : 0;
  } else {
    double* fit = P.fit + oi * 2;
    fit[0] = ok ? sqrt(J0 / n_obs) * P.sigma_px : nan;
    fit[1] = ok ? sqrt(acc[27] / n_obs) * P.sigma_px : nan;
  }
  write_information(acc, ok, info);
  P.n_obs[oi] = n_obs;
  P.status[oi] = status;
}

}  // namespace

// okp_refine_pose_views_wide (prior = null) and, for okp_refine_pose_views_weighted beyond one wave of views, its PRIOR instances
static int wide_launch(const char* fn, const char* what, bool weighted, const double* obs, const double* prior, const double* views, int32_t views_each,
                       const double* pose, const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters,
                       double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs, int32_t* n_inlier,
                       double* weight, double* information, int32_t* status, void* stream) {
  ViewsParams v;
  const int rc = refine_views_params(fn, obs, views, pose, assignment, n_obj, model, sigma_px, &huber_px, true, &views_each, iters, damping, B,
                                     max_obj, S, V, OKP_REFINE_WIDE_MAX_VIEWS, pose_out, fit, n_obs, n_inlier, weight, information, status, v);
  if (rc) return rc;
  if (weighted && !prior) { okp_set_error("%s: null prior", fn); return OKP_EINVAL; }
  WideParams p = {};
  p.obs = v.obs; p.views = v.views; p.pose = v.pose; p.assignment = v.assignment; p.n_obj = v.n_obj; p.model = v.model;
  p.max_obj = v.max_obj; p.S = v.S; p.V = v.V; p.iters = v.iters; p.each = v.each; p.sigma_px = v.sigma_px; p.damping = v.damping; p.c = v.c; p.c2 = v.c2;
  p.pose_out = v.pose_out; p.fit = v.fit; p.n_obs = v.n_obs; p.n_inlier = v.n_inlier; p.weight = v.weight; p.information = v.information; p.status = v.status;
  p.prior = prior;
  const dim3 grid((unsigned)((size_t)B * max_obj)), block(64u * (unsigned)((V + 63) / 64));
  const hipStream_t st = (hipStream_t)stream;
  if (weighted && huber_px > 0.0) hipLaunchKernelGGL((okp_refine_pose_views_wide_kernel<true, true>), grid, block, 0, st, p);
  else if (weighted) hipLaunchKernelGGL((okp_refine_pose_views_wide_kernel<false, true>), grid, block, 0, st, p);
  else if (huber_px > 0.0) hipLaunchKernelGGL((okp_refine_pose_views_wide_kernel<true, false>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((okp_refine_pose_views_wide_kernel<false, false>), grid, block, 0, st, p);
  return okp_check_hip(hipGetLastError(), what);
}

extern "C" int okp_refine_pose_views_wide(const double* obs, const double* views, int32_t views_each, const double* pose, const int32_t* assignment,
                                          const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters, double damping, int32_t B,
                                          int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs, int32_t* n_inlier, double* weight,
                                          double* information, int32_t* status, void* stream) {
  return wide_launch("okp_refine_pose_views_wide", "okp_refine_pose_views_wide launch", false, obs, nullptr, views, views_each, pose, assignment, n_obj, model, sigma_px,
                     huber_px, iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
}

// okp_refine_pose_views_weighted on the wide kernel's PRIOR instances whatever V is: with all priors 1.0 the bits of okp_refine_pose_views_wide
extern "C" int okp_refine_pose_views_weighted_wide(const double* obs, const double* prior, const double* views, int32_t views_each, const double* pose,
                                                   const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters,
                                                   double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs,
                                                   int32_t* n_inlier, double* weight, double* information, int32_t* status, void* stream) {
  return wide_launch("okp_refine_pose_views_weighted_wide", "okp_refine_pose_views_weighted_wide launch", true, obs, prior, views, views_each, pose, assignment, n_obj, model,
                     sigma_px, huber_px, iters, damping, B, max_obj, S, V, pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
}

int okp_refine_views_weighted_wide(const char* fn, const double* obs, const double* prior, const double* views, int32_t views_each, const double* pose,
                                   const int32_t* assignment, const int32_t* n_obj, const double* model, double sigma_px, double huber_px, int32_t iters,
                                   double damping, int32_t B, int32_t max_obj, int32_t S, int32_t V, double* pose_out, double* fit, int32_t* n_obs,
                                   int32_t* n_inlier, double* weight, double* information, int32_t* status, void* stream) {
  return wide_launch(fn, "okp_refine_pose_views_weighted launch", true, obs, prior, views, views_each, pose, assignment, n_obj, model, sigma_px, huber_px, iters,
                     damping, B, max_obj, S, V, pose_out, fit, n_obs, n_inlier, weight, information, status, stream);
}
