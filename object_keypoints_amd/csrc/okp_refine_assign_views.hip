// Resolving a rig's interchangeable key points against every camera's bearings (okp_refine_assignments_views; contract in include/okp.h).
// okp_object_pose picks the assignment of an object's key points to interchangeable model instances by a rigid fit to FUSED points, which the
// depth noise of short baselines misleads; okp_refine_pose_views then polishes the pose under that assignment, right or wrong.  The bearings
// of the 2P cameras do tell the assignments apart: this stage refines EVERY assignment - each from its own rigid fit to the fused points, by
// the Gauss-Newton steps of okp_refine_pose_views - and keeps the one of least final cost, as okp_refine_assignments does for one camera.
//
//   okp_refine_assignments_views_kernel   one workgroup of FOUR waves per object; wave w runs the hypotheses w, w + 4, ... over ceil(H / 4)
//                                  rounds, so the six assignments of a valve take two.  Within a wave the lanes are laid out as in
//                                  okp_refine_pose_views_kernel (csrc/okp_refine_views.hip): G = 64 / Vp groups of Vp lanes, lane (g, v) is
//                                  camera v and takes the slots g, g + G, ...; its row of `views` and its bearings stay in registers over all
//                                  rounds, only the model rows of its slots change with the hypothesis.  The start of a hypothesis is
//                                  computed as in okp_refine_assignments_kernel (csrc/okp_refine_assign.hip): every lane loads table slot
//                                  lane & 15, decodes the model row that slot takes, and sums run over sixteen lanes, so every lane of the wave
//                                  holds the same bits of Horn's fit; a lane then fetches the rows of its own slots from the lanes that
//                                  decoded them.  The iteration is the one-wave kernel's: a lane adds its slots' terms in ascending
//                                  order, one xor-butterfly over the 64 lanes, every lane solves the same 6 x 6 system (refine_step).  A
//                                  status, once set, sticks; the arithmetic runs on regardless.  A wave keeps its best two hypotheses by
//                                  (cost, index) and the best one's record in registers.  Four waves of a workgroup are one wave per SIMD:
//                                  each has the one-wave kernel's register budget, and the kernel uses no scratch memory.
//
// Barriers.  There is ONE: after its last round every wave stores its best two and its winner's record to LDS, the workgroup meets, and wave 0
// selects among the four and writes every output word.  No thread returns before it; a skipped object skips the rounds on a branch and still
// arrives.  What decides that branch and the number of rounds - whether the object is live, its pose finite, its bearings well-formed, the
// filled mask, the observed slots - every wave computes from the same words of memory by the same instructions, so they are the same in all
// four (the note on barriers in csrc/okp_refine_views_wide.hip); the loop over the rounds encloses no barrier.
// fp64, no atomics, no host wait, contraction off; the summation order is fixed, so the bits are the same on every run.
#include "okp_pose_math.h"           // PoseTypes, pose_types, hypothesis_instance, horn_matrix, jacobi_sym, scatter_degenerate, view_term, refine_step, ...

#pragma clang fp contract(off)

namespace {

#define OKP_RAV_WAVES 4
#define OKP_RAV_RECORD 34            // a wave's winner: R (9), t (3), the upper triangle of H (21), the cost at its start

struct AssignViewsParams {
  const double* obs; const double* views; const double* tab; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, V, iters, vshift;             // Vp = 1 << vshift >= V lanes per group
  PoseTypes types;
  double sigma_px, damping;
  double* pose_out; double* fit; int32_t* n_obs; double* information; int32_t* status; int32_t* assignment_out; int32_t* hypothesis; double* cost;
};

__device__ __forceinline__ double sum16(double v) {
#pragma unroll
  for (int off = OKP_REFINE_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The sums over the wave's 64 lanes (H, g and the cost)
__device__ __forceinline__ void sum64(double (&acc)[OKP_REFINE_SUMS]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] += __shfl_xor(acc[i], off);
}

// (cost a, index i) comes before (cost b, index j); an index < 0 is no hypothesis
__device__ __forceinline__ bool before(double a, int i, double b, int j) { return i >= 0 && (j < 0 || a < b || (a == b && i < j)); }

__global__ __launch_bounds__(64 * OKP_RAV_WAVES) void okp_refine_assignments_views_kernel(const AssignViewsParams P) {
  __shared__ double s_cost[OKP_RAV_WAVES][2];
  __shared__ int32_t s_hyp[OKP_RAV_WAVES][2];
  __shared__ double s_rec[OKP_RAV_WAVES][OKP_RAV_RECORD];
  __shared__ int32_t s_row[OKP_RAV_WAVES][OKP_REFINE_LANES];

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane & (OKP_REFINE_LANES - 1);
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];
  const int K = P.types.K, S = P.types.S, V = P.V;
  const int G = 64 >> P.vshift, grp = lane >> P.vshift, cam = lane & ((1 << P.vshift) - 1);
  const int passes = (S + G - 1) / G;                             // slots per lane: slot grp + G i in pass i
  const bool view = cam < V;
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  // (0) the precheck, the same in every wave.  The table: lane s of every sixteen holds slot s
  bool pose_finite = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_finite = pose_finite && finite64(P.pose[oi * 12 + i]);
  double X = 0.0, Y = 0.0, Z = 0.0;
  bool filled = false;
  if (live && sub < S) {
    const double* row = P.tab + (oi * S + sub) * 4;
    const double r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
    filled = finite64(r0) && finite64(r1) && finite64(r2) && finite64(r3);
    if (filled) { X = r0; Y = r1; Z = r2; }
  }
  const uint32_t mask = (uint32_t)(__ballot(filled) & 0xffffull);            // (the four groups of sixteen hold the same slots)
  const int n = __popc(mask);
  // this lane's camera: [R_v | t_v] and k_v = (fx_v, fy_v) / sigma_px (the lanes past V: an identity that observes nothing)
  double rv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tv[3] = {0.0, 0.0, 0.0}, kx = 1.0, ky = 1.0;
  if (view) {
    const double* row = P.views + (size_t)cam * 14;
#pragma unroll
    for (int i = 0; i < 3; ++i) { rv[3 * i + 0] = row[4 * i + 0]; rv[3 * i + 1] = row[4 * i + 1]; rv[3 * i + 2] = row[4 * i + 2]; tv[i] = row[4 * i + 3]; }
    kx = row[12] / P.sigma_px; ky = row[13] / P.sigma_px;
  }
  // the bearings of this lane's slots; an observation is a filled entry of a FILLED slot, whatever the hypothesis
  double ou[OKP_POSE_MAX_POINTS], ov[OKP_POSE_MAX_POINTS];
  unsigned seen = 0u, rows = 0u;                                  // bit i: this lane observed its slot of pass i; some lane's slot of pass i is filled
  int n_obs = 0, n_rows = 0;
  bool bad = false;
  unsigned long long first = 0ull;                                // the first lane of every group
  for (int g = 0; g < G; ++g) first |= 1ull << (g << P.vshift);
#pragma unroll
  for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
    ou[i] = 0.0; ov[i] = 0.0;
    if (i < passes) {                                             // (wave-uniform)
      const int s = grp + G * i;
      const bool slot = live && s < S;
      const bool has = slot && ((mask >> s) & 1u);
      double u = nan, v = nan;
      if (slot && view) {
        const double* e = P.obs + ((oi * S + s) * V + cam) * 2;
        u = e[0]; v = e[1];
      }
      bad = bad || ((u != u) != (v != v)) || fabs(u) == inf || fabs(v) == inf;
      const bool mine = has && finite64(u) && finite64(v);
      unsigned long long who = __ballot(mine);
      n_obs += __popcll(who);
      for (int sh = 1; sh < (1 << P.vshift); sh <<= 1) who |= who >> sh;          // a group's first lane: some lane of the group observed the slot
      n_rows += __popcll(who & first);
      if (mine) { ou[i] = u; ov[i] = v; seen |= 1u << i; }
      if (__ballot(has) != 0ull) rows |= 1u << i;
    }
  }
  const bool any_bad = __ballot(bad) != 0ull;
  const bool skipped = !live || !pose_finite || any_bad || n_rows < 3;        // (the same in the four waves: no word of it is a wave's own)

  // this wave's best hypothesis so far, with what the outputs need of it, and its second best by cost and index
  double best_J = inf, second_J = inf;
  int best_h = -1, second_h = -1, best_row = -1;
  double best[OKP_RAV_RECORD];
#pragma unroll
  for (int i = 0; i < OKP_RAV_RECORD; ++i) best[i] = nan;

  if (!skipped) {
    // (1) what every hypothesis shares: the fused points centred on their mean, the number of hypotheses
    const double inv_n = 1.0 / n;
    const double pb0 = sum16(filled ? X : 0.0) * inv_n, pb1 = sum16(filled ? Y : 0.0) * inv_n, pb2 = sum16(filled ? Z : 0.0) * inv_n;
    const double c0 = filled ? X - pb0 : 0.0, c1 = filled ? Y - pb1 : 0.0, c2 = filled ? Z - pb2 : 0.0;
    const double g0 = P.model[0], g1 = P.model[1], g2 = P.model[2];             // model row 0: the model points are taken relative to it
    int H = 1;
    for (int k = 1; k < K; ++k) {
      const int c = P.types.count[k];
      const int nk = __popc((mask >> P.types.base[k]) & ((1u << c) - 1u));
      for (int i = 0; i < nk; ++i) H *= c - i;
    }
    const int rounds = (H + OKP_RAV_WAVES - 1) / OKP_RAV_WAVES;

    for (int round = 0; round < rounds; ++round) {
      const int h = round * OKP_RAV_WAVES + wave;
      if (h >= H) continue;                                       // (wave-uniform; an idle wave of the last round keeps nothing, and no barrier is inside)
      // (2) the model row of slot `sub` under hypothesis h: mixed radix over the types, type 1 the slowest digit
      int row = (sub == 0 && filled) ? 0 : -1;
      {
        int stride = 1;
        for (int k = K - 1; k >= 1; --k) {
          const int c = P.types.count[k], base = P.types.base[k];
          const uint32_t tmask = (mask >> base) & ((1u << c) - 1u);
          const int nk = __popc(tmask);
          int hk = 1;
          for (int i = 0; i < nk; ++i) hk *= c - i;
          const int digit = (h / stride) % hk;
          stride *= hk;
          if (filled && sub >= base && sub < base + c) {
            const int mine = __popc(tmask & ((1u << (sub - base)) - 1u));
            row = base + hypothesis_instance(c, nk, hk, digit, mine);
          }
        }
      }
      row = min(row, S - 1);
      const bool pair = row >= 0;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0;                        // the model point relative to row 0
      if (pair) { m0 = P.model[row * 3 + 0] - g0; m1 = P.model[row * 3 + 1] - g1; m2 = P.model[row * 3 + 2] - g2; }
      // (3) the start: the rigid fit of the hypothesis (Horn), and the degeneracy rule on its matched model points
      const double mb0 = sum16(m0) * inv_n, mb1 = sum16(m1) * inv_n, mb2 = sum16(m2) * inv_n;
      const double a0 = pair ? m0 - mb0 : 0.0, a1 = pair ? m1 - mb1 : 0.0, a2 = pair ? m2 - mb2 : 0.0;
      double R[9], t[3];
      int status = 0;
      {
        double M[3][3], Am[3][3], N[4][4], Vq[4][4];
        M[0][0] = sum16(a0 * c0); M[0][1] = sum16(a0 * c1); M[0][2] = sum16(a0 * c2);
        M[1][0] = sum16(a1 * c0); M[1][1] = sum16(a1 * c1); M[1][2] = sum16(a1 * c2);
        M[2][0] = sum16(a2 * c0); M[2][1] = sum16(a2 * c1); M[2][2] = sum16(a2 * c2);
        Am[0][0] = sum16(a0 * a0); Am[0][1] = sum16(a0 * a1); Am[0][2] = sum16(a0 * a2);
        Am[1][1] = sum16(a1 * a1); Am[1][2] = sum16(a1 * a2); Am[2][2] = sum16(a2 * a2);
        Am[1][0] = Am[0][1]; Am[2][0] = Am[0][2]; Am[2][1] = Am[1][2];
        status = scatter_degenerate(Am) ? OKP_REFINE_SINGULAR : 0;
        horn_matrix(M, N);
        jacobi_sym<4, true>(N, Vq);
        int top = 0;
#pragma unroll
        for (int i = 1; i < 4; ++i) top = N[i][i] > N[top][top] ? i : top;
        double q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = top == 0 ? Vq[i][0] : top == 1 ? Vq[i][1] : top == 2 ? Vq[i][2] : Vq[i][3];
        const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
        R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
        R[3] = 2.0 * (y * x + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
        R[6] = 2.0 * (z * x - w * y);         R[7] = 2.0 * (z * y + w * x);         R[8] = w * w - x * x - y * y + z * z;
        const double s0 = g0 + mb0, s1 = g1 + mb1, s2 = g2 + mb2;                // the matched model points' mean
        t[0] = pb0 - ((R[0] * s0 + R[1] * s1) + R[2] * s2);
        t[1] = pb1 - ((R[3] * s0 + R[4] * s1) + R[5] * s2);
        t[2] = pb2 - ((R[6] * s0 + R[7] * s1) + R[8] * s2);
      }
      // the model rows of this lane's own slots, from the lanes that decoded them (lane s of the wave holds slot s)
      double m[OKP_POSE_MAX_POINTS][3];
#pragma unroll
      for (int i = 0; i < OKP_POSE_MAX_POINTS; ++i) {
        m[i][0] = 0.0; m[i][1] = 0.0; m[i][2] = 0.0;
        if (i < passes) {                                           // (wave-uniform)
          const int s = grp + G * i;
          const int a = __shfl(row, s & (OKP_REFINE_LANES - 1));
          if (s < S && a >= 0) { m[i][0] = P.model[a * 3 + 0]; m[i][1] = P.model[a * 3 + 1]; m[i][2] = P.model[a * 3 + 2]; }
        }
      }
      // (4) exactly `iters` steps of okp_refine_pose_views from that start
      double acc[OKP_REFINE_SUMS];
      double J0 = nan;
      for (int k = 0;; ++k) {
#pragma unroll
        for (int i = 0; i < OKP_REFINE_SUMS; ++i) acc[i] = 0.0;
        bool behind = false;
#pragma unroll
        for (int s = 0; s < OKP_POSE_MAX_POINTS; ++s) {           // (s: the pass; the lane's slot of it)
          if (!((rows >> s) & 1u)) continue;                      // (wave-uniform)
          const bool mine = (seen >> s) & 1u;
          const ViewTerm T = view_term(R, t, rv, tv, kx, ky, m[s][0], m[s][1], m[s][2], ou[s], ov[s]);
          behind = behind || (mine && T.qz <= 0.0);
          double e[2] = {T.e0, T.e1};
          double j[2][6] = {{T.p1 * T.bu2 - T.p2 * T.bu1, T.p2 * T.bu0 - T.p0 * T.bu2, T.p0 * T.bu1 - T.p1 * T.bu0, T.bu0, T.bu1, T.bu2},
                            {T.p1 * T.bv2 - T.p2 * T.bv1, T.p2 * T.bv0 - T.p0 * T.bv2, T.p0 * T.bv1 - T.p1 * T.bv0, T.bv0, T.bv1, T.bv2}};
          if (!mine) {
            e[0] = 0.0; e[1] = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) { j[0][c] = 0.0; j[1][c] = 0.0; }
          }
          int idx = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { acc[idx] += j[0][r] * j[0][c] + j[1][r] * j[1][c]; ++idx; }
#pragma unroll
          for (int r = 0; r < 6; ++r) acc[21 + r] += j[0][r] * e[0] + j[1][r] * e[1];
          acc[27] += e[0] * e[0] + e[1] * e[1];
        }
        if (status == 0 && __ballot(behind) != 0ull) status = OKP_REFINE_BEHIND;
        sum64(acc);
        if (k == 0) J0 = acc[27];
        if (k == P.iters) break;                                  // acc holds the sums at the final iterate
        const bool singular = refine_step(acc, P.damping, R, t);
        if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
      }
      const double J1 = acc[27];
      if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n_obs)) status = OKP_REFINE_REJECTED;
      // (5) this wave's best two by (cost, index); its hypotheses come in ascending order, so a tie keeps the earlier one
      if (status == 0) {
        if (best_h < 0 || J1 < best_J) {
          second_J = best_J; second_h = best_h;
          best_J = J1; best_h = h; best_row = row;
#pragma unroll
          for (int i = 0; i < 9; ++i) best[i] = R[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) best[9 + i] = t[i];
#pragma unroll
          for (int i = 0; i < 21; ++i) best[12 + i] = acc[i];
          best[33] = J0;
        } else if (second_h < 0 || J1 < second_J) {
          second_J = J1; second_h = h;
        }
      }
    }
  }

  // (6) every wave's best two and its winner's record to LDS - every lane of the wave holds the same values -, then the ONE barrier
  if (lane < OKP_REFINE_LANES) s_row[wave][lane] = best_row;
  if (lane == 0) {
    s_cost[wave][0] = best_J; s_cost[wave][1] = second_J;
    s_hyp[wave][0] = best_h; s_hyp[wave][1] = second_h;
#pragma unroll
    for (int i = 0; i < OKP_RAV_RECORD; ++i) s_rec[wave][i] = best[i];
  }
  __syncthreads();
  if (wave != 0) return;

  // (7) wave 0: the winner over the four waves, then the runner-up among what is left
  double wc = inf, sc = inf;
  int wh = -1, sh = -1, ww = 0;
#pragma unroll
  for (int w = 0; w < OKP_RAV_WAVES; ++w)
    if (before(s_cost[w][0], s_hyp[w][0], wc, wh)) { wc = s_cost[w][0]; wh = s_hyp[w][0]; ww = w; }
#pragma unroll
  for (int w = 0; w < OKP_RAV_WAVES; ++w) {
    const int which = w == ww ? 1 : 0;                            // (the winner's wave offers its second)
    if (before(s_cost[w][which], s_hyp[w][which], sc, sh)) { sc = s_cost[w][which]; sh = s_hyp[w][which]; }
  }

  // (8) outputs: every word is written by every call
  const bool ok = wh >= 0;
  if (lane < S) P.assignment_out[oi * S + lane] = ok ? s_row[ww][lane] : (live ? P.assignment[oi * S + lane] : -1);
  if (lane != 0) return;
  double* pose_out = P.pose_out + oi * 12;
  double* fit = P.fit + oi * 2;
  const double* rec = s_rec[ww];
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = rec[3 * i + 0]; pose_out[4 * i + 1] = rec[3 * i + 1]; pose_out[4 * i + 2] = rec[3 * i + 2]; pose_out[4 * i + 3] = rec[9 + i]; }
  } else {                                                        // the input pose, bit for bit (NaN payloads included); NaN past n_obj
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pose_out);
    const unsigned long long nan_bits = 0x7ff8000000000000ull;
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = live ? src[i] : nan_bits;
  }
  fit[0] = ok ? sqrt(rec[33] / n_obs) * P.sigma_px : nan;
  fit[1] = ok ? sqrt(wc / n_obs) * P.sigma_px : nan;
  double Hm[21];
#pragma unroll
  for (int i = 0; i < 21; ++i) Hm[i] = rec[12 + i];
  write_information(Hm, ok, P.information + oi * 36);
  P.n_obs[oi] = n_obs;
  P.hypothesis[oi * 2 + 0] = ok ? wh : -1; P.hypothesis[oi * 2 + 1] = ok ? sh : -1;
  P.cost[oi * 2 + 0] = ok ? wc : nan; P.cost[oi * 2 + 1] = (ok && sh >= 0) ? sc : nan;
  P.status[oi] = ok ? 0 : (skipped ? OKP_REFINE_SKIPPED : OKP_REFINE_NONE);
}

}  // namespace

extern "C" int okp_refine_assignments_views(const double* obs, const double* views, const double* tab, const double* pose, const int32_t* assignment,
                                            const int32_t* n_obj, const double* model, const int32_t* type_count, int32_t K, double sigma_px, int32_t iters,
                                            double damping, int32_t B, int32_t max_obj, int32_t V, double* pose_out, double* fit, int32_t* n_obs,
                                            double* information, int32_t* status, int32_t* assignment_out, int32_t* hypothesis, double* cost, void* stream) {
  const char* fn = "okp_refine_assignments_views";
  AssignViewsParams p = {};
  long long H = 0;
  int rc = pose_types(fn, type_count, K, OKP_POSE_MAX_TYPES, p.types, &H);
  if (rc) return rc;
  if (H > OKP_REFINE_MAX_HYPOTHESES) {
    okp_set_error("%s: type_count gives prod(c_k!) = %lld hypotheses per object, above %d", fn, H, OKP_REFINE_MAX_HYPOTHESES);
    return OKP_EINVAL;
  }
  if ((rc = refine_scalars(fn, B, max_obj, p.types.S, V, OKP_REFINE_MAX_VIEWS, iters, sigma_px, nullptr, damping))) return rc;      // (S: pose_types has checked it)
  const NamedArg required[] = {
      {obs, "obs"}, {views, "views"}, {tab, "tab"}, {pose, "pose"}, {assignment, "assignment"}, {n_obj, "n_obj"}, {model, "model"}, {pose_out, "pose_out"},
      {fit, "fit"}, {n_obs, "n_obs"}, {information, "information"}, {status, "status"}, {assignment_out, "assignment_out"}, {hypothesis, "hypothesis"},
      {cost, "cost"}};
  if ((rc = require_args(fn, required))) return rc;
  const size_t n_total = (size_t)B * max_obj;
  if ((rc = refuse_pose_overlap(fn, pose, pose_out, n_total))) return rc;
  if (overlap(assignment_out, n_total * p.types.S * sizeof(int32_t), assignment, n_total * p.types.S * sizeof(int32_t))) {
    okp_set_error("%s: assignment_out overlaps assignment: the input assignment is the fallback", fn);
    return OKP_EINVAL;
  }
  p.obs = obs; p.views = views; p.tab = tab; p.pose = pose; p.assignment = assignment; p.n_obj = n_obj; p.model = model;
  p.max_obj = max_obj; p.V = V; p.iters = iters;
  while ((1 << p.vshift) < V) ++p.vshift;
  p.sigma_px = sigma_px; p.damping = damping;
  p.pose_out = pose_out; p.fit = fit; p.n_obs = n_obs; p.information = information; p.status = status; p.assignment_out = assignment_out;
  p.hypothesis = hypothesis; p.cost = cost;
  hipLaunchKernelGGL(okp_refine_assignments_views_kernel, dim3((unsigned)n_total), dim3(64 * OKP_RAV_WAVES), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_refine_assignments_views launch");
}
