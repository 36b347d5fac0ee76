// Resolving interchangeable key points by refinement (okp_refine_assignments; contract in include/okp.h): okp_object_pose picks the assignment
// of an object's key points to interchangeable model instances by a rigid 3D fit, which centimetres of depth noise mislead; the bearings do
// tell the assignments apart.  This stage refines EVERY assignment of an object - each from its own rigid fit, by the Gauss-Newton steps of
// okp_refine_pose - and keeps the one with the least final cost.
//
// At most 24 six-parameter problems per object, a few hundred objects per step: latency-bound.  One wave per object, one workgroup per wave;
// the four 16-lane groups of the wave run one hypothesis each at a time, over ceil(H / 4) rounds; no LDS, no atomics, no host wait.
//
//   lane s of a group = table slot s: its bearing (u, v), its depth Z and the centred point stay in registers over all rounds.  Per round the
//   lane decodes the model row its slot takes under the group's hypothesis, two butterflies over the sixteen lanes give the correlation with
//   the centred points and the scatter of the matched model points - after them every lane of the group holds the same bits -, every lane
//   solves Horn's 4 x 4 problem by Jacobi (the start) and then runs the steps of okp_refine_pose (csrc/okp_pose_math.h: the very functions
//   that kernel calls).  A status, once set, sticks; the arithmetic runs on regardless, so the four groups stay in step.  A group keeps its
//   best hypothesis' results in registers; after the last round two butterflies across the groups pick the winner and the runner-up by
//   (cost, index), and the group that holds the winner writes it.  A group without a hypothesis in the last round computes on hypothesis 0
//   and keeps nothing.
#include "okp_pose_math.h"

#pragma clang fp contract(off)

static_assert(OKP_REFINE_MAX_HYPOTHESES <= 0x7fff, "a hypothesis index and -1 fit an int32 with room to spare");

namespace {

struct AssignParams {
  const double* tab; const double* pose; const int32_t* assignment; const int32_t* n_obj; const double* model;
  int32_t max_obj, iters;
  PoseTypes types;
  double kx, ky, kz, sigma_px, damping;          // fx / sigma_px, fy / sigma_px, 1 / sigma_z (0: no depth term), formed once on the host
  double* pose_out; double* fit; double* information; int32_t* status; int32_t* assignment_out; int32_t* hypothesis; double* cost;
};

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int off = OKP_REFINE_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(64) void okp_refine_assignments_kernel(const AssignParams P) {
  const int lane = threadIdx.x, sub = lane & (OKP_REFINE_LANES - 1), grp = lane / OKP_REFINE_LANES;
  const size_t oi = blockIdx.x;
  const int b = (int)(oi / P.max_obj), o = (int)(oi - (size_t)b * P.max_obj);
  const bool live = o < P.n_obj[b];
  const int K = P.types.K, S = P.types.S;
  const double nan = __builtin_nan(""), inf = __builtin_inf();

  // (0) the precheck of okp_refine_pose on the filled slots; the whole wave serves one object, so the way out is uniform
  bool pose_finite = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) pose_finite = pose_finite && finite64(P.pose[oi * 12 + i]);
  double X = 0.0, Y = 0.0, Z = 1.0;
  bool filled = false;
  if (live && sub < S) {
    const double* row = P.tab + (oi * S + sub) * 4;
    const double r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
    filled = finite64(r0) && finite64(r1) && finite64(r2) && finite64(r3);
    if (filled) { X = r0; Y = r1; Z = r2; }
  }
  const double u = X / Z, v = Y / Z;
  const bool bad = filled && (Z == 0.0 || !finite64(u) || !finite64(v));
  const uint32_t mask = (uint32_t)(__ballot(filled) & 0xffffull);            // (the four groups hold the same slots)
  const int n = __popc(mask);
  const bool any_bad = __ballot(bad) != 0ull;
  int32_t* assignment_out = P.assignment_out + oi * S;
  if (!live || !pose_finite || n < 3 || any_bad) {
    if (grp != 0) return;
    if (sub < S) assignment_out[sub] = live ? P.assignment[oi * S + sub] : -1;
    if (sub != 0) return;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(P.pose_out + oi * 12);
    const unsigned long long nan_bits = 0x7ff8000000000000ull;
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = live ? src[i] : nan_bits;           // the input pose, bit for bit (NaN payloads included)
#pragma unroll
    for (int i = 0; i < 4; ++i) P.fit[oi * 4 + i] = nan;
#pragma unroll
    for (int i = 0; i < 36; ++i) P.information[oi * 36 + i] = nan;
    P.hypothesis[oi * 2 + 0] = -1; P.hypothesis[oi * 2 + 1] = -1;
    P.cost[oi * 2 + 0] = nan; P.cost[oi * 2 + 1] = nan;
    P.status[oi] = OKP_REFINE_SKIPPED;
    return;
  }

  // (1) what every hypothesis shares: the detected points centred on their mean, this slot's type, the number of hypotheses
  const double inv_n = 1.0 / n;
  const double pb0 = group_sum(filled ? X : 0.0) * inv_n, pb1 = group_sum(filled ? Y : 0.0) * inv_n, pb2 = group_sum(filled ? Z : 0.0) * inv_n;
  const double c0 = filled ? X - pb0 : 0.0, c1 = filled ? Y - pb1 : 0.0, c2 = filled ? Z - pb2 : 0.0;
  const double g0 = P.model[0], g1 = P.model[1], g2 = P.model[2];             // model row 0: the model points are taken relative to it
  int H = 1;
  for (int k = 1; k < K; ++k) {
    const int c = P.types.count[k];
    const int nk = __popc((mask >> P.types.base[k]) & ((1u << c) - 1u));
    for (int i = 0; i < nk; ++i) H *= c - i;
  }
  const int rounds = (H + 3) / 4;
  const double kx = P.kx, ky = P.ky, kz = P.kz;

  // this group's best hypothesis so far, with what the outputs need of it, and its second best by cost and index
  double best_J = inf, second_J = inf;
  int best_h = -1, second_h = -1, best_row = -1;
  double best_R[9], best_t[3], best_H[21], best_px0 = nan, best_px1 = nan, best_dz0 = nan, best_dz1 = nan;
#pragma unroll
  for (int i = 0; i < 9; ++i) best_R[i] = nan;
#pragma unroll
  for (int i = 0; i < 3; ++i) best_t[i] = nan;
#pragma unroll
  for (int i = 0; i < 21; ++i) best_H[i] = nan;

  for (int round = 0; round < rounds; ++round) {
    const bool valid = round * 4 + grp < H;
    const int h = valid ? round * 4 + grp : 0;
    // (2) the model row of this slot under hypothesis h: mixed radix over the types, type 1 the slowest digit
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
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0;           // the model point as it is, and relative to row 0
    if (pair) {
      e0 = P.model[row * 3 + 0]; e1 = P.model[row * 3 + 1]; e2 = P.model[row * 3 + 2];
      m0 = e0 - g0; m1 = e1 - g1; m2 = e2 - g2;
    }
    // (3) the start: the rigid fit of the hypothesis (Horn), and the degeneracy rule on its matched model points
    const double mb0 = group_sum(m0) * inv_n, mb1 = group_sum(m1) * inv_n, mb2 = group_sum(m2) * inv_n;
    const double a0 = pair ? m0 - mb0 : 0.0, a1 = pair ? m1 - mb1 : 0.0, a2 = pair ? m2 - mb2 : 0.0;
    double M[3][3], Am[3][3], N[4][4], Vq[4][4];
    M[0][0] = group_sum(a0 * c0); M[0][1] = group_sum(a0 * c1); M[0][2] = group_sum(a0 * c2);
    M[1][0] = group_sum(a1 * c0); M[1][1] = group_sum(a1 * c1); M[1][2] = group_sum(a1 * c2);
    M[2][0] = group_sum(a2 * c0); M[2][1] = group_sum(a2 * c1); M[2][2] = group_sum(a2 * c2);
    Am[0][0] = group_sum(a0 * a0); Am[0][1] = group_sum(a0 * a1); Am[0][2] = group_sum(a0 * a2);
    Am[1][1] = group_sum(a1 * a1); Am[1][2] = group_sum(a1 * a2); Am[2][2] = group_sum(a2 * a2);
    Am[1][0] = Am[0][1]; Am[2][0] = Am[0][2]; Am[2][1] = Am[1][2];
    int status = scatter_degenerate(Am) ? OKP_REFINE_SINGULAR : 0;
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
    double R[9], t[3];
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (y * x + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (z * x - w * y);         R[7] = 2.0 * (z * y + w * x);         R[8] = w * w - x * x - y * y + z * z;
    {
      const double s0 = g0 + mb0, s1 = g1 + mb1, s2 = g2 + mb2;                // the matched model points' mean
      t[0] = pb0 - ((R[0] * s0 + R[1] * s1) + R[2] * s2);
      t[1] = pb1 - ((R[3] * s0 + R[4] * s1) + R[5] * s2);
      t[2] = pb2 - ((R[6] * s0 + R[7] * s1) + R[8] * s2);
    }
    // (4) exactly `iters` steps of okp_refine_pose from that start
    const int shift = grp * OKP_REFINE_LANES;
    double acc[OKP_REFINE_SUMS];
    double J0 = nan, px0 = nan, dz0 = nan;
    for (int k = 0;; ++k) {
      const double q2 = refine_pair_terms(R, t, pair, e0, e1, e2, u, v, Z, kx, ky, kz, acc);
      const bool behind = pair && q2 <= 0.0;
      const bool any_behind = ((__ballot(behind) >> shift) & 0xffffull) != 0ull;
      if (status == 0 && any_behind) status = OKP_REFINE_BEHIND;
      refine_butterfly(acc);
      if (k == 0) { J0 = acc[27] + acc[28]; px0 = acc[27]; dz0 = acc[29]; }
      if (k == P.iters) break;                                    // acc holds the sums at the final iterate
      const bool singular = refine_step(acc, P.damping, R, t);
      if (status == 0 && singular) status = OKP_REFINE_SINGULAR;
    }
    const double J1 = acc[27] + acc[28];
    if (status == 0 && (!(J1 < inf) || J1 > J0 + 1e-12 * n)) status = OKP_REFINE_REJECTED;
    // (5) this group's best two by (cost, index); its hypotheses come in ascending order, so a tie keeps the earlier one
    if (valid && status == 0) {
      if (best_h < 0 || J1 < best_J) {
        second_J = best_J; second_h = best_h;
        best_J = J1; best_h = h; best_row = row;
#pragma unroll
        for (int i = 0; i < 9; ++i) best_R[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) best_t[i] = t[i];
#pragma unroll
        for (int i = 0; i < 21; ++i) best_H[i] = acc[i];
        best_px0 = px0; best_px1 = acc[27]; best_dz0 = dz0; best_dz1 = acc[29];
      } else if (second_h < 0 || J1 < second_J) {
        second_J = J1; second_h = h;
      }
    }
  }

  // (6) the winner over the four groups, then the runner-up among what is left (every lane of a group holds the group's values)
  double wc = best_J; int wh = best_h;
#pragma unroll
  for (int off = 32; off >= OKP_REFINE_LANES; off >>= 1) {
    const double oc = __shfl_xor(wc, off); const int oh = __shfl_xor(wh, off);
    if (oh >= 0 && (wh < 0 || oc < wc || (oc == wc && oh < wh))) { wc = oc; wh = oh; }
  }
  double sc = best_h == wh ? second_J : best_J; int sh = best_h == wh ? second_h : best_h;
#pragma unroll
  for (int off = 32; off >= OKP_REFINE_LANES; off >>= 1) {
    const double oc = __shfl_xor(sc, off); const int oh = __shfl_xor(sh, off);
    if (oh >= 0 && (sh < 0 || oc < sc || (oc == sc && oh < sh))) { sc = oc; sh = oh; }
  }

  // (7) outputs: every word is written by every call - by the group that holds the winner, or by group 0 when there is none
  double* pose_out = P.pose_out + oi * 12;
  double* fit = P.fit + oi * 4;
  double* info = P.information + oi * 36;
  if (wh < 0) {
    if (grp != 0) return;
    if (sub < S) assignment_out[sub] = P.assignment[oi * S + sub];
    if (sub != 0) return;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.pose + oi * 12);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(pose_out);
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = src[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) fit[i] = nan;
#pragma unroll
    for (int i = 0; i < 36; ++i) info[i] = nan;
    P.hypothesis[oi * 2 + 0] = -1; P.hypothesis[oi * 2 + 1] = -1;
    P.cost[oi * 2 + 0] = nan; P.cost[oi * 2 + 1] = nan;
    P.status[oi] = OKP_REFINE_NONE;
    return;
  }
  if (best_h != wh) return;
  if (sub < S) assignment_out[sub] = best_row;
  if (sub != 0) return;
#pragma unroll
  for (int i = 0; i < 3; ++i) { pose_out[4 * i + 0] = best_R[3 * i + 0]; pose_out[4 * i + 1] = best_R[3 * i + 1]; pose_out[4 * i + 2] = best_R[3 * i + 2]; pose_out[4 * i + 3] = best_t[i]; }
  fit[0] = sqrt(best_px0 / n) * P.sigma_px;
  fit[1] = sqrt(best_px1 / n) * P.sigma_px;
  fit[2] = sqrt(best_dz0 / n);
  fit[3] = sqrt(best_dz1 / n);
  {
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        const double hv = best_H[idx++];
        info[6 * r + c] = hv; info[6 * c + r] = hv;
      }
  }
  P.hypothesis[oi * 2 + 0] = wh; P.hypothesis[oi * 2 + 1] = sh;
  P.cost[oi * 2 + 0] = wc; P.cost[oi * 2 + 1] = sh >= 0 ? sc : nan;
  P.status[oi] = 0;
}

}  // namespace

extern "C" int okp_refine_assignments(const double* tab, const double* pose, const int32_t* assignment, const int32_t* n_obj, const double* model,
                                      const int32_t* type_count, int32_t K, const okp_camera* cam, double sigma_px, double sigma_z, int32_t iters,
                                      double damping, int32_t B, int32_t max_obj, double* pose_out, double* fit, double* information, int32_t* status,
                                      int32_t* assignment_out, int32_t* hypothesis, double* cost, void* stream) {
  const char* fn = "okp_refine_assignments";
  AssignParams p = {};
  long long H = 0;
  int rc = pose_types(fn, type_count, K, OKP_POSE_MAX_TYPES, p.types, &H);
  if (rc) return rc;
  if (H > OKP_REFINE_MAX_HYPOTHESES) {
    okp_set_error("%s: type_count gives prod(c_k!) = %lld hypotheses per object, above %d", fn, H, OKP_REFINE_MAX_HYPOTHESES);
    return OKP_EINVAL;
  }
  if ((rc = refine_scalars(fn, B, max_obj, p.types.S, 0, 0, iters, sigma_px, &sigma_z, damping))) return rc;      // (S: pose_types has checked it)
  if ((rc = refine_camera(fn, cam))) return rc;
  const NamedArg required[] = {
      {tab, "tab"}, {pose, "pose"}, {assignment, "assignment"}, {n_obj, "n_obj"}, {model, "model"}, {pose_out, "pose_out"}, {fit, "fit"},
      {information, "information"}, {status, "status"}, {assignment_out, "assignment_out"}, {hypothesis, "hypothesis"}, {cost, "cost"}};
  if ((rc = require_args(fn, required))) return rc;
  const size_t n_total = (size_t)B * max_obj;
  if ((rc = refuse_pose_overlap(fn, pose, pose_out, n_total))) return rc;
  if (overlap(assignment_out, n_total * p.types.S * sizeof(int32_t), assignment, n_total * p.types.S * sizeof(int32_t))) {
    okp_set_error("%s: assignment_out overlaps assignment: the input assignment is the fallback", fn);
    return OKP_EINVAL;
  }
  p.tab = tab; p.pose = pose; p.assignment = assignment; p.n_obj = n_obj; p.model = model;
  p.max_obj = max_obj; p.iters = iters;
  p.kx = cam->fx / sigma_px; p.ky = cam->fy / sigma_px; p.kz = 1.0 / sigma_z; p.sigma_px = sigma_px; p.damping = damping;
  p.pose_out = pose_out; p.fit = fit; p.information = information; p.status = status; p.assignment_out = assignment_out; p.hypothesis = hypothesis; p.cost = cost;
  hipLaunchKernelGGL(okp_refine_assignments_kernel, dim3((unsigned)n_total), dim3(64), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_refine_assignments launch");
}
