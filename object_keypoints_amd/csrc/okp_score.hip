// Accuracy of labelled scenes (okp_score_objects; contract in include/okp.h): a step's object table and up to four sets of poses against
// labelled truth, tabulated in an append-only log in device memory.  The key-point part restates the reference's Results.add
// (scripts/eval_model.py:129-232: match by the centre's x/y, view test of the truth centre, nearest truth row per lifted key point, the 2 m
// range); the pose errors and the detection counters have no reference counterpart.
//
// Two launches.  okp_score_frames_kernel: one wave per frame.  The frame's truth rows and their view flags are staged in LDS once (lanes over
// rows), then lanes over detections take steps 1-3, lanes over detection x slot step 4, lanes over detections step 5 (the sets unrolled, so
// that every set pointer is a scalar load), and the frame's counters are wave reductions of integers.  It writes every record at a fixed
// place of a staging table, [b][o][s] and [b][o], so nothing depends on an order of arrival.  okp_score_log_kernel: one workgroup scans the
// per-detection record counts in (b, o) order from the cursors in `counts` and copies the staged records behind the log's earlier ones.
//
// fp64, no floating-point atomics, no host wait; the same bits on every run and as tests/score_spec.py - except the view test, which
// projects with the arithmetic of okp_project_labels (okp_project_point, compiled with its contraction) and yields a decision only.
#include <math.h>
#include "okp_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMaxObj = 64;               // one lane per detection
constexpr int kMaxTruth = 64;
constexpr int kMaxS = OKP_POSE_MAX_POINTS;
constexpr int kFrameInts = 16;            // per-frame counters at the indices OKP_SCORE_* (2 .. 11 used), then (key-point records, pose records) per detection
constexpr int kLogThreads = 256;
constexpr double kDegrees = 57.29577951308232;      // 180 / pi

struct ScoreSets {
  const double* pose[OKP_SCORE_MAX_POSES];
  const int32_t* index[OKP_SCORE_MAX_POSES];
  int32_t rows[OKP_SCORE_MAX_POSES];
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// step 5: the three errors of one estimated pose E against the labelled pose T (both [R | t] row-major), over the model's S rows
__device__ __forceinline__ void pose_errors(const double* __restrict__ E, const double* __restrict__ T, const double* __restrict__ model, int S,
                                            double* __restrict__ out) {
  double e[12], t[12];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) { e[i] = E[i]; t[i] = T[i]; ok = ok && isfinite(e[i]) && isfinite(t[i]); }
  if (!ok) { out[0] = out[1] = out[2] = NAN; return; }
  double Q[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[3 * a + c] = (t[a] * e[c] + t[4 + a] * e[4 + c]) + t[8 + a] * e[8 + c];
  const double w0 = Q[7] - Q[5], w1 = Q[2] - Q[6], w2 = Q[3] - Q[1];
  const double s = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  const double theta = atan2(s * 0.5, (((Q[0] + Q[4]) + Q[8]) - 1.0) * 0.5);
  double sum = 0.0, centre = 0.0;
  for (int i = 0; i < S; ++i) {
    const double m0 = model[3 * i], m1 = model[3 * i + 1], m2 = model[3 * i + 2];
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double pe = ((e[4 * r] * m0 + e[4 * r + 1] * m1) + e[4 * r + 2] * m2) + e[4 * r + 3];
      const double pt = ((t[4 * r] * m0 + t[4 * r + 1] * m1) + t[4 * r + 2] * m2) + t[4 * r + 3];
      const double d = pe - pt;
      sq = r == 0 ? d * d : sq + d * d;
    }
    if (i == 0) centre = sqrt(sq);
    sum = i == 0 ? sq : sum + sq;
  }
  out[0] = theta * kDegrees;
  out[1] = centre;
  out[2] = sqrt(sum / (double)S);
}

__global__ __launch_bounds__(kWave) void okp_score_frames_kernel(const double* __restrict__ tab, const int32_t* __restrict__ n_obj_dev,
                                                                 const double* __restrict__ truth, const int32_t* __restrict__ n_truth_dev, int32_t max_obj,
                                                                 int32_t G, int32_t S, int32_t has_cam, okp_camera cam, double size_x, double size_y,
                                                                 ScoreSets sets, int32_t P, const double* __restrict__ truth_pose,
                                                                 const double* __restrict__ model, double radius2, double max_range,
                                                                 int32_t* __restrict__ match_out, int32_t* __restrict__ nearest_out,
                                                                 double* __restrict__ stage_f, int32_t* __restrict__ stage_i) {
  __shared__ double tr[kMaxTruth * kMaxS * 3];      // the frame's truth rows (x, y, z), row g * S + j
  __shared__ uint8_t vis[kMaxTruth * kMaxS];        // that row is in view (all 1 without a camera)
  __shared__ uint8_t rec[kMaxObj * kMaxS];          // slot (o, s) emitted a key-point record
  __shared__ int32_t m_of[kMaxObj];
  __shared__ int32_t detected[kMaxTruth];
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = n_obj_dev[b];
  n = n < 0 ? 0 : (n > max_obj ? max_obj : n);
  int nt = n_truth_dev[b];
  nt = nt < 0 ? 0 : (nt > G ? G : nt);
  const double* tb = truth + (size_t)b * G * S * 4;
  for (int r = lane; r < nt * S; r += kWave) {
    const double x = tb[4 * r], y = tb[4 * r + 1], z = tb[4 * r + 2];
    tr[3 * r] = x; tr[3 * r + 1] = y; tr[3 * r + 2] = z;
    bool v = true;
    if (has_cam) {
      double px, py;
      okp_project_point(cam, x, y, z, px, py);
      v = z > 0.0 && px > 0.0 && px < size_x && py > 0.0 && py < size_y;       // (false for a NaN row)
    }
    vis[r] = v ? 1 : 0;
  }
  detected[lane] = 0;
  __syncthreads();

  // steps 1-3: one lane per detection
  int m = -4, c_det = 0, c_noc = 0, c_unm = 0, c_oov = 0;
  if (lane < n) {
    const double* c = tab + ((size_t)b * max_obj + lane) * S * 4;
    const double x = c[0], y = c[1], z = c[2], w = c[3];
    if (!(finite3(x, y, z) && isfinite(w))) {
      m = -1; c_noc = 1;
    } else {
      double best = INFINITY;
      int gs = -1;
      for (int g = 0; g < nt; ++g) {
        const double dx = x - tr[3 * g * S], dy = y - tr[3 * g * S + 1];
        const double d2 = dx * dx + dy * dy;
        if (d2 < best) { best = d2; gs = g; }
      }
      if (gs < 0 || best > radius2) { m = -2; c_unm = 1; }
      else if (!vis[gs * S]) { m = -3; c_oov = 1; }
      else { m = gs; c_det = 1; detected[gs] = 1; }
    }
  }
  if (lane < max_obj) { match_out[(size_t)b * max_obj + lane] = m; m_of[lane] = m; }
  __syncthreads();

  // step 4: lanes over detection x slot
  const int F = 2 * S + 3 * OKP_SCORE_MAX_POSES;    // staged doubles per detection
  int c_pts = 0, c_mis = 0, c_abs = 0, c_hid = 0;
  for (int idx = lane; idx < max_obj * S; idx += kWave) {
    const int o = idx / S, s = idx - o * S;
    int near = -1, emitted = 0;
    double err = NAN, err_xy = NAN;
    const int g = o < n ? m_of[o] : -1;
    if (g >= 0) {
      const double* p = tab + (((size_t)b * max_obj + o) * S + s) * 4;
      const double x = p[0], y = p[1], z = p[2], w = p[3];
      if (!isfinite(w)) {
        c_abs++;
      } else if (!(finite3(x, y, z) && x < max_range && y < max_range && z < max_range)) {
        c_pts++; c_mis++;
      } else {
        double best = INFINITY, best_xy = 0.0;
        for (int j = 0; j < S; ++j) {
          const double* t = tr + 3 * (g * S + j);
          const double dx = x - t[0], dy = y - t[1], dz = z - t[2];
          const double dxy = dx * dx + dy * dy;
          const double d2 = dxy + dz * dz;
          if (d2 < best) { best = d2; best_xy = dxy; near = j; }      // (never for a NaN row)
        }
        if (near < 0 || !vis[g * S + near]) {
          c_hid++;
        } else {
          c_pts++; emitted = 1;
          err = sqrt(best); err_xy = sqrt(best_xy);
        }
      }
    }
    nearest_out[((size_t)b * max_obj + o) * S + s] = near;
    double* out = stage_f + ((size_t)b * max_obj + o) * F + 2 * s;
    out[0] = err; out[1] = err_xy;
    rec[idx] = (uint8_t)emitted;
  }
  __syncthreads();

  // step 5: one lane per detection, the sets in turn
  const bool scored = lane < n && m >= 0;
  if (P > 0 && scored) {
    double* out = stage_f + ((size_t)b * max_obj + lane) * F + 2 * S;
    const double* T = truth_pose + ((size_t)b * G + m) * 12;
#pragma unroll
    for (int p = 0; p < OKP_SCORE_MAX_POSES; ++p) {
      int row = -1;
      if (p < P) row = sets.index[p] ? sets.index[p][(size_t)b * max_obj + lane] : lane;
      if (p < P && row >= 0 && row < sets.rows[p]) pose_errors(sets.pose[p] + ((size_t)b * sets.rows[p] + row) * 12, T, model, S, out + 3 * p);
      else out[3 * p] = out[3 * p + 1] = out[3 * p + 2] = NAN;
    }
  }

  // step 6 and the frame's counters
  int32_t* fi = stage_i + (size_t)b * (kFrameInts + 2 * max_obj);
  if (lane < max_obj) {
    int k = 0;
    for (int s = 0; s < S; ++s) k += rec[lane * S + s];
    fi[kFrameInts + 2 * lane] = k;
    fi[kFrameInts + 2 * lane + 1] = (P > 0 && scored) ? 1 : 0;
  }
  const int seen = lane < nt && vis[lane * S] ? 1 : 0;
  const int found = seen && detected[lane] ? 1 : 0;
  const int t_det = wave_sum(c_det), t_noc = wave_sum(c_noc), t_unm = wave_sum(c_unm), t_oov = wave_sum(c_oov);
  const int t_pts = wave_sum(c_pts), t_mis = wave_sum(c_mis), t_abs = wave_sum(c_abs), t_hid = wave_sum(c_hid);
  const int t_seen = wave_sum(seen), t_found = wave_sum(found);
  if (lane == 0) {
    fi[OKP_SCORE_CALLS] = 0; fi[OKP_SCORE_FRAMES] = 0;
    fi[OKP_SCORE_DETECTIONS] = t_det; fi[OKP_SCORE_NO_CENTRE] = t_noc; fi[OKP_SCORE_UNMATCHED] = t_unm; fi[OKP_SCORE_OUT_OF_VIEW] = t_oov;
    fi[OKP_SCORE_POINTS] = t_pts; fi[OKP_SCORE_MISSING] = t_mis; fi[OKP_SCORE_ABSENT] = t_abs; fi[OKP_SCORE_TRUTH_HIDDEN] = t_hid;
    fi[OKP_SCORE_TRUTH_VISIBLE] = t_seen; fi[OKP_SCORE_TRUTH_DETECTED] = t_found;
    fi[OKP_SCORE_KP_WRITTEN] = 0; fi[OKP_SCORE_POSE_WRITTEN] = 0; fi[OKP_SCORE_OVERFLOW_WORD] = 0; fi[15] = 0;
  }
}

// The staged records of one call, in (b, o, s) order, behind the log's earlier ones.  One workgroup: an exclusive scan of the per-detection
// record counts in chunks of 256 detections with a running carry; every thread then copies its own detection's records.
__global__ __launch_bounds__(kLogThreads) void okp_score_log_kernel(const double* __restrict__ stage_f, const int32_t* __restrict__ stage_i,
                                                                    const int32_t* __restrict__ match, int32_t B, int32_t max_obj, int32_t S,
                                                                    double* __restrict__ kp_err, int32_t* __restrict__ kp_id, int32_t cap_kp,
                                                                    double* __restrict__ pose_err, int32_t* __restrict__ pose_id, int32_t cap_pose,
                                                                    long long* __restrict__ counts) {
  __shared__ int wtot[kLogThreads / kWave][2];
  __shared__ long long red[kLogThreads / kWave][10];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // every thread reads the cursors; they are written once, by thread 0, behind the last barrier
  const int32_t step = (int32_t)counts[OKP_SCORE_CALLS];
  const long long base_kp = counts[OKP_SCORE_KP_WRITTEN], base_pose = counts[OKP_SCORE_POSE_WRITTEN];
  const int W = kFrameInts + 2 * max_obj, F = 2 * S + 3 * OKP_SCORE_MAX_POSES;
  const int N = B * max_obj;
  long long run_kp = 0, run_pose = 0;               // records of the detections before this chunk (the same in every thread)
  for (int c0 = 0; c0 < N; c0 += kLogThreads) {
    const int it = c0 + tid;
    int b = 0, o = 0, ck = 0, cp = 0;
    if (it < N) {
      b = it / max_obj; o = it - b * max_obj;
      ck = stage_i[(size_t)b * W + kFrameInts + 2 * o];
      cp = stage_i[(size_t)b * W + kFrameInts + 2 * o + 1];
    }
    int ik = ck, ip = cp;                           // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int uk = __shfl_up(ik, d), up = __shfl_up(ip, d);
      if (lane >= d) { ik += uk; ip += up; }
    }
    if (lane == kWave - 1) { wtot[wave][0] = ik; wtot[wave][1] = ip; }
    __syncthreads();
    int before_k = 0, before_p = 0, all_k = 0, all_p = 0;
#pragma unroll
    for (int w = 0; w < kLogThreads / kWave; ++w) {
      if (w < wave) { before_k += wtot[w][0]; before_p += wtot[w][1]; }
      all_k += wtot[w][0]; all_p += wtot[w][1];
    }
    if (it < N) {
      long long pos = base_kp + run_kp + before_k + (ik - ck);
      const double* sf = stage_f + ((size_t)b * max_obj + o) * F;
      for (int s = 0; s < S && ck > 0; ++s) {
        const double err = sf[2 * s];
        if (err != err) continue;                   // no record in this slot
        if (pos >= 0 && pos < cap_kp) {
          kp_err[2 * pos] = err; kp_err[2 * pos + 1] = sf[2 * s + 1];
          int32_t* id = kp_id + 4 * pos;
          id[0] = step; id[1] = b; id[2] = o; id[3] = s;
        }
        ++pos;
      }
      if (cp) {
        const long long q = base_pose + run_pose + before_p + (ip - cp);
        if (q >= 0 && q < cap_pose) {
#pragma unroll
          for (int i = 0; i < 3 * OKP_SCORE_MAX_POSES; ++i) pose_err[3 * OKP_SCORE_MAX_POSES * q + i] = sf[2 * S + i];
          int32_t* id = pose_id + 4 * q;
          id[0] = step; id[1] = b; id[2] = o; id[3] = match[(size_t)b * max_obj + o];
        }
      }
    }
    run_kp += all_k; run_pose += all_p;
    __syncthreads();                                // (wtot is reused)
  }
  // the frames' counters: integer sums, exact in any order
  long long tot[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) tot[i] = 0;
  for (int b = tid; b < B; b += kLogThreads)
#pragma unroll
    for (int i = 0; i < 10; ++i) tot[i] += stage_i[(size_t)b * W + OKP_SCORE_DETECTIONS + i];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) tot[i] += __shfl_xor(tot[i], d);
    if (lane == 0) red[wave][i] = tot[i];
  }
  __syncthreads();
  if (tid == 0) {
    counts[OKP_SCORE_CALLS] += 1;
    counts[OKP_SCORE_FRAMES] += B;
    for (int i = 0; i < 10; ++i) counts[OKP_SCORE_DETECTIONS + i] += ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    const long long end_kp = base_kp + run_kp, end_pose = base_pose + run_pose;
    counts[OKP_SCORE_KP_WRITTEN] = end_kp > cap_kp ? cap_kp : end_kp;
    counts[OKP_SCORE_POSE_WRITTEN] = end_pose > cap_pose ? cap_pose : end_pose;
    if (end_kp > cap_kp || end_pose > cap_pose) counts[OKP_SCORE_OVERFLOW_WORD] |= OKP_SCORE_OVERFLOW;
  }
}

}  // namespace

extern "C" int okp_score_objects(const double* tab_dev, const int32_t* n_obj_dev, const double* truth_dev, const int32_t* n_truth_dev, int32_t B,
                                 int32_t max_obj, int32_t G, int32_t S, const okp_camera* cam, double size_x, double size_y,
                                 const double* const* set_pose_dev, const int32_t* const* set_index_dev, const int32_t* set_rows, int32_t P,
                                 const double* truth_pose_dev, const double* model_dev, double match_radius, double max_range, double* kp_err_dev,
                                 int32_t* kp_id_dev, int32_t cap_kp, double* pose_err_dev, int32_t* pose_id_dev, int32_t cap_pose, int64_t* counts_dev,
                                 int32_t* match_dev, int32_t* nearest_dev, double* stage_f_dev, int32_t* stage_i_dev, void* stream) {
  const char* fn = "okp_score_objects";
  if (B < 1 || B > (1 << 20)) { okp_set_error("%s: B = %d frames, 1 to %d are supported", fn, B, 1 << 20); return OKP_EINVAL; }
  if (max_obj < 1 || max_obj > kMaxObj) { okp_set_error("%s: max_obj = %d, 1 to %d are supported (one lane per detection)", fn, max_obj, kMaxObj); return OKP_EINVAL; }
  if (G < 1 || G > kMaxTruth) { okp_set_error("%s: G = %d labelled objects, 1 to %d are supported", fn, G, kMaxTruth); return OKP_EINVAL; }
  if (S < 1 || S > kMaxS) { okp_set_error("%s: S = %d rows per object, 1 to %d (OKP_POSE_MAX_POINTS) are supported", fn, S, kMaxS); return OKP_EINVAL; }
  if (P < 0 || P > OKP_SCORE_MAX_POSES) { okp_set_error("%s: P = %d pose sets, 0 to %d are supported", fn, P, OKP_SCORE_MAX_POSES); return OKP_EINVAL; }
  if (cap_kp < 1) { okp_set_error("%s: cap_kp = %d: the key-point log holds at least one record", fn, cap_kp); return OKP_EINVAL; }
  if (cap_pose < 1) { okp_set_error("%s: cap_pose = %d: the pose log holds at least one record", fn, cap_pose); return OKP_EINVAL; }
  if (!(match_radius > 0.0)) { okp_set_error("%s: match_radius must be positive (infinity: no gate)", fn); return OKP_EINVAL; }
  if (!(max_range > 0.0)) { okp_set_error("%s: max_range must be positive", fn); return OKP_EINVAL; }
  okp_camera c = {};
  if (cam) {
    if (cam->model != OKP_CAM_EQUIDISTANT && cam->model != OKP_CAM_RADTAN) { okp_set_error("%s: cam: unknown camera model %d", fn, cam->model); return OKP_EINVAL; }
    if (!(size_x > 0.0)) { okp_set_error("%s: size_x must be positive", fn); return OKP_EINVAL; }
    if (!(size_y > 0.0)) { okp_set_error("%s: size_y must be positive", fn); return OKP_EINVAL; }
    c = *cam;
  }
  const struct { const void* p; const char* name; } required[] = {
      {tab_dev, "tab"}, {n_obj_dev, "n_obj"}, {truth_dev, "truth"}, {n_truth_dev, "n_truth"}, {kp_err_dev, "kp_err"}, {kp_id_dev, "kp_id"},
      {pose_err_dev, "pose_err"}, {pose_id_dev, "pose_id"}, {counts_dev, "counts"}, {match_dev, "match"}, {nearest_dev, "nearest"},
      {stage_f_dev, "stage_f"}, {stage_i_dev, "stage_i"}};
  for (const auto& r : required)
    if (!r.p) { okp_set_error("%s: null %s", fn, r.name); return OKP_EINVAL; }
  ScoreSets sets = {};
  if (P > 0) {
    if (!set_pose_dev) { okp_set_error("%s: null set_pose with P = %d", fn, P); return OKP_EINVAL; }
    if (!set_index_dev) { okp_set_error("%s: null set_index with P = %d (an array of P pointers, each of which may be null)", fn, P); return OKP_EINVAL; }
    if (!set_rows) { okp_set_error("%s: null set_rows with P = %d", fn, P); return OKP_EINVAL; }
    if (!truth_pose_dev) { okp_set_error("%s: null truth_pose with P = %d", fn, P); return OKP_EINVAL; }
    if (!model_dev) { okp_set_error("%s: null model with P = %d", fn, P); return OKP_EINVAL; }
    for (int p = 0; p < P; ++p) {
      if (!set_pose_dev[p]) { okp_set_error("%s: null set_pose[%d]", fn, p); return OKP_EINVAL; }
      if (set_rows[p] < 1) { okp_set_error("%s: set_rows[%d] = %d: a set has at least one row per frame", fn, p, set_rows[p]); return OKP_EINVAL; }
      if (!set_index_dev[p] && set_rows[p] != max_obj) {
        okp_set_error("%s: set_rows[%d] = %d without set_index[%d]: row o is taken, so the set has max_obj = %d rows", fn, p, set_rows[p], p, max_obj);
        return OKP_EINVAL;
      }
      sets.pose[p] = set_pose_dev[p]; sets.index[p] = set_index_dev[p]; sets.rows[p] = set_rows[p];
    }
  }
  const double radius2 = match_radius * match_radius;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(okp_score_frames_kernel, dim3(B), dim3(kWave), 0, st, tab_dev, n_obj_dev, truth_dev, n_truth_dev, max_obj, G, S, cam ? 1 : 0, c, size_x,
                     size_y, sets, P, truth_pose_dev, model_dev, radius2, max_range, match_dev, nearest_dev, stage_f_dev, stage_i_dev);
  if (int rc = okp_check_hip(hipGetLastError(), "okp_score_objects launch")) return rc;
  hipLaunchKernelGGL(okp_score_log_kernel, dim3(1), dim3(kLogThreads), 0, st, stage_f_dev, stage_i_dev, match_dev, B, max_obj, S, kp_err_dev, kp_id_dev, cap_kp,
                     pose_err_dev, pose_id_dev, cap_pose, reinterpret_cast<long long*>(counts_dev));
  return okp_check_hip(hipGetLastError(), "okp_score_objects log launch");
}
