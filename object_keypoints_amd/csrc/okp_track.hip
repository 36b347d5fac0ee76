// Object tracking across ticks (okp_track_objects; contract in include/okp.h): the poses of one tick's objects -> stable ids and filtered
// poses, with the tracker's state in device memory between the calls.
//
// The work is a handful of objects per stream, so the stage is latency-bound: one wave per stream, everything in registers, no LDS traffic
// inside a stream, no atomics, no host wait.  One workgroup of min(B, 8) waves; wave w steps streams w, w + 8, ...; the only word the
// streams share, `overflow`, is folded through LDS and written by one thread (which is also why overflow_in may be the same address).
//
//   lane o = measurement o (its kind, z and - through the pose rows in memory - R_meas), lane i = track slot i, both at once.
//   (2-3) every unmatched live track scans the free measurements for its nearest one inside the gate (z comes by v_readlane: the scan's
//         index is uniform); one butterfly over (d2, slot) accepts the global best - the track's own scan already took the lowest object index
//         on equal d2; a track scans again only when the measurement it had chosen went to another track.
//   (4-5) the lane updates or coasts its own track, (6) free slots and unmatched full measurements find each other by their ranks in two
//         ballots.
// All of it with contraction off, so that every decision is the one NumPy takes on the same numbers.
#include "okp_internal.h"

#pragma clang fp contract(off)

#define OKP_TRACK_WAVES 8
static_assert(OKP_TRACK_MAX_TRACKS == 64 && OKP_TRACK_MAX_OBJECTS == 64, "one lane per track slot and per measurement");

namespace {

struct TrackParams {
  const double* tab; const double* pose; const int32_t* status; const int32_t* n_obj; const double* model; const int32_t* overflow_in;
  int32_t B, max_obj, S, T, max_misses;
  double gate2, dt, alpha, beta_dt, alpha_R;
  double* track_f; int32_t* track_i; int32_t* next_id;
  double* track_pose; int32_t* track_of; int32_t* meas_of; int32_t* n_tracks; int32_t* overflow;
};

__device__ __forceinline__ bool finite64(double x) { return fabs(x) < __builtin_inf(); }      // (false for NaN)

// the index of the r-th set bit of m, ascending (r < popcount(m))
__device__ __forceinline__ int nth_bit(unsigned long long m, int r) {
  for (int q = 0; q < r; ++q) m &= m - 1ull;
  return __builtin_ctzll(m);
}

__device__ __forceinline__ int sat_inc(int v) { return v == 0x7fffffff ? v : v + 1; }

// R_meas of object row `row`: the rotation of a row-major [R | t]
__device__ __forceinline__ void load_rotation(const double* row, double (&M)[9]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) { M[3 * a + 0] = row[4 * a + 0]; M[3 * a + 1] = row[4 * a + 1]; M[3 * a + 2] = row[4 * a + 2]; }
}

// step 4, full measurement, alpha_R < 1: R <- R exp(alpha_R log(R^T M))
__device__ void blend_rotation(double (&R)[9], const double (&M)[9], double alpha_R) {
  double Q[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[3 * a + c] = (R[a] * M[c] + R[3 + a] * M[3 + c]) + R[6 + a] * M[6 + c];
  const double w0 = Q[7] - Q[5], w1 = Q[2] - Q[6], w2 = Q[3] - Q[1];
  const double s = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  if (s <= 1e-9) {                                               // the rotations agree, or a half turn whose axis the data do not give
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = M[i];
    return;
  }
  const double theta = atan2(s * 0.5, (((Q[0] + Q[4]) + Q[8]) - 1.0) * 0.5);
  const double u0 = w0 / s, u1 = w1 / s, u2 = w2 / s;
  const double phi = alpha_R * theta;
  const double sn = sin(phi), vs = 1.0 - cos(phi);
  const double K[9] = {0.0, -u2, u1, u2, 0.0, -u0, -u1, u0, 0.0};
  double E[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double k2 = (K[3 * a] * K[c] + K[3 * a + 1] * K[3 + c]) + K[3 * a + 2] * K[6 + c];
      E[3 * a + c] = ((a == c ? 1.0 : 0.0) + sn * K[3 * a + c]) + vs * k2;
    }
  double N[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) N[3 * a + c] = (R[3 * a] * E[c] + R[3 * a + 1] * E[3 + c]) + R[3 * a + 2] * E[6 + c];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = N[i];
}

__global__ __launch_bounds__(64 * OKP_TRACK_WAVES) void okp_track_objects_kernel(const TrackParams P) {
  __shared__ int32_t wave_bits[OKP_TRACK_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  const unsigned long long below = (1ull << lane) - 1ull;
  const double m0x = P.model[0], m0y = P.model[1], m0z = P.model[2];
  int32_t bits = 0;

  for (int b = wave; b < P.B; b += n_waves) {                     // (uniform per wave: every lane of the wave steps the same stream)
    // (0) lane o: measurement o
    const int n = min(max(P.n_obj[b], 0), P.max_obj);
    int kind = 0;                                                 // 0 none, 1 position-only, 2 full
    double zx = 0.0, zy = 0.0, zz = 0.0;
    if (lane < n) {
      const size_t row = (size_t)b * P.max_obj + lane;
      const double* ps = P.pose + row * 12;
      bool full = P.status[row] == 0;
      double q[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) { q[i] = ps[i]; full = full && finite64(q[i]); }
      if (full) {
        kind = 2;
        zx = q[3] + ((q[0] * m0x + q[1] * m0y) + q[2] * m0z);
        zy = q[7] + ((q[4] * m0x + q[5] * m0y) + q[6] * m0z);
        zz = q[11] + ((q[8] * m0x + q[9] * m0y) + q[10] * m0z);
      } else {
        const double* c = P.tab + row * P.S * 4;
        const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        if (finite64(c0) && finite64(c1) && finite64(c2) && finite64(c3)) { kind = 1; zx = c0; zy = c1; zz = c2; }
      }
    }
    const unsigned long long full_mask = __ballot(kind == 2);
    unsigned long long avail = __ballot(kind != 0);               // measurements no track has taken yet

    // (1) lane i: track slot i, predicted
    const bool slot = lane < P.T;
    double* tf = P.track_f + ((size_t)b * P.T + lane) * 16;
    int32_t* ti = P.track_i + ((size_t)b * P.T + lane) * 4;
    double c[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int id = 0, hits = 0, misses = 0, age = 0;
    if (slot) {
      id = ti[0]; hits = ti[1]; misses = ti[2]; age = ti[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { c[i] = tf[i]; v[i] = tf[3 + i]; }
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = tf[6 + i];
    }
    const bool was_live = slot && id != 0;
    const double px = c[0] + P.dt * v[0], py = c[1] + P.dt * v[1], pz = c[2] + P.dt * v[2];

    // (2-3) greedy association
    int my_meas = -1, my_track = -1;                              // the measurement of track `lane`; the track of measurement `lane`
    bool searching = was_live, scan = was_live;
    double best_d = inf;
    int best_o = -1;
    for (;;) {
      if (__any(scan)) {                                          // (uniform: the shuffles below read every lane; a second scan of a track whose
        best_d = inf; best_o = -1;                                //  choice is still free finds that choice again)
        for (unsigned long long m = avail; m; m &= m - 1ull) {    // ascending o, strict <: the lower object index on equal d2
          const int o = __builtin_ctzll(m);
          const double dx = __shfl(zx, o) - px, dy = __shfl(zy, o) - py, dz = __shfl(zz, o) - pz;
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 <= P.gate2 && d2 < best_d) { best_d = d2; best_o = o; }
        }
        scan = false;
      }
      double wd = best_d;
      int wi = (searching && best_o >= 0) ? lane : 64, wo = best_o;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(wd, off);
        const int oi = __shfl_xor(wi, off), oo = __shfl_xor(wo, off);
        if (oi < 64 && (wi == 64 || od < wd || (od == wd && oi < wi))) { wd = od; wi = oi; wo = oo; }
      }
      if (wi == 64) break;                                        // (uniform: the butterfly leaves the same triple in every lane)
      avail &= ~(1ull << wo);
      if (lane == wo) my_track = wi;
      if (lane == wi) { my_meas = wo; searching = false; best_o = -1; }
      else if (searching && best_o == wo) scan = true;
    }

    // (4) matched, (5) unmatched
    const int src = my_meas >= 0 ? my_meas : 0;
    const double mzx = __shfl(zx, src), mzy = __shfl(zy, src), mzz = __shfl(zz, src);
    if (was_live) {
      if (my_meas >= 0) {
        const double rx = mzx - px, ry = mzy - py, rz = mzz - pz;
        c[0] = px + P.alpha * rx; c[1] = py + P.alpha * ry; c[2] = pz + P.alpha * rz;
        v[0] = v[0] + P.beta_dt * rx; v[1] = v[1] + P.beta_dt * ry; v[2] = v[2] + P.beta_dt * rz;
        hits = sat_inc(hits); age = sat_inc(age); misses = 0;
        if ((full_mask >> my_meas) & 1ull) {
          double M[9];
          load_rotation(P.pose + ((size_t)b * P.max_obj + my_meas) * 12, M);
          if (P.alpha_R == 1.0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = M[i];
          } else {
            blend_rotation(R, M, P.alpha_R);
          }
        }
      } else {
        c[0] = px; c[1] = py; c[2] = pz;
        misses = sat_inc(misses); age = sat_inc(age);
        if (misses > P.max_misses) {
          id = hits = misses = age = 0;
#pragma unroll
          for (int i = 0; i < 3; ++i) { c[i] = 0.0; v[i] = 0.0; }
#pragma unroll
          for (int i = 0; i < 9; ++i) R[i] = 0.0;
        }
      }
    }

    // (6) births: the k-th unmatched full measurement takes the k-th free slot
    const unsigned long long free_mask = __ballot(slot && id == 0);
    const unsigned long long birth_mask = __ballot(kind == 2 && my_track < 0);
    const int n_free = __popcll(free_mask), n_birth = __popcll(birth_mask);
    const int next = P.next_id[b];
    const int my_rank = __popcll(free_mask & below);
    const bool born = slot && id == 0 && my_rank < n_birth;
    const int founder = born ? nth_bit(birth_mask, my_rank) : 0;
    const double bzx = __shfl(zx, founder), bzy = __shfl(zy, founder), bzz = __shfl(zz, founder);
    if (born) {
      id = next + my_rank + 1;
      c[0] = bzx; c[1] = bzy; c[2] = bzz;
      load_rotation(P.pose + ((size_t)b * P.max_obj + founder) * 12, R);
      hits = 1; age = 1; misses = 0;
      my_meas = founder;
    }
    if ((birth_mask >> lane) & 1ull) {
      const int k = __popcll(birth_mask & below);
      my_track = k < n_free ? nth_bit(free_mask, k) : -1;
    }
    if (n_birth > n_free) bits |= OKP_TRACK_OVERFLOW;

    // outputs: every word is written by every call
    const bool live = slot && id != 0;
    if (slot) {
      ti[0] = id; ti[1] = hits; ti[2] = misses; ti[3] = age;
#pragma unroll
      for (int i = 0; i < 3; ++i) { tf[i] = c[i]; tf[3 + i] = v[i]; }
#pragma unroll
      for (int i = 0; i < 9; ++i) tf[6 + i] = R[i];
      tf[15] = 0.0;
      double* tp = P.track_pose + ((size_t)b * P.T + lane) * 12;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        tp[4 * a + 0] = live ? R[3 * a + 0] : nan; tp[4 * a + 1] = live ? R[3 * a + 1] : nan; tp[4 * a + 2] = live ? R[3 * a + 2] : nan;
        tp[4 * a + 3] = live ? c[a] - ((R[3 * a] * m0x + R[3 * a + 1] * m0y) + R[3 * a + 2] * m0z) : nan;
      }
      P.meas_of[(size_t)b * P.T + lane] = my_meas;
    }
    if (lane < P.max_obj) P.track_of[(size_t)b * P.max_obj + lane] = my_track;
    const int n_live = __popcll(__ballot(live));
    if (lane == 0) {
      P.n_tracks[b] = n_live;
      P.next_id[b] = next + min(n_birth, n_free);
    }
  }

  if (lane == 0) wave_bits[wave] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t word = P.overflow_in ? *P.overflow_in : 0;
    for (int w = 0; w < n_waves; ++w) word |= wave_bits[w];
    *P.overflow = word;
  }
}

bool positive_finite(double x) { return x > 0.0 && x < __builtin_inf(); }

}  // namespace

extern "C" int okp_track_objects(const double* tab, const double* pose, const int32_t* status, const int32_t* n_obj, const double* model,
                                 int32_t B, int32_t max_obj, int32_t S, int32_t T, double gate, double dt, double alpha, double beta, double alpha_R,
                                 int32_t min_hits, int32_t max_misses, const int32_t* overflow_in, double* track_f, int32_t* track_i, int32_t* next_id,
                                 double* track_pose, int32_t* track_of, int32_t* meas_of, int32_t* n_tracks, int32_t* overflow, void* stream) {
  const char* fn = "okp_track_objects";
  if (B < 1) { okp_set_error("%s: B = %d; a tracker holds at least one stream", fn, B); return OKP_EINVAL; }
  if (max_obj < 1 || max_obj > OKP_TRACK_MAX_OBJECTS) { okp_set_error("%s: max_obj = %d outside [1, %d] (one lane per measurement)", fn, max_obj, OKP_TRACK_MAX_OBJECTS); return OKP_EINVAL; }
  if (S < 1 || S > OKP_POSE_MAX_POINTS) { okp_set_error("%s: S = %d outside [1, %d] model points", fn, S, OKP_POSE_MAX_POINTS); return OKP_EINVAL; }
  if (T < 1 || T > OKP_TRACK_MAX_TRACKS) { okp_set_error("%s: T = %d outside [1, %d] (one lane per track slot)", fn, T, OKP_TRACK_MAX_TRACKS); return OKP_EINVAL; }
  if (!positive_finite(gate)) { okp_set_error("%s: gate = %g must be a positive, finite length in metres", fn, gate); return OKP_EINVAL; }
  if (!positive_finite(dt)) { okp_set_error("%s: dt = %g must be a positive, finite tick period in seconds", fn, dt); return OKP_EINVAL; }
  if (!(alpha > 0.0 && alpha <= 1.0)) { okp_set_error("%s: alpha = %g outside (0, 1]", fn, alpha); return OKP_EINVAL; }
  if (!(beta >= 0.0 && beta < __builtin_inf())) { okp_set_error("%s: beta = %g must be finite and not negative", fn, beta); return OKP_EINVAL; }
  if (!(alpha_R > 0.0 && alpha_R <= 1.0)) { okp_set_error("%s: alpha_R = %g outside (0, 1]", fn, alpha_R); return OKP_EINVAL; }
  if (min_hits < 1) { okp_set_error("%s: min_hits = %d below 1", fn, min_hits); return OKP_EINVAL; }
  if (max_misses < 0) { okp_set_error("%s: max_misses = %d is negative", fn, max_misses); return OKP_EINVAL; }
  const struct { const void* p; const char* name; } required[] = {
      {tab, "tab"}, {pose, "pose"}, {status, "status"}, {n_obj, "n_obj"}, {model, "model"}, {track_f, "track_f"}, {track_i, "track_i"}, {next_id, "next_id"},
      {track_pose, "track_pose"}, {track_of, "track_of"}, {meas_of, "meas_of"}, {n_tracks, "n_tracks"}, {overflow, "overflow"}};
  for (const auto& r : required)
    if (!r.p) { okp_set_error("%s: null %s", fn, r.name); return OKP_EINVAL; }
  TrackParams p = {};
  p.tab = tab; p.pose = pose; p.status = status; p.n_obj = n_obj; p.model = model; p.overflow_in = overflow_in;
  p.B = B; p.max_obj = max_obj; p.S = S; p.T = T; p.max_misses = max_misses;
  p.gate2 = gate * gate; p.dt = dt; p.alpha = alpha; p.beta_dt = beta / dt; p.alpha_R = alpha_R;
  p.track_f = track_f; p.track_i = track_i; p.next_id = next_id;
  p.track_pose = track_pose; p.track_of = track_of; p.meas_of = meas_of; p.n_tracks = n_tracks; p.overflow = overflow;
  const int waves = B < OKP_TRACK_WAVES ? B : OKP_TRACK_WAVES;
  hipLaunchKernelGGL(okp_track_objects_kernel, dim3(1), dim3(64 * waves), 0, (hipStream_t)stream, p);
  return okp_check_hip(hipGetLastError(), "okp_track_objects launch");
}
