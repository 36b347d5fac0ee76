// What the two sliding-window pushes share (csrc/okp_window.hip: one camera, one wave per slot; csrc/okp_window_views.hip: a rig, 256 threads per
// slot): whose ring a slot's is and whether it is emptied or pushed to, the ages of its columns, and what a push leaves behind - the control
// words, n_views, the start of the refinement; on the host the scalar refusals of their entry points.  How the new column is formed, the
// parameter structs, the barriers and the launches are each file's own: nothing here synchronises, and every thread of a slot calls every
// function here (the decisions are the same in all of them: they read the same words).
// fp64, no atomics, contraction off; the same bits as tests/window_spec.py and tests/window_views_spec.py.
#pragma once
#include "okp_pose_math.h"           // finite64, NamedArg / require_args: the walk over an entry point's table of pointers

#pragma clang fp contract(off)

namespace {

// Steps 1 - 4 of the contract (include/okp.h) for slot bi = b * T + i: the ring is emptied (clear) when the slot is free, has a new owner,
// holds corrupt control words or the track is faster than max_speed; there is a column to push when the track was measured by an object o whose
// pose has status 0 under a finite frame pose T [B][12].  owner, head, filled: the control words after the resets, before the push
struct RingStep { int id, o, owner, head, filled; bool clear, push; };

__device__ __forceinline__ RingStep ring_step(const int32_t* track_i, const int32_t* wi, const double* track_f, const int32_t* meas_of, const int32_t* status,
                                              const double* T, size_t bi, size_t b, int32_t max_obj, int W, double max_speed2) {
  RingStep r;
  r.id = track_i[bi * 4];
  r.owner = wi[0]; r.head = wi[1]; r.filled = wi[2];
  r.clear = false; r.push = false;
  r.o = -1;
  if (r.id == 0) {
    r.clear = true; r.owner = 0; r.head = 0; r.filled = 0;
  } else {
    if (r.id != r.owner || r.head < 0 || r.head >= W || r.filled < 0 || r.filled > W) { r.clear = true; r.owner = r.id; r.head = 0; r.filled = 0; }
    const double* f = track_f + bi * 16;
    const double vx = f[3], vy = f[4], vz = f[5];
    if ((vx * vx + vy * vy) + vz * vz > max_speed2) { r.clear = true; r.head = 0; r.filled = 0; }
    // 4: is there a column to push
    r.o = meas_of[bi];
    if (r.o >= 0 && r.o < max_obj && status[b * max_obj + r.o] == 0) {
      r.push = true;
#pragma unroll
      for (int k = 0; k < 12; ++k) r.push = r.push && finite64(T[b * 12 + k]);
    }
  }
  return r;
}

// The ages of a timed ring, V views to each of its columns: a pushed column is 0 ticks old, a free slot's are 0, every other one a tick older
__device__ __forceinline__ void ring_age(int32_t* ages, int tid, int threads, int columns, int V, const RingStep& r) {
  for (int cv = tid; cv < columns * V; cv += threads) {
    const int32_t old = r.clear ? 0 : ages[cv];
    ages[cv] = (r.push && cv / V == r.head) || r.id == 0 ? 0 : (old < (1 << 30) ? old + 1 : (1 << 30));
  }
}

// After the ring's pass: the head and the count move on a push, thread 0 leaves the control words and n_views, threads 0 .. 11 the start of the
// refinement - the track pose bit for bit from min_views columns on, otherwise NaN - and, TIMED, threads 0 .. 2 the track's velocity likewise
template <bool TIMED>
__device__ __forceinline__ void ring_finish(RingStep r, int tid, size_t bi, int W, int min_views, int32_t* wi, int32_t* n_views, const double* track_pose,
                                            double* start, const double* track_f, double* start_velocity) {
  const double nan = __builtin_nan("");
  if (r.push) { r.head = r.head + 1 == W ? 0 : r.head + 1; r.filled = r.filled < W ? r.filled + 1 : W; }

  if (tid == 0) { wi[0] = r.owner; wi[1] = r.head; wi[2] = r.filled; wi[3] = 0; n_views[bi] = r.filled; }
  if (tid < 12) {
    const unsigned long long bits = reinterpret_cast<const unsigned long long*>(track_pose)[bi * 12 + tid];
    if (r.filled >= min_views) reinterpret_cast<unsigned long long*>(start)[bi * 12 + tid] = bits;
    else start[bi * 12 + tid] = nan;
  }
  if constexpr (TIMED) {
    if (tid < 3) {
      const unsigned long long bits = reinterpret_cast<const unsigned long long*>(track_f)[bi * 16 + 3 + tid];
      if (r.filled >= min_views) reinterpret_cast<unsigned long long*>(start_velocity)[bi * 3 + tid] = bits;
      else start_velocity[bi * 3 + tid] = nan;
    }
  }
}

// The scalar refusals of the six entry points, in the order they have always been made.  V = null: one camera; otherwise the cameras of a rig,
// checked after T, and W * V after W
int window_scalars(const char* fn, int32_t B, int32_t max_obj, int32_t S, int32_t T, int32_t W, const int32_t* V, int32_t min_views, double max_speed) {
  if (B < 1) { okp_set_error("%s: B = %d; at least one stream", fn, B); return OKP_EINVAL; }
  if (max_obj < 1) { okp_set_error("%s: max_obj = %d; a stream holds at least one object", fn, max_obj); return OKP_EINVAL; }
  if (S < 1 || S > OKP_POSE_MAX_POINTS) { okp_set_error("%s: S = %d outside [1, %d] model points", fn, S, OKP_POSE_MAX_POINTS); return OKP_EINVAL; }
  if (T < 1 || T > OKP_TRACK_MAX_TRACKS) { okp_set_error("%s: T = %d outside [1, %d] track slots", fn, T, OKP_TRACK_MAX_TRACKS); return OKP_EINVAL; }
  if (V && (*V < 1 || *V > 2 * OKP_RIG_MAX_PAIRS)) { okp_set_error("%s: V = %d outside [1, %d] cameras", fn, *V, 2 * OKP_RIG_MAX_PAIRS); return OKP_EINVAL; }
  if (W < 1 || W > OKP_REFINE_MAX_VIEWS) { okp_set_error("%s: W = %d outside [1, %d] ticks", fn, W, OKP_REFINE_MAX_VIEWS); return OKP_EINVAL; }
  if (V && W * *V > OKP_REFINE_WIDE_MAX_VIEWS) {
    okp_set_error("%s: W * V = %d x %d = %d views exceed the %d of okp_refine_pose_views_wide", fn, W, *V, W * *V, OKP_REFINE_WIDE_MAX_VIEWS);
    return OKP_EINVAL;
  }
  if (min_views < 1 || min_views > W) { okp_set_error("%s: min_views = %d outside [1, W = %d]", fn, min_views, W); return OKP_EINVAL; }
  if (!(max_speed > 0.0)) { okp_set_error("%s: max_speed = %g must be positive (metres per second; +inf: never reset)", fn, max_speed); return OKP_EINVAL; }
  if ((long long)B * T > 0x7fffffffll) { okp_set_error("%s: B * T = %lld track slots do not fit one launch", fn, (long long)B * T); return OKP_EINVAL; }
  return OKP_OK;
}

}  // namespace
