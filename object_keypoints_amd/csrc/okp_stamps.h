// Shader-clock stamps of the one-launch fire kernels (okp_fire2, okp_fire_chain, okp_fire_x3): the project's in-kernel instrument.
// Debug build only - OKP_EXTRA_CFLAGS=-DOKP_FIRE_STAMPS, printed with OKP_FIRE_STAMPS_PRINT=1 (scripts/probe_fire2.py) - and included only
// under that switch.  Every wave of workgroups 0..15 writes its clock at up to eight points: [wg 16][wave 8][slot 8] u32 behind the
// kernel parameter `dbg`; each kernel file keeps the printout of its own phases.
#ifndef OKP_STAMPS_H
#define OKP_STAMPS_H

#include <cstdint>
#include <cstdlib>

#include <hip/hip_runtime.h>

// in a kernel with `lane`, the wave index `w` and the parameters `p` in scope: slot i of a workgroup of nw waves, where cond holds
#define OKP_FIRE_STAMP(cond, nw, i) do { if ((cond) && lane == 0 && blockIdx.x < 16) { uint64_t t_; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); p.dbg[(blockIdx.x * (nw) + w) * 8 + (i)] = (uint32_t)t_; } } while (0)

// the launcher's side: one per kernel family (a function-local static); the buffer lives as long as the process
struct OkpFireStamps {
  static constexpr int kWords = 16 * 8 * 8;
  uint32_t* dev = nullptr;
  uint32_t* reset(hipStream_t stream) {            // zeroed in stream order, in front of the launch that gets it as p.dbg
    if (!dev) (void)hipMalloc((void**)&dev, kWords * 4);
    (void)hipMemsetAsync(dev, 0, kWords * 4, stream);
    return dev;
  }
  bool fetch(uint32_t (&h)[kWords], hipStream_t stream) const {   // false unless a printout is asked for; waits for the stream
    if (!getenv("OKP_FIRE_STAMPS_PRINT")) return false;
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost);
    return true;
  }
};

#endif  // OKP_STAMPS_H
