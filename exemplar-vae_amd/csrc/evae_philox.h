// Counter-based generator (Philox4x32-10: Salmon, Moraes, Dror, Shaw, SC'11) shared by the step's prologue (evae_loss.hip) and the
// dropout masks (evae_attn.hip): a (counter, key) pair always gives the same 128 random bits, whatever the launch geometry, so a
// mask is regenerated in a backward pass instead of being stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace evae {

__device__ __forceinline__ uint4 philox4x32(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}
__device__ __forceinline__ float u01(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }          // [0, 1)
__device__ __forceinline__ float u01_open(uint32_t r) { return (float)((r >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]

}  // namespace evae
