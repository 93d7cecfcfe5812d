// KV4 dequantisation shared by the kernels that read the paged cache (decode attention: kv_cache.hip; prefill attention over
// the pages: attn_prefill_paged.hip).
#pragma once
#include "common.h"

namespace omni {

// unpack 16 packed bytes (32 codes) and dequantise with fp16 fma(u, scale, c), c = h(-scale*zero).
// Output order per 32-bit word of 8 codes e0..e7: half2 pairs (e0,e4) (e1,e5) (e2,e6) (e3,e7),
// i.e. out[w*4 + j] = {e_j, e_{j+4}} of word w (the q operand is loaded in the same order).
// (x & mask) | magic in one VALU op.  VOP3 on gfx9 takes one scalar operand, so the magic lives in a VGPR; the
// compiler emits v_and + v_or with two literals otherwise (64 extra ops per 32-token tile of the decode kernels).
__device__ __forceinline__ uint32_t and_or(uint32_t x, uint32_t mask, uint32_t magic) {
  uint32_t r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(mask), "v"(magic));
  return r;
}

template <bool CHEAP = false>
__device__ __forceinline__ void kv4_dequant16(const uint4 raw, v2h scale2, v2h c2, v2h out[16]) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  if constexpr (CHEAP) {      // (timing experiments only: 16 instead of 52 operations, no dependent chains)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = __builtin_bit_cast(v2h, w[i & 3]) * scale2;
    return;
  }
  const v2h k1024 = {(half_t)1024.0f, (half_t)1024.0f};
  const v2h k16th = {(half_t)0.0625f, (half_t)0.0625f};
  const v2h k64 = {(half_t)64.0f, (half_t)64.0f};
  const uint32_t magic = 0x64006400u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = w[i], y = w[i] >> 8;
    uint32_t h0 = and_or(x, 0x000f000fu, magic);  // {1024+e0, 1024+e4}
    uint32_t h1 = and_or(x, 0x00f000f0u, magic);  // {1024+16 e1, 1024+16 e5}
    uint32_t h2 = and_or(y, 0x000f000fu, magic);  // e2, e6
    uint32_t h3 = and_or(y, 0x00f000f0u, magic);  // e3, e7
    v2h u0 = __builtin_bit_cast(v2h, h0) - k1024;
    v2h u1 = __builtin_elementwise_fma(__builtin_bit_cast(v2h, h1), k16th, -k64);
    v2h u2 = __builtin_bit_cast(v2h, h2) - k1024;
    v2h u3 = __builtin_elementwise_fma(__builtin_bit_cast(v2h, h3), k16th, -k64);
    out[i * 4 + 0] = __builtin_elementwise_fma(u0, scale2, c2);
    out[i * 4 + 1] = __builtin_elementwise_fma(u1, scale2, c2);
    out[i * 4 + 2] = __builtin_elementwise_fma(u2, scale2, c2);
    out[i * 4 + 3] = __builtin_elementwise_fma(u3, scale2, c2);
  }
}

}  // namespace omni
