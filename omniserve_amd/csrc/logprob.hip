// Log-probabilities for MI355X (gfx950): per logits row the log-sum-exp, one token's log-probability and rank, and the top-n
// tokens with theirs -- under the RAW distribution of the row (no temperature, no filter).
//
// Stands in for what the reference never computes: SamplingParams.logprobs / prompt_logprobs are accepted
// (omniserve/sampling_params.py:69-75) and carried (Sequence.append_token_id, SequenceOutput.logprobs) but its sampler fills
// none of them.  The contract is DESIGN.md section 4.6a; tests/logprob_cases.py holds its f64 oracle.
//
// Two launches, no state between calls, nothing to zero:
//   logprob_chunk_kernel  (chunks, rows): a workgroup walks its chunk of the row three ways.  (1) the chunk's maximum as the
//       arg-max kernel's 64-bit key (orderable fp16 bits << 32 | ~index); (2) the sum of exp(x - chunk maximum) as 2^40 fixed
//       point (the sampler's: integer sums do not depend on the order in which lanes and waves add) and the number of tokens in
//       front of the target in the canonical order (a key comparison); (3) n_top times "the largest key below the previous
//       one": the chunk's first n_top tokens in the canonical order.  With n_top == 0 part (3) does not run.
//   logprob_final_kernel  (rows): one wave merges the chunks in chunk order -- maximum of the maxima, sum of the chunk sums
//       rescaled by exp(chunk maximum - row maximum) in f64 over a fixed tree, sum of the counts, n_top times the largest of
//       the chunks' candidates -- and writes lse = max + ln(sum), (x - max) - ln(sum) per token, the rank.
// Order and rank are integer comparisons only; the floating-point steps are per token its weight and per row 32 products, one
// sum tree and one logarithm, so the bits depend on the row's values and on cols (the chunk geometry), not on the grid, the
// layout, the slice of rows or n_top.
#include "common.h"
#include "omniserve_hip.h"

namespace omni {

constexpr int LOGPROB_CHUNKS = 32;
constexpr int LOGPROB_THREADS = 256;
constexpr int LOGPROB_MAX_COLS = 1 << 22;
constexpr int LOGPROB_MAX_TOP = 20;
constexpr uint32_t LP_KEY_POS_INF = 0xFC00u;      // keys >= this: +inf and the NaNs that arg-max treats as the maximum
constexpr uint32_t LP_KEY_NEG_INF = 0x03FFu;      // keys <= this: -inf (and negative NaNs below it): weight 0

// argmax_key of elementwise.hip / sample_key of sampling.hip: -0 == +0, positive NaN above +inf, negative NaN below -inf
__device__ __forceinline__ uint32_t lp_key(uint32_t h16) {
  uint32_t h = h16 & 0xFFFFu;
  if (h == 0x8000u) h = 0;
  return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
__device__ __forceinline__ unsigned long long lp_key64(uint32_t h16, uint32_t idx) {
  return ((unsigned long long)lp_key(h16) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
__device__ __forceinline__ uint32_t lp_half_bits(half_t v) { return __builtin_bit_cast(uint16_t, v); }
__device__ __forceinline__ float lp_key_value(uint32_t key) {
  const uint16_t h = (uint16_t)((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
  return (float)__builtin_bit_cast(half_t, h);
}
// ONE definition of exp(a - b) for finite a <= b (a token against its chunk's maximum, a chunk's maximum against the row's)
__device__ __forceinline__ float lp_exp_diff(float a, float b) { return __builtin_amdgcn_exp2f((a - b) * 1.4426950408889634f); }

__device__ __forceinline__ unsigned long long lp_shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lp_wave_max(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long o = lp_shfl_xor_u64(v, m);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long lp_wave_sum(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += lp_shfl_xor_u64(v, m);
  return v;
}
// 256 threads, red: LDS [4]; every thread gets the result
__device__ __forceinline__ unsigned long long lp_block_max(unsigned long long v, unsigned long long* red) {
  v = lp_wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < LOGPROB_THREADS / 64; ++w) r = red[w] > r ? red[w] : r;
  __syncthreads();
  return r;
}
__device__ __forceinline__ unsigned long long lp_block_sum(unsigned long long v, unsigned long long* red) {
  v = lp_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < LOGPROB_THREADS / 64; ++w) r += red[w];
  __syncthreads();
  return r;
}

// f(fp16 bits, column) for every column of [c0, c1); 16-byte loads where the row layout allows (as the arg-max kernel)
template <class F>
__device__ __forceinline__ void lp_for_each(const half_t* xr, int c0, int c1, bool vec, F&& f) {
  if (vec) {
    for (int c = c0 + 8 * (int)threadIdx.x; c < c1; c += 8 * LOGPROB_THREADS) {
      if (c + 8 <= c1) {
        const uint4 v = *reinterpret_cast<const uint4*>(xr + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f(w[j] & 0xFFFFu, c + 2 * j);
          f(w[j] >> 16, c + 2 * j + 1);
        }
      } else {
        for (int e = c; e < c1; ++e) f(lp_half_bits(xr[e]), e);
      }
    }
  } else {
    for (int e = c0 + (int)threadIdx.x; e < c1; e += LOGPROB_THREADS) f(lp_half_bits(xr[e]), e);
  }
}

struct LogprobArgs {
  const half_t* x;
  int64_t row_stride;
  int cols, n_top;
  const long long* target;
  float* lse;
  float* token_logprob;
  int* rank;
  long long* top_token;
  float* top_logprob;
  unsigned long long* part_key;      // [rows][LOGPROB_CHUNKS]  the chunk's largest key64 (0: the chunk is empty)
  unsigned long long* part_sum;      // [rows][LOGPROB_CHUNKS]  sum of exp(x - chunk maximum) * 2^40
  uint32_t* part_cnt;                // [rows][LOGPROB_CHUNKS]  tokens in front of the target
  unsigned long long* cand;          // [rows][LOGPROB_CHUNKS][n_top]  the chunk's first n_top key64s, descending (0: none)
};

__device__ __forceinline__ int lp_per(int cols) { return ((cols + LOGPROB_CHUNKS - 1) / LOGPROB_CHUNKS + 7) & ~7; }

__global__ __launch_bounds__(LOGPROB_THREADS) void logprob_chunk_kernel(LogprobArgs a) {
  __shared__ unsigned long long red[LOGPROB_THREADS / 64];
  const int row = blockIdx.y, chunk = blockIdx.x;
  const int per = lp_per(a.cols);
  const int c0 = chunk * per, c1 = min(a.cols, c0 + per);      // (c0 >= cols: an empty chunk, every loop below is empty)
  const half_t* xr = a.x + (size_t)row * a.row_stride;
  const bool vec = (a.row_stride % 8) == 0 && (reinterpret_cast<uintptr_t>(a.x) % 16) == 0;
  const size_t slot = (size_t)row * LOGPROB_CHUNKS + chunk;

  unsigned long long best = 0ull;
  lp_for_each(xr, c0, c1, vec, [&](uint32_t h, int c) {
    const unsigned long long k = lp_key64(h, (uint32_t)c);
    best = k > best ? k : best;
  });
  best = lp_block_max(best, red);
  const uint32_t mkey = (uint32_t)(best >> 32);
  // a chunk whose maximum is NaN / +inf makes the row degenerate, one with nothing above -inf weighs nothing: no sum
  const bool summed = best != 0ull && mkey < LP_KEY_POS_INF && mkey > LP_KEY_NEG_INF;
  const float vmax = lp_key_value(mkey);

  unsigned long long tkey = ~0ull;      // nothing is in front of a target outside the row
  if (a.target) {
    const long long t = a.target[row];
    if (t >= 0 && t < a.cols) tkey = lp_key64(lp_half_bits(xr[t]), (uint32_t)t);
  }
  unsigned long long sum = 0ull, cnt = 0ull;
  lp_for_each(xr, c0, c1, vec, [&](uint32_t h, int c) {
    const uint32_t key = lp_key(h);
    if (summed && key > LP_KEY_NEG_INF) sum += (unsigned long long)(lp_exp_diff(lp_key_value(key), vmax) * 1099511627776.0f);
    cnt += lp_key64(h, (uint32_t)c) > tkey ? 1ull : 0ull;
  });
  sum = lp_block_sum(sum, red);
  cnt = lp_block_sum(cnt, red);
  if (threadIdx.x == 0) {
    a.part_key[slot] = best;
    a.part_sum[slot] = sum;
    a.part_cnt[slot] = (uint32_t)cnt;
  }

  unsigned long long prev = ~0ull;
  for (int j = 0; j < a.n_top; ++j) {      // (uniform: prev is the same in every thread)
    unsigned long long b = 0ull;
    if (prev != 0ull)
      lp_for_each(xr, c0, c1, vec, [&](uint32_t h, int c) {
        const unsigned long long k = lp_key64(h, (uint32_t)c);
        b = (k < prev && k > b) ? k : b;
      });
    prev = lp_block_max(b, red);
    if (threadIdx.x == 0) a.cand[slot * a.n_top + j] = prev;
  }
}

__device__ __forceinline__ double lp_wave_sum_f64(double v) {      // a fixed tree: the same bits in every lane, every run
#pragma unroll
  for (int m = 32; m > 0; m >>= 1)
    v += __builtin_bit_cast(double, lp_shfl_xor_u64(__builtin_bit_cast(unsigned long long, v), m));
  return v;
}

__global__ __launch_bounds__(64) void logprob_final_kernel(LogprobArgs a) {
  __shared__ unsigned long long cand[LOGPROB_CHUNKS * LOGPROB_MAX_TOP];
  const int row = blockIdx.x, lane = threadIdx.x;
  const half_t* xr = a.x + (size_t)row * a.row_stride;
  const size_t slot = (size_t)row * LOGPROB_CHUNKS + (lane & (LOGPROB_CHUNKS - 1));
  const bool mine = lane < LOGPROB_CHUNKS;
  const unsigned long long ckey = mine ? a.part_key[slot] : 0ull;
  const unsigned long long csum = mine ? a.part_sum[slot] : 0ull;
  const unsigned long long ccnt = mine ? a.part_cnt[slot] : 0ull;
  const uint32_t maxkey = (uint32_t)(lp_wave_max(ckey) >> 32);
  const bool degenerate = maxkey >= LP_KEY_POS_INF || maxkey <= LP_KEY_NEG_INF;
  const float vmax = lp_key_value(maxkey);
  double term = 0.0;
  if (!degenerate && csum != 0ull) term = (double)csum * (double)lp_exp_diff(lp_key_value((uint32_t)(ckey >> 32)), vmax);
  const double z = lp_wave_sum_f64(term) * (1.0 / 1099511627776.0);
  const float nan = __builtin_nanf("");
  // a log-probability is (x - max) - ln(sum), not x - lse: with a maximum of 65504 lse is good to 2^-9 only, and the tokens near
  // the maximum would inherit that
  const float ln_z = __builtin_logf((float)z);
  const float lse = degenerate ? nan : vmax + ln_z;
  const unsigned long long ahead = lp_wave_sum(ccnt);
  if (lane == 0) {
    if (a.lse) a.lse[row] = lse;
    if (a.token_logprob || a.rank) {
      const long long t = a.target[row];
      const bool in = t >= 0 && t < a.cols;
      if (a.token_logprob) a.token_logprob[row] = (in && !degenerate) ? ((float)xr[in ? t : 0] - vmax) - ln_z : nan;
      if (a.rank) a.rank[row] = in ? (int)ahead + 1 : 0;
    }
  }
  if (a.n_top == 0) return;
  const int n_cand = LOGPROB_CHUNKS * a.n_top;
  for (int i = lane; i < n_cand; i += 64) cand[i] = a.cand[(size_t)row * n_cand + i];
  __syncthreads();
  for (int j = 0; j < a.n_top; ++j) {
    unsigned long long b = 0ull;
    for (int i = lane; i < n_cand; i += 64) b = cand[i] > b ? cand[i] : b;
    b = lp_wave_max(b);
    if (b != 0ull)      // (key64s are distinct: exactly one entry goes)
      for (int i = lane; i < n_cand; i += 64)
        if (cand[i] == b) cand[i] = 0ull;
    if (lane == 0) {
      const size_t o = (size_t)row * a.n_top + j;
      if (b == 0ull) {      // fewer than n_top columns
        a.top_token[o] = -1;
        a.top_logprob[o] = -__builtin_inff();
      } else {
        a.top_token[o] = (long long)(0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFull));
        a.top_logprob[o] = degenerate ? nan : (lp_key_value((uint32_t)(b >> 32)) - vmax) - ln_z;
      }
    }
    __syncthreads();
  }
}

}  // namespace omni

using namespace omni;

extern "C" size_t omni_logprob_workspace_bytes(int rows, int cols, int n_top) {
  if (rows <= 0 || cols < 1 || n_top < 0 || n_top > LOGPROB_MAX_TOP) return 0;
  return (size_t)rows * LOGPROB_CHUNKS * (2 * sizeof(unsigned long long) + sizeof(uint32_t) + (size_t)n_top * sizeof(unsigned long long));
}

extern "C" int omni_logprob_f16(void* lse_out_f32, void* token_logprob_out_f32, void* rank_out_i32, void* top_token_out_i64,
                                void* top_logprob_out_f32, const void* logits_f16, int64_t row_stride, int rows, int cols,
                                const void* target_i64, int n_top, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits_f16 || !workspace || rows < 0 || rows > 65535 || cols < 1 || cols > LOGPROB_MAX_COLS || row_stride < cols ||
      n_top < 0 || n_top > LOGPROB_MAX_TOP || (n_top > 0 && (!top_token_out_i64 || !top_logprob_out_f32)) ||
      ((token_logprob_out_f32 || rank_out_i32) && !target_i64))
    return OMNI_EINVAL;
  if (workspace_bytes < omni_logprob_workspace_bytes(rows, cols, n_top)) return OMNI_ENOMEM;
  if (rows == 0) return OMNI_OK;
  LogprobArgs a;
  a.x = (const half_t*)logits_f16;
  a.row_stride = row_stride;
  a.cols = cols;
  a.n_top = n_top;
  a.target = (token_logprob_out_f32 || rank_out_i32) ? (const long long*)target_i64 : nullptr;
  a.lse = (float*)lse_out_f32;
  a.token_logprob = (float*)token_logprob_out_f32;
  a.rank = (int*)rank_out_i32;
  a.top_token = (long long*)top_token_out_i64;
  a.top_logprob = (float*)top_logprob_out_f32;
  const size_t n = (size_t)rows * LOGPROB_CHUNKS;
  uint8_t* p = (uint8_t*)workspace;
  a.part_key = (unsigned long long*)p;      p += n * sizeof(unsigned long long);
  a.part_sum = (unsigned long long*)p;      p += n * sizeof(unsigned long long);
  a.cand = (unsigned long long*)p;          p += n * (size_t)n_top * sizeof(unsigned long long);
  a.part_cnt = (uint32_t*)p;
  hipLaunchKernelGGL(logprob_chunk_kernel, dim3(LOGPROB_CHUNKS, rows), dim3(LOGPROB_THREADS), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(logprob_final_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, a);
  return omni_launch_status();
}
