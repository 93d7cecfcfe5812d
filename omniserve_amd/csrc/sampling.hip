// Sampled decoding for MI355X (gfx950): temperature, top-p and top-k filters and the draw, one token per logits row.
//
// Replaces the torch code of the reference's sampler (omniserve/modeling/layers/sampler.py:29-50, 96-102: temperature
// warper, top-p warper, top-k warper, softmax, torch.multinomial) -- the full-vocabulary sort included.  The contract is
// DESIGN.md section 4.6; tests/sampling_cases.py holds its f64 oracle.
//
// fp16 logits have at most 65 536 distinct values, and the 16-bit orderable key of the arg-max kernel (argmax_key in
// elementwise.hip) orders them.  Every token with the same key has the same weight, so both filter thresholds and the draw
// are found by radix selection over COUNT histograms of the key, without sorting anything:
//   pass A  per high byte of the key: token count and mass (the sum of the weights as 2^40 fixed point),
//   pass B  per low byte, inside the one high-byte bin that holds the threshold max(t_p, t_k): token count,
//   pass C  per low byte, inside the high-byte bin in which u * Z crosses: token count, also kept per chunk,
//   pass D  the chosen token is the r-th occurrence of key K in index order: the one workgroup whose chunk holds it counts.
// Each pass is a (chunks, rows) grid.  A pass begins by locating its bin from the previous pass's table with a 256-wide
// scan that every workgroup of the row repeats (same integers in, same integers out); workgroup 0 of the row records what
// it found for the passes behind it.  All sums are integers (counts; weights as w * 2^40, at most 2^40 each, so 2^22
// columns cannot overflow 64 bits) and reach the tables through integer atomics: the result does not depend on arrival order
// or on the grid.  The only floating-point steps are per KEY: its weight, p * Z and u * Z.
// Greedy rows (and every row's maximum) come from omni_argmax_f16 itself, so they are its answer bit for bit.
#include "common.h"
#include "omniserve_hip.h"

namespace omni {

constexpr int SAMPLE_CHUNKS = 32;
constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_MAX_COLS = 1 << 22;
constexpr uint32_t KEY_POS_INF = 0xFC00u;      // keys >= this: +inf and the NaNs that arg-max treats as the maximum
constexpr uint32_t KEY_NEG_INF = 0x03FFu;      // keys <= this: -inf (and negative NaNs below it): weight 0

struct SampleRowState {      // one per row; written by workgroup 0 of the row, read by the passes behind
  uint32_t greedy, maxkey;   // pass A
  float scale;               //   log2(e) / temperature
  uint32_t s_t;              // pass B: slot (255 - high byte) of the bin that holds the threshold key
  unsigned long long m_above, p_ceil;   //   mass above that bin; ceil(top_p * Z) if top-p cuts inside it, else 0
  uint32_t c_above, k_eff;   //   tokens above that bin; top_k if top-k cuts inside it, else 0
  unsigned long long target, mu_above;  // pass C: floor(u * Z'), the (exclusion-adjusted) mass above the draw's bin
  uint32_t thr_key, s_u, empty, pad[15];
};
static_assert(sizeof(SampleRowState) == 128, "row state is one 128-byte line");

// the value part of argmax_key (elementwise.hip): -0 == +0, positive NaN above +inf, negative NaN below -inf
__device__ __forceinline__ uint32_t sample_key(uint32_t h16) {
  uint32_t h = h16 & 0xFFFFu;
  if (h == 0x8000u) h = 0;
  return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
}
__device__ __forceinline__ uint32_t half_bits(half_t v) { return __builtin_bit_cast(uint16_t, v); }
__device__ __forceinline__ float key_value(uint32_t key) {
  const uint16_t h = (uint16_t)((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
  return (float)__builtin_bit_cast(half_t, h);
}
// ONE definition of a key's weight, exp((x - max) / T) * 2^40 truncated: pass A (per token) and the scans (per key) agree.
// A finite logit weighs at least one unit (2^-40 of the maximum's weight): when `exclude` takes the token that held all the
// resolvable mass, what is left of the kept set still has a mass to draw from.
__device__ __forceinline__ unsigned long long key_weight(uint32_t key, float vmax, float scale) {
  if (key <= KEY_NEG_INF) return 0ull;
  const float w = __builtin_amdgcn_exp2f((key_value(key) - vmax) * scale);
  const unsigned long long fx = (unsigned long long)(w * 1099511627776.0f);
  return fx ? fx : 1ull;
}

template <class T>
__device__ __forceinline__ T block_scan_incl(T v, T* wave_tot) {      // 256 threads, wave_tot: LDS [4]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wv] = v;
  __syncthreads();
  T add = 0;
  for (int w = 0; w < wv; ++w) add += wave_tot[w];
  return v + add;
}

// f(fp16 bits, column) for every column of [c0, c1); 16-byte loads where the row layout allows (as the arg-max kernel)
template <class F>
__device__ __forceinline__ void chunk_for_each(const half_t* xr, int c0, int c1, bool vec, F&& f) {
  if (vec) {
    for (int c = c0 + 8 * (int)threadIdx.x; c < c1; c += 8 * SAMPLE_THREADS) {
      if (c + 8 <= c1) {
        const uint4 v = *reinterpret_cast<const uint4*>(xr + c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f(w[j] & 0xFFFFu, c + 2 * j);
          f(w[j] >> 16, c + 2 * j + 1);
        }
      } else {
        for (int e = c; e < c1; ++e) f(half_bits(xr[e]), e);
      }
    }
  } else {
    for (int e = c0 + (int)threadIdx.x; e < c1; e += SAMPLE_THREADS) f(half_bits(xr[e]), e);
  }
}

struct SampleArgs {
  const half_t* x;
  int64_t row_stride;
  int cols;
  const float* temperature;
  const int* top_k;
  const float* top_p;
  const float* u;
  const long long* probe;
  const long long* exclude;
  long long* token;
  float* probe_prob;
  SampleRowState* state;
  uint32_t* hi_cnt;                 // [rows][256]
  unsigned long long* hi_mass;      // [rows][256]
  uint32_t* lo_b;                   // [rows][256]
  uint32_t* lo_c;                   // [rows][256]
  uint32_t* part_c;                 // [rows][SAMPLE_CHUNKS][256]
};

struct RowView {
  const half_t* xr;
  int c0, c1, per;
  bool vec;
};
__device__ __forceinline__ RowView row_view(const SampleArgs& a) {
  RowView v;
  v.per = ((a.cols + SAMPLE_CHUNKS - 1) / SAMPLE_CHUNKS + 7) & ~7;
  v.c0 = (int)blockIdx.x * v.per;
  v.c1 = min(a.cols, v.c0 + v.per);
  v.xr = a.x + (size_t)blockIdx.y * a.row_stride;
  v.vec = (a.row_stride % 8) == 0 && (reinterpret_cast<uintptr_t>(a.x) % 16) == 0;
  return v;
}

// the excluded token of a row, if it has one inside the row: its key and weight (the caller decides whether it is kept)
struct Excluded { long long idx; uint32_t key; unsigned long long w; };
__device__ __forceinline__ Excluded excluded_of(const SampleArgs& a, const RowView& v, int row, float vmax, float scale) {
  Excluded e{-1, 0u, 0ull};
  if (a.exclude) {
    const long long i = a.exclude[row];
    if (i >= 0 && i < a.cols) {
      e.idx = i;
      e.key = sample_key(half_bits(v.xr[i]));
      e.w = key_weight(e.key, vmax, scale);
    }
  }
  return e;
}

// tokens of [c0, c1) whose key has high byte `hi`, counted per low byte into lds[256]; added to tab[256], copied to part
__device__ __forceinline__ void hist_low_byte(const RowView& v, uint32_t hi, uint32_t* lds, uint32_t* tab, uint32_t* part) {
  lds[threadIdx.x] = 0u;
  __syncthreads();
  chunk_for_each(v.xr, v.c0, v.c1, v.vec, [&](uint32_t h, int) {
    const uint32_t key = sample_key(h);
    if ((key >> 8) == hi) atomicAdd(&lds[key & 255u], 1u);
  });
  __syncthreads();
  const uint32_t n = lds[threadIdx.x];
  if (n) atomicAdd(&tab[threadIdx.x], n);
  if (part) part[threadIdx.x] = n;
}

// the row's tables start from zero (a kernel, not a memset node: one kind of node in a captured step)
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_zero_kernel(uint4* __restrict__ tables, size_t n16) {
  const size_t i = (size_t)blockIdx.x * SAMPLE_THREADS + threadIdx.x;
  if (i < n16) tables[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- pass A: greedy test, then count and mass per high byte ------------------------------------------------
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_pass_a_kernel(SampleArgs a) {
  __shared__ uint32_t cnt[256];
  __shared__ unsigned long long mass[256];
  const int row = blockIdx.y, t = threadIdx.x;
  const RowView v = row_view(a);
  const long long tok = a.token[row];                      // omni_argmax_f16's answer: the first maximum
  const uint32_t maxkey = sample_key(half_bits(v.xr[tok]));
  const float temp = a.temperature[row], p = a.top_p[row];
  const bool greedy = !(temp >= 1e-5f) || !(p >= 1e-8f) || a.top_k[row] == 1 || maxkey >= KEY_POS_INF || maxkey <= KEY_NEG_INF;
  const float scale = 1.4426950408889634f / temp;
  if (blockIdx.x == 0 && t == 0) {
    SampleRowState* st = a.state + row;
    st->greedy = greedy ? 1u : 0u;
    st->maxkey = maxkey;
    st->scale = scale;
    if (a.probe_prob) a.probe_prob[row] = (greedy && a.probe[row] == tok) ? 1.0f : 0.0f;
  }
  if (greedy) return;
  cnt[t] = 0u;
  mass[t] = 0ull;
  __syncthreads();
  const float vmax = key_value(maxkey);
  chunk_for_each(v.xr, v.c0, v.c1, v.vec, [&](uint32_t h, int) {
    const uint32_t key = sample_key(h);
    const unsigned long long w = key_weight(key, vmax, scale);
    atomicAdd(&cnt[key >> 8], 1u);
    if (w) atomicAdd(&mass[key >> 8], w);
  });
  __syncthreads();
  if (cnt[t]) atomicAdd(&a.hi_cnt[(size_t)row * 256 + t], cnt[t]);
  if (mass[t]) atomicAdd(&a.hi_mass[(size_t)row * 256 + t], mass[t]);
}

// ---- pass B: the high-byte bin of the threshold max(t_p, t_k); count per low byte inside it -------------------
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_pass_b_kernel(SampleArgs a) {
  __shared__ uint32_t lds[256];
  __shared__ unsigned long long tot64[4];
  __shared__ uint32_t tot32[4];
  __shared__ unsigned long long sh_z, sh_mabove;
  __shared__ uint32_t sh_cabove;
  const int row = blockIdx.y, t = threadIdx.x;
  const SampleRowState* st = a.state + row;
  if (st->greedy) return;
  const RowView v = row_view(a);
  // slot t = high byte 255 - t: descending key order
  const uint32_t c = a.hi_cnt[(size_t)row * 256 + 255 - t];
  const unsigned long long m = a.hi_mass[(size_t)row * 256 + 255 - t];
  const uint32_t C = block_scan_incl(c, tot32);
  const unsigned long long M = block_scan_incl(m, tot64);
  if (t == 255) sh_z = M;
  __syncthreads();
  const float p = a.top_p[row];
  const int k = a.top_k[row];
  const bool p_on = p < 1.0f, k_on = k > 0 && k <= a.cols;
  // a key is kept by top-p iff the mass strictly above it is < p * Z: the threshold is the first slot whose inclusive
  // mass reaches ceil(p * Z); by top-k iff fewer than k tokens lie strictly above it
  const unsigned long long p_ceil = p_on ? (unsigned long long)__builtin_ceil((double)p * (double)sh_z) : 0ull;
  const int np = __syncthreads_count(p_on && M < p_ceil);
  const int nk = __syncthreads_count(k_on && C < (uint32_t)k);
  const int sp = p_on ? min(np, 255) : 255, sk = k_on ? min(nk, 255) : 255;
  const int s_t = min(sp, sk);
  if (t == s_t) {
    sh_mabove = M - m;
    sh_cabove = C - c;
  }
  __syncthreads();
  if (blockIdx.x == 0 && t == 0) {
    SampleRowState* w = a.state + row;
    w->s_t = (uint32_t)s_t;
    w->m_above = sh_mabove;
    w->c_above = sh_cabove;
    w->p_ceil = (p_on && sp == s_t) ? p_ceil : 0ull;
    w->k_eff = (k_on && sk == s_t) ? (uint32_t)k : 0u;
  }
  hist_low_byte(v, 255u - (uint32_t)s_t, lds, a.lo_b + (size_t)row * 256, nullptr);
}

// ---- pass C: the threshold key, Z, probe_prob, u * Z' and its high-byte bin; count per low byte inside it -----
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_pass_c_kernel(SampleArgs a) {
  __shared__ uint32_t lds[256];
  __shared__ unsigned long long tot64[4];
  __shared__ uint32_t tot32[4];
  __shared__ unsigned long long sh_zkept, sh_muabove;
  const int row = blockIdx.y, t = threadIdx.x;
  const SampleRowState* st = a.state + row;
  if (st->greedy) return;
  const RowView v = row_view(a);
  const float vmax = key_value(st->maxkey), scale = st->scale;
  const int s_t = (int)st->s_t;
  const uint32_t hi_t = 255u - (uint32_t)s_t;
  const unsigned long long m_above = st->m_above, p_ceil = st->p_ceil;
  const uint32_t c_above = st->c_above, k_eff = st->k_eff;
  // slot t = low byte 255 - t inside the threshold's bin
  const uint32_t key = (hi_t << 8) | (255u - (uint32_t)t);
  const uint32_t c = a.lo_b[(size_t)row * 256 + 255 - t];
  const unsigned long long m = (unsigned long long)c * key_weight(key, vmax, scale);
  const uint32_t C = block_scan_incl(c, tot32);
  const unsigned long long M = block_scan_incl(m, tot64);
  const int np = __syncthreads_count(p_ceil != 0ull && m_above + M < p_ceil);
  const int nk = __syncthreads_count(k_eff != 0u && c_above + C < k_eff);
  const int l_t = min(p_ceil ? min(np, 255) : 255, k_eff ? min(nk, 255) : 255);
  const uint32_t thr_key = (hi_t << 8) | (255u - (uint32_t)l_t);
  if (t == l_t) sh_zkept = m_above + M;
  __syncthreads();
  const unsigned long long z_kept = sh_zkept;
  Excluded e = excluded_of(a, v, row, vmax, scale);
  const bool excl = e.idx >= 0 && e.key >= thr_key;
  const unsigned long long z_draw = z_kept - (excl ? e.w : 0ull);
  const bool empty = z_draw == 0ull;
  const float u = __builtin_fminf(__builtin_fmaxf(a.u[row], 0.0f), 1.0f);
  unsigned long long target = 0ull;
  if (!empty) {
    target = (unsigned long long)((double)u * (double)z_draw);
    if (target > z_draw - 1ull) target = z_draw - 1ull;
  }
  // the draw's bin: the first slot whose inclusive mass (less the excluded token's weight at and below its bin) exceeds
  // the target; never below the threshold's bin
  const int s_e = excl ? 255 - (int)(e.key >> 8) : 256;
  const unsigned long long m2 = a.hi_mass[(size_t)row * 256 + 255 - t];
  const unsigned long long M2 = block_scan_incl(m2, tot64);
  const unsigned long long M2x = M2 - (t >= s_e ? e.w : 0ull);
  const int nu = __syncthreads_count(M2x <= target);
  const int s_u = min(nu, s_t);
  if (t == s_u) sh_muabove = (M2 - m2) - ((t - 1 >= s_e) ? e.w : 0ull);
  __syncthreads();
  if (blockIdx.x == 0 && t == 0) {
    SampleRowState* w = a.state + row;
    w->thr_key = thr_key;
    w->target = target;
    w->s_u = (uint32_t)s_u;
    w->mu_above = sh_muabove;
    w->empty = empty ? 1u : 0u;
    if (a.probe_prob) {
      const long long pr = a.probe[row];
      float prob = 0.0f;
      if (pr >= 0 && pr < a.cols) {
        const uint32_t kp = sample_key(half_bits(v.xr[pr]));
        if (kp >= thr_key) prob = (float)((double)key_weight(kp, vmax, scale) / (double)z_kept);
      }
      a.probe_prob[row] = prob;
    }
  }
  if (empty) return;
  hist_low_byte(v, 255u - (uint32_t)s_u, lds, a.lo_c + (size_t)row * 256,
                a.part_c + ((size_t)row * SAMPLE_CHUNKS + blockIdx.x) * 256);
}

// ---- pass D: the key K in which the target falls and r; the r-th occurrence of K in index order ------------------
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_pass_d_kernel(SampleArgs a) {
  __shared__ unsigned long long tot64[4];
  __shared__ uint32_t tot32[4];
  __shared__ uint32_t sh_key;
  __shared__ unsigned long long sh_r;
  const int row = blockIdx.y, t = threadIdx.x;
  const SampleRowState* st = a.state + row;
  if (st->greedy) return;
  const RowView v = row_view(a);
  const float vmax = key_value(st->maxkey), scale = st->scale;
  Excluded e = excluded_of(a, v, row, vmax, scale);
  if (st->empty) {      // the excluded token was the whole kept set: hand it back (its probe_prob is 1)
    if (blockIdx.x == 0 && t == 0) a.token[row] = e.idx;
    return;
  }
  const bool excl = e.idx >= 0 && e.key >= st->thr_key;
  const uint32_t hi_u = 255u - st->s_u;
  const unsigned long long target = st->target, mu_above = st->mu_above;
  const uint32_t key = (hi_u << 8) | (255u - (uint32_t)t);
  uint32_t c = a.lo_c[(size_t)row * 256 + 255 - t];
  if (excl && e.key == key && c > 0u) c -= 1u;
  const unsigned long long w = key_weight(key, vmax, scale);
  const unsigned long long m = (unsigned long long)c * w;
  const unsigned long long M = block_scan_incl(m, tot64);
  const int nu = __syncthreads_count(mu_above + M <= target);
  const int l_u = min(nu, 255);
  if (t == l_u) {
    unsigned long long r = w ? (target - (mu_above + M - m)) / w : 0ull;
    if (c > 0u && r > (unsigned long long)(c - 1u)) r = c - 1u;
    sh_key = key;
    sh_r = r;
  }
  __syncthreads();
  const uint32_t key_u = sh_key;
  const unsigned long long r = sh_r;
  const long long skip = (excl && e.key == key_u) ? e.idx : -1;
  // occurrences of the key in the chunks in front of this one (pass C's per-chunk counts, less the excluded token)
  unsigned long long before = 0ull, mine = 0ull;
  for (int ch = 0; ch <= (int)blockIdx.x; ++ch) {
    unsigned long long n = a.part_c[((size_t)row * SAMPLE_CHUNKS + ch) * 256 + (key_u & 255u)];
    if (skip >= (long long)ch * v.per && skip < (long long)(ch + 1) * v.per && n > 0ull) n -= 1ull;
    if (ch < (int)blockIdx.x) before += n; else mine = n;
  }
  if (r < before || r >= before + mine) return;
  // thread t owns a contiguous span of the chunk, so thread order is index order
  const int sub = (v.per + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
  const int b0 = min(v.c1, v.c0 + t * sub), b1 = min(v.c1, b0 + sub);
  uint32_t n = 0u;
  for (int i = b0; i < b1; ++i) n += (sample_key(half_bits(v.xr[i])) == key_u && i != skip) ? 1u : 0u;
  const uint32_t N = block_scan_incl(n, tot32);
  const unsigned long long want = r - before;
  if (want >= (unsigned long long)(N - n) && want < (unsigned long long)N) {
    uint32_t left = (uint32_t)(want - (N - n));
    for (int i = b0; i < b1; ++i) {
      if (sample_key(half_bits(v.xr[i])) == key_u && i != skip) {
        if (left == 0u) {
          a.token[row] = i;
          break;
        }
        left -= 1u;
      }
    }
  }
}

constexpr size_t SAMPLE_TABLE_BYTES = 256 * (sizeof(uint32_t) * 3 + sizeof(unsigned long long));      // per row, zeroed per call

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace omni

using namespace omni;

extern "C" size_t omni_sample_workspace_bytes(int rows, int cols) {
  if (rows <= 0 || cols < 1) return 0;
  return align256(omni_argmax_workspace_bytes(rows)) + (size_t)rows * (sizeof(SampleRowState) + SAMPLE_TABLE_BYTES +
                                                                         (size_t)SAMPLE_CHUNKS * 256 * sizeof(uint32_t));
}

extern "C" int omni_sample_f16(void* token_out_i64, void* probe_prob_out_f32, const void* logits_f16, int64_t row_stride,
                               int rows, int cols, const void* temperature_f32, const void* top_k_i32, const void* top_p_f32,
                               const void* u_f32, const void* probe_i64, const void* exclude_i64, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!token_out_i64 || !logits_f16 || !temperature_f32 || !top_k_i32 || !top_p_f32 || !u_f32 || !workspace || rows < 0 ||
      rows > 65535 || cols < 1 || cols > SAMPLE_MAX_COLS || row_stride < cols || (probe_prob_out_f32 && !probe_i64))
    return OMNI_EINVAL;
  if (workspace_bytes < omni_sample_workspace_bytes(rows, cols)) return OMNI_ENOMEM;
  if (rows == 0) return OMNI_OK;
  uint8_t* ws = (uint8_t*)workspace;
  const size_t argmax_bytes = align256(omni_argmax_workspace_bytes(rows));
  SampleArgs a;
  a.x = (const half_t*)logits_f16;
  a.row_stride = row_stride;
  a.cols = cols;
  a.temperature = (const float*)temperature_f32;
  a.top_k = (const int*)top_k_i32;
  a.top_p = (const float*)top_p_f32;
  a.u = (const float*)u_f32;
  a.probe = probe_prob_out_f32 ? (const long long*)probe_i64 : nullptr;
  a.exclude = (const long long*)exclude_i64;
  a.token = (long long*)token_out_i64;
  a.probe_prob = (float*)probe_prob_out_f32;
  uint8_t* p = ws + argmax_bytes;
  a.state = (SampleRowState*)p;             p += (size_t)rows * sizeof(SampleRowState);
  uint8_t* tables = p;
  a.hi_mass = (unsigned long long*)p;       p += (size_t)rows * 256 * sizeof(unsigned long long);
  a.hi_cnt = (uint32_t*)p;                  p += (size_t)rows * 256 * sizeof(uint32_t);
  a.lo_b = (uint32_t*)p;                    p += (size_t)rows * 256 * sizeof(uint32_t);
  a.lo_c = (uint32_t*)p;                    p += (size_t)rows * 256 * sizeof(uint32_t);
  a.part_c = (uint32_t*)p;
  const size_t n16 = (size_t)rows * SAMPLE_TABLE_BYTES / 16;
  hipLaunchKernelGGL(sample_zero_kernel, dim3((unsigned)((n16 + SAMPLE_THREADS - 1) / SAMPLE_THREADS)), dim3(SAMPLE_THREADS), 0,
                     (hipStream_t)stream, (uint4*)tables, n16);
  const int rc = omni_argmax_f16(token_out_i64, logits_f16, row_stride, rows, cols, ws, argmax_bytes, stream);
  if (rc != OMNI_OK) return rc;
  const dim3 grid(SAMPLE_CHUNKS, rows), block(SAMPLE_THREADS);
  hipLaunchKernelGGL(sample_pass_a_kernel, grid, block, 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sample_pass_b_kernel, grid, block, 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sample_pass_c_kernel, grid, block, 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sample_pass_d_kernel, grid, block, 0, (hipStream_t)stream, a);
  return omni_launch_status();
}
