// Prefill attention whose keys come partly from the KV4 page cache (chunked prefill, multi-turn, prefix reuse) for MI355X
// (gfx950).  A project extension: the reference's prefill attention cannot continue from its cache either.
//
// Per sequence b and q head: the `past[b]` tokens already in the pages are the first keys / values, dequantised with the
// reference's fp16 fma(u4, scale, h(-scale*zero)) (kv4_dequant.h, the decode kernel's arithmetic); the call's own len_q tokens
// follow as the un-quantised fp16 k_new / v_new ("history from the cache, current tokens fresh", the decode kernel's rule).  The
// page slots of [past, past + len_q) -- where the writer, which runs first, has already put the chunk's quantised copy -- are
// never read.  Mask: causal, bottom-right aligned: query i sees every past key and the new keys <= i.  softmax scale 1/sqrt(128),
// GQA by head index division.
//
// Structure = attn_prefill.hip's 16-row kernel (8 waves x 16 query rows, 64-key K / V tiles double buffered in LDS, the same XOR
// swizzles, S^T = K Q^T with Q in registers, probabilities straight into the B operand of O^T = V^T P^T, exp2 online softmax,
// mask-free path for whole tiles), dense heads only.  What is new is how a tile of the PAST gets into LDS: waves 0-3 own the K
// tile, waves 4-7 the V tile; a lane fetches 16 packed bytes (32 codes = a quarter of one key row) and the row's scale / zero
// with plain vector loads BEFORE the MFMAs of the current tile, and after them dequantises in registers and writes four 16-B
// slots (ds_write_b128) to the swizzled places the LDS-DMA of a fresh tile would have filled.  The page is looked up per key
// (wave: one 16-key group, so one page for any tokens_per_block >= 16): a 64-key tile may cross pages.  Keys >= past of the last
// past tile are staged as zeros (scale and offset forced to 0: whatever their bytes decode to, NaN included, never reaches an
// accumulator) and masked like keys behind the end.  The chunk's own keys then run through the LDS-DMA staging unchanged, with
// the key index restarting at 0.
#include "attn_prefill_tile.h"
#include "kv4_dequant.h"

namespace omni {

constexpr int GPACKED_ROW = PDH / 2;   // bytes of one key row of one head in a page

struct PagedPrefillArgs {
  const half_t* q; const half_t* k; const half_t* v; half_t* out;
  int64_t q_stride, k_stride, v_stride;     // elements between consecutive tokens
  const int* cu_q;                           // [B + 1]: the call's own tokens (queries and fresh keys)
  const int* past;                           // [B]: tokens already in the pages
  const int64_t* kv_pointers;                // [B][2][max_blocks] page addresses
  int max_blocks, tpb, tpb_log2;
  int num_heads, num_kv_heads;
};

__global__ __launch_bounds__(64 * PWAVES, 2) __attribute__((amdgpu_waves_per_eu(4, 4), amdgpu_num_vgpr(128)))
void prefill_attn_paged_kv4_kernel(PagedPrefillArgs p) {
  // (four LDS objects and a loop body per buffer parity, as in attn_prefill.hip: static indices keep the staging of the next
  //  tile apart from the reads of the current one)
  __shared__ __attribute__((aligned(16))) uint8_t ktile0[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t ktile1[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t vtile0[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t vtile1[PTILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, qt = gridDim.x - 1 - blockIdx.x;   // long (late) query tiles first
  const int hk = h / (p.num_heads / p.num_kv_heads);
  const int q_begin = p.cu_q[b], len_q = p.cu_q[b + 1] - q_begin;
  const int q_first = qt * PQROWS;
  if (q_first >= len_q) return;                                 // (covers len_q = 0)
  const int past = max(p.past[b], 0);
  const int q_last = min(q_first + PQROWS, len_q) - 1;
  const int qrow = q_first + wave * 16 + l15;
  const float scale2 = 0.08838834764831845f * 1.4426950408889634f;   // log2(e)/sqrt(128): scores in the exp2 domain

  v8h qb[4];
  load_q16(p.q, p.q_stride, q_begin, qrow, len_q, h, l4, qb);
  v4f oacc[8];
  float m_run = -1e30f, l_run = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) oacc[c] = (v4f){0.f, 0.f, 0.f, 0.f};

  const int n_past = (past + PKT - 1) / PKT;          // tiles of the past (the last may be partial)
  const int f_hi = q_last + 1;                        // fresh keys this workgroup needs (causal): [0, f_hi), f_hi <= len_q
  const int n_tiles = n_past + (f_hi + PKT - 1) / PKT;

  // ---- fresh tiles: LDS-DMA, the swizzles applied on the global side (attn_prefill.hip) ----------------------------------
  const uint8_t* kbase = reinterpret_cast<const uint8_t*>(p.k + (size_t)q_begin * p.k_stride + (size_t)hk * PDH);
  const uint8_t* vbase = reinterpret_cast<const uint8_t*>(p.v + (size_t)q_begin * p.v_stride + (size_t)hk * PDH);
  const uint32_t kstride_b = (uint32_t)(p.k_stride * 2), vstride_b = (uint32_t)(p.v_stride * 2);   // host: < 2^32
#define PAGED_DMA_TILE(kb_, kt_, vt_)                                                                             \
  do {                                                                                                            \
    int ln_ = lane;                                                                                               \
    asm volatile("" : "+v"(ln_));   /* opaque per tile: the per-piece lane constants must not be hoisted */       \
    const int ss_ = ln_ & 15, lr_ = ln_ >> 4;                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < PPT; ++i_) {                                                          \
      const int row_ = 4 * PPT * wave + 4 * i_ + lr_;                                                             \
      const uint32_t kr_ = (uint32_t)((kb_) + row_ < len_q ? (kb_) + row_ : (len_q - 1));                         \
      lds_dma16(kbase + ((uint64_t)kr_ * kstride_b + (uint32_t)((ss_ ^ (row_ & 15)) << 4)),                       \
                (kt_) + (4 * PPT * wave + 4 * i_) * PROW);                                                        \
      lds_dma16(vbase + ((uint64_t)kr_ * vstride_b + (uint32_t)((ss_ ^ (2 * (row_ & 7))) << 4)),                  \
                (vt_) + (4 * PPT * wave + 4 * i_) * PROW);                                                        \
    }                                                                                                             \
  } while (0)

  // ---- past tiles: packed bytes -> registers -> dequant -> LDS ------------------------------------------------------------
  // waves 0-3: K, waves 4-7: V.  Lane t of the half: key t / 4 of the tile, codes [32 * (t % 4), + 32) of its row.
  const int is_v = wave >> 2;
  const int pkey = (tid & 255) >> 2, pquarter = tid & 3;
  const int64_t* tab = p.kv_pointers + ((size_t)b * 2 + is_v) * p.max_blocks;
  const int tail_off = p.num_kv_heads * p.tpb * GPACKED_ROW;      // scale tail of a page; the zero tail follows it
  uint4 praw = {0u, 0u, 0u, 0u};
  half_t psc = (half_t)0.0f, pze = (half_t)0.0f;
  auto past_request = [&](int kb) {
    // keys >= past of the last tile: the address of key past - 1 (a page the table is known to hold); staged as zeros below
    const int kp = min(kb + pkey, past - 1);
    const uint8_t* page = reinterpret_cast<const uint8_t*>(tab[kp >> p.tpb_log2]);
    const int row = hk * p.tpb + (kp & (p.tpb - 1));
    praw = *reinterpret_cast<const uint4*>(page + (size_t)row * GPACKED_ROW + 16 * pquarter);
    const half_t* tail = reinterpret_cast<const half_t*>(page + tail_off) + row;
    psc = tail[0];
    pze = tail[p.num_kv_heads * p.tpb];
  };
  auto past_commit = [&](int kb, uint8_t* kt, uint8_t* vt) {
    const bool live = kb + pkey < past;
    const half_t sc = live ? psc : (half_t)0.0f;
    const half_t ch = live ? (half_t)(-(float)psc * (float)pze) : (half_t)0.0f;
    v2h d[16];
    kv4_dequant16(praw, (v2h){sc, sc}, (v2h){ch, ch}, d);
    // word i of the 16 bytes = elements 8i .. 8i+7 of the quarter, delivered as the pairs (e_j, e_{j+4}): back to natural order
    uint8_t* rowp = (is_v ? vt : kt) + pkey * PROW;
    const int swz = is_v ? 2 * (pkey & 7) : (pkey & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const v8h nat = {d[4 * i][0], d[4 * i + 1][0], d[4 * i + 2][0], d[4 * i + 3][0],
                       d[4 * i][1], d[4 * i + 1][1], d[4 * i + 2][1], d[4 * i + 3][1]};
      *reinterpret_cast<v8h*>(rowp + (((4 * pquarter + i) ^ swz) << 4)) = nat;
    }
  };

  const int tr_a0 = pv16_lane_addr(l15, l4);

  if (n_past > 0) {
    past_request(0);
    past_commit(0, ktile0, vtile0);
  } else {
    PAGED_DMA_TILE(0, ktile0, vtile0);
  }
  __syncthreads();     // (carries the vmcnt(0) of the DMA pieces / the lgkmcnt(0) of the tile writes)

  int t = 0;
  auto tile_step = [&](auto parity) {
    constexpr int B = decltype(parity)::value;
    const uint8_t* kt = B ? ktile1 : ktile0;
    const uint8_t* vt = B ? vtile1 : vtile0;
    uint8_t* kt_next = B ? ktile0 : ktile1;
    uint8_t* vt_next = B ? vtile0 : vtile1;
    const bool cur_past = t < n_past;
    const int kb = PKT * (cur_past ? t : t - n_past);          // first key of the tile, counted inside its own phase
    const bool next_any = t + 1 < n_tiles, next_past = t + 1 < n_past;
    const int kb_next = PKT * (next_past ? t + 1 : t + 1 - n_past);
    // the keys of this phase end at klim; the causal diagonal only exists in the fresh phase (coff: key <= qrow + coff)
    const int klim = cur_past ? past : len_q;
    const int coff = cur_past ? (1 << 30) : 0;
    // the next past tile's packed bytes are requested before the MFMAs of this one ...
    if (next_past) past_request(kb_next);
    // ---- S^T tile: 4 blocks of 16 keys ------------------------------------------------------------------------------
    __builtin_amdgcn_s_setprio(1);
    v4f st[4];
    stage_s16(kt, qb, l15, l4, st);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    // ... and go to the other buffer (every wave left it at the previous barrier) behind them: dequant + tile writes of a
    // past tile, the LDS-DMA of a fresh one (issued only now for the reason given in attn_prefill.hip)
    if (next_past) past_commit(kb_next, kt_next, vt_next);
    else if (next_any) PAGED_DMA_TILE(kb_next, kt_next, vt_next);
    __builtin_amdgcn_sched_barrier(0);
    // does any (row, key) pair of this workgroup's tile need the mask?  (workgroup-uniform)
    const bool full = (kb + PKT <= klim) && (q_first + PQROWS <= len_q) && (kb + PKT - 1 <= q_first + coff);
    // ---- online softmax (per query row = per lane column), probabilities straight into the B operand ------------------
    v8h pb[2];
    {
      float tmax = -1e30f, m_new, alpha, psum = 0.0f;
      if (full) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) tmax = __builtin_fmaxf(tmax, st[u][r]);
        tmax = rows4_max(tmax);
        m_new = __builtin_fmaxf(m_run, tmax * scale2);
        alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(st[e >> 2][e & 3], scale2, -m_new));
          pb[e >> 3][e & 7] = (half_t)pe;
          psum += pe;
        }
      } else {
        bool okv[16];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb + 16 * u + 4 * l4 + r;
            const int ok = (int)(key < klim) & (int)(qrow < len_q) & (int)(key <= qrow + coff);
            okv[4 * u + r] = ok != 0;
            tmax = __builtin_fmaxf(tmax, ok ? st[u][r] : -1e30f);
          }
        tmax = rows4_max(tmax);
        m_new = __builtin_fmaxf(m_run, tmax * scale2);   // tmax = -1e30 (all masked) stays hugely negative
        alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = okv[e] ? __builtin_amdgcn_exp2f(__builtin_fmaf(st[e >> 2][e & 3], scale2, -m_new)) : 0.0f;
          pb[e >> 3][e & 7] = (half_t)pe;
          psum += pe;
        }
      }
      l_run = l_run * alpha + psum;
      if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {   // (wave-uniform) rescale only when a row's max moved
#pragma unroll
        for (int c = 0; c < 8; ++c) oacc[c] *= alpha;
      }
      m_run = m_new;
    }
    __builtin_amdgcn_s_setprio(1);
    stage_pv16(vt, tr_a0, pb, oacc);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();     // the next tile has landed
    ++t;
  };
  while (t < n_tiles) {
    tile_step(IntTag<0>{});
    if (t >= n_tiles) break;
    tile_step(IntTag<1>{});
  }
  store_rows16(p.out, q_begin, qrow, len_q, p.num_heads, h, l4, l_run, oacc);
}
#undef PAGED_DMA_TILE

}  // namespace omni

using namespace omni;

extern "C" int omni_prefill_attention_paged_kv4(void* out_f16, const void* q_f16, const void* k_new_f16, const void* v_new_f16,
                                                int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                                const void* cu_seqlens_q_i32, const void* past_lens_i32,
                                                const void* kv_pointers_i64, int batch, int max_blocks, int tokens_per_block,
                                                int max_seqlen_q, int num_heads, int num_kv_heads, int head_dim, void* stream) {
  if (batch < 0 || max_seqlen_q < 0) return OMNI_EINVAL;
  if (!prefill_layout_ok(head_dim, num_heads, num_kv_heads, q_stride, k_stride, v_stride) || q_stride < 0 ||
      tokens_per_block < 16 || (tokens_per_block & (tokens_per_block - 1)) != 0 || max_blocks < 0)
    return OMNI_EINVAL;
  if (batch == 0 || max_seqlen_q == 0) return OMNI_OK;        // no query token: nothing to do
  if (!out_f16 || !q_f16 || !k_new_f16 || !v_new_f16 || !cu_seqlens_q_i32 || !past_lens_i32 || !kv_pointers_i64)
    return OMNI_EINVAL;
  if (num_heads > 65535 || batch > 65535) return OMNI_EINVAL;
  PagedPrefillArgs a;
  a.q = (const half_t*)q_f16; a.k = (const half_t*)k_new_f16; a.v = (const half_t*)v_new_f16; a.out = (half_t*)out_f16;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride;
  a.cu_q = (const int*)cu_seqlens_q_i32; a.past = (const int*)past_lens_i32;
  a.kv_pointers = (const int64_t*)kv_pointers_i64;
  a.max_blocks = max_blocks; a.tpb = tokens_per_block;
  a.tpb_log2 = 0;
  while ((1 << a.tpb_log2) < tokens_per_block) ++a.tpb_log2;
  a.num_heads = num_heads; a.num_kv_heads = num_kv_heads;
  // one workgroup per (128 query rows, q head, sequence); the kernel takes blockIdx.x in reverse: long tiles first
  const dim3 grid((max_seqlen_q + PQROWS - 1) / PQROWS, num_heads, batch);
  hipLaunchKernelGGL(prefill_attn_paged_kv4_kernel, grid, dim3(64 * PWAVES), 0, (hipStream_t)stream, a);
  return omni_launch_status();
}
