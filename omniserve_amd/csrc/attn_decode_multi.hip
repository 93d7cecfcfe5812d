// Multi-token decode attention over the KV4 page cache for MI355X (gfx950): 1 - 8 new tokens per sequence (the verify step of
// speculative decoding, multi-token heads, lookahead) against a long quantised past.  A project extension with no reference
// counterpart.
//
// Semantics = attn_prefill_paged.hip's (omni_prefill_attention_paged_kv4) restricted to 0 <= len_q <= 8: keys / values
// [0, past) from the pages with the reference's fp16 fma(u4, scale, h(-scale*zero)) (kv4_dequant.h), then the call's own len_q
// tokens as un-quantised fp16 k_new / v_new; page slots at positions >= past are never read; query i sees every past key and
// the new keys <= i; scale 1/sqrt(128); probabilities rounded to fp16 before P.V, f32 accumulation.
//
// Structure.  The paged prefill kernel spends one workgroup per (128 query rows, Q HEAD, sequence): at len_q = 4 it uses 4 of
// its 128 rows, sweeps the whole past serially and dequantises every page once per q head.  Here
//   * one workgroup serves ALL G x len_q query rows of a (sequence, kv head): rows are (token, head) pairs, row r = token r / G,
//     head hk * G + r % G, packed into 16-row MFMA tiles, one tile per wave (8 waves = 128 rows; a larger group takes further
//     workgroups).  Every wave that owns rows runs its tile against the SAME dequantised 64-key K / V tile in LDS, so a page
//     is fetched and unpacked once per kv head; all 8 waves share the unpacking whether they own rows or not.
//   * the past is split over `nsplit` workgroups (the host plans the count from max_past, its bound; the lengths stay on the
//     device and every sequence deals its own 64-key tiles evenly over the splits).  A split that gets no tile -- past = 1 under
//     3 splits, past = 0 -- records (m, l) = (-1e30, 0) and the merge never looks at its accumulator.  The fresh keys belong to
//     split 0, behind its share of the past.
//   * nsplit > 1: unnormalised f32 accumulators + running max (exp2 domain) + sum go to the caller's workspace, and a second
//     launch merges them in split order (a fixed order: two runs give the same bits).  nsplit = 1 normalises and stores itself.
// The tile body (S^T = K Q^T, online softmax, O^T += V^T P^T), the tile staging of the past (packed bytes -> registers ->
// dequant -> swizzled LDS slots) and of the fresh keys (LDS-DMA) are those of attn_prefill_paged.hip.
//
// Tree form (omni_decode_attention_tree_kv4, the verify step over a token TREE: Medusa / EAGLE heads, top-k branching): the
// same kernel body with TREE = true, up to 32 new tokens per sequence.  Only the mask of the fresh tile differs: row (token i)
// sees fresh key j iff bit j of tree_mask[token i] is set and j < len_q (the word = the node's ancestors and itself), in
// place of the chain's j <= i.  The past tiles, their `full` fast path, the split and the merge are untouched.
#include "attn_prefill_tile.h"
#include "kv4_dequant.h"

namespace omni {

constexpr int DM_PACKED_ROW = PDH / 2;   // bytes of one key row of one head in a page
constexpr int DM_MAX_Q = 8;              // new tokens per sequence (chain form)
constexpr int DM_TREE_MAX_Q = 32;        // ... of the tree form: one mask word per token; the fresh tile holds 64 keys
constexpr int DM_MAX_SPLITS = 16;
// 256 CUs hold one 512-thread workgroup each (134 VGPRs): the planner aims at two rounds, which evens out ragged lengths
constexpr int DM_SLOTS = 512;

struct DecodeMultiArgs {
  const half_t* q; const half_t* k; const half_t* v; half_t* out;
  int64_t q_stride, k_stride, v_stride;     // elements between consecutive tokens
  const int* cu_q;                           // [B + 1]
  const int* past;                           // [B]
  const uint32_t* tree_mask;                 // [tokens], tree form only: bit j = the token sees fresh key j of its sequence
  const int64_t* kv_pointers;                // [B][2][max_blocks]
  int max_blocks, tpb, tpb_log2;
  int num_heads, num_kv_heads;
  int max_n;                                 // host bound of len_q (<= DM_MAX_Q, tree form DM_TREE_MAX_Q); longer sequences are cut
  int nsplit, row_groups;
  float* part_o;                             // [nsplit][B * max_n * Hq][128]
  float* part_ml;                            // [nsplit][B * max_n * Hq][2]
  int part_rows;                             // B * max_n * Hq
};

// (134 VGPRs, no scratch: three waves per SIMD, i.e. ONE 512-thread workgroup per CU.  Two would need <= 128 -- the staging
//  registers of the past tile beside the accumulators and the score tile cost the six that are over, as in the paged kernel.
//  TREE = true: 140 VGPRs, no scratch -- the mask word is one more live register, the occupancy is the same.)
template <bool TREE>
__global__ __launch_bounds__(64 * PWAVES)
void kv4_decode_multi_kernel(DecodeMultiArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t ktile0[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t ktile1[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t vtile0[PTILE];
  __shared__ __attribute__((aligned(16))) uint8_t vtile1[PTILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int b = blockIdx.z, split = blockIdx.x;
  const int hk = blockIdx.y / p.row_groups, rg = blockIdx.y - hk * p.row_groups;
  const int G = p.num_heads / p.num_kv_heads;
  const int q_begin = p.cu_q[b];
  const int len_q = min(max(p.cu_q[b + 1] - q_begin, 0), p.max_n);
  const int rows = G * len_q;
  if (rg * PQROWS >= rows) return;                              // (covers len_q = 0)
  const int past = max(p.past[b], 0);
  const float scale2 = 0.08838834764831845f * 1.4426950408889634f;   // log2(e)/sqrt(128): scores in the exp2 domain

  // ---- this wave's 16 rows: lane (l15, l4) works on row l15 of them ------------------------------------------------------
  const int row = rg * PQROWS + wave * 16 + l15;
  const bool wave_on = rg * PQROWS + wave * 16 < rows;          // (wave-uniform) a wave without rows only stages tiles
  const bool row_on = row < rows;
  const int row_c = row_on ? row : rows - 1;                    // a row behind the group reads the last one, stores nothing
  const int tok = row_c / G, head = hk * G + (row_c - tok * G);
  const size_t part_slot = ((size_t)b * p.max_n + tok) * p.num_heads + head;

  // ---- this split's share of the past: whole 64-key tiles, dealt evenly; split 0 also owns the fresh keys ----------------
  const int n_past_all = (past + PKT - 1) / PKT;
  const int per_split = (n_past_all + p.nsplit - 1) / p.nsplit;
  const int t_lo = min(split * per_split, n_past_all), t_hi = min(t_lo + per_split, n_past_all);
  const int n_past = t_hi - t_lo;
  const int n_tiles = n_past + (split == 0 ? 1 : 0);
  if (n_tiles == 0) {                                           // nothing to contribute: the merge skips l = 0
    if (wave_on && row_on && l4 == 0)
      *reinterpret_cast<v2f*>(p.part_ml + ((size_t)split * p.part_rows + part_slot) * 2) = (v2f){-1e30f, 0.0f};
    return;
  }

  v8h qb[4];
  {
    const half_t* qp = p.q + (size_t)(q_begin + tok) * p.q_stride + (size_t)head * PDH + 8 * l4;
#pragma unroll
    for (int s = 0; s < 4; ++s) qb[s] = *reinterpret_cast<const v8h*>(qp + 32 * s);
  }
  // tree form: the row's ancestor bits among the fresh keys.  Bits >= len_q are cleared here: the fresh tile's rows >= len_q
  // repeat the last key, and a set bit there would count it again.
  uint32_t mword = 0u;
  if constexpr (TREE) mword = p.tree_mask[q_begin + tok] & (len_q >= 32 ? 0xFFFFFFFFu : ((1u << len_q) - 1u));
  v4f oacc[8];
  float m_run = -1e30f, l_run = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) oacc[c] = (v4f){0.f, 0.f, 0.f, 0.f};

  // ---- the fresh tile: LDS-DMA, the swizzles applied on the global side (attn_prefill.hip); rows >= len_q repeat the last ----
  const uint8_t* kbase = reinterpret_cast<const uint8_t*>(p.k + (size_t)q_begin * p.k_stride + (size_t)hk * PDH);
  const uint8_t* vbase = reinterpret_cast<const uint8_t*>(p.v + (size_t)q_begin * p.v_stride + (size_t)hk * PDH);
  const uint32_t kstride_b = (uint32_t)(p.k_stride * 2), vstride_b = (uint32_t)(p.v_stride * 2);   // host: < 2^32
#define DM_DMA_TILE(kt_, vt_)                                                                                     \
  do {                                                                                                            \
    int ln_ = lane;                                                                                               \
    asm volatile("" : "+v"(ln_));   /* opaque per tile: the per-piece lane constants must not be hoisted */       \
    const int ss_ = ln_ & 15, lr_ = ln_ >> 4;                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < PPT; ++i_) {                                                          \
      const int row_ = 4 * PPT * wave + 4 * i_ + lr_;                                                             \
      const uint32_t kr_ = (uint32_t)(row_ < len_q ? row_ : (len_q - 1));                                         \
      lds_dma16(kbase + ((uint64_t)kr_ * kstride_b + (uint32_t)((ss_ ^ (row_ & 15)) << 4)),                       \
                (kt_) + (4 * PPT * wave + 4 * i_) * PROW);                                                        \
      lds_dma16(vbase + ((uint64_t)kr_ * vstride_b + (uint32_t)((ss_ ^ (2 * (row_ & 7))) << 4)),                  \
                (vt_) + (4 * PPT * wave + 4 * i_) * PROW);                                                        \
    }                                                                                                             \
  } while (0)

  // ---- past tiles: packed bytes -> registers -> dequant -> LDS (attn_prefill_paged.hip) -----------------------------------
  // waves 0-3: K, waves 4-7: V.  Lane t of the half: key t / 4 of the tile, codes [32 * (t % 4), + 32) of its row.
  const int is_v = wave >> 2;
  const int pkey = (tid & 255) >> 2, pquarter = tid & 3;
  const int64_t* tab = p.kv_pointers + ((size_t)b * 2 + is_v) * p.max_blocks;
  const int tail_off = p.num_kv_heads * p.tpb * DM_PACKED_ROW;      // scale tail of a page; the zero tail follows it
  uint4 praw = {0u, 0u, 0u, 0u};
  half_t psc = (half_t)0.0f, pze = (half_t)0.0f;
  auto past_request = [&](int kb) {
    // keys >= past of the last tile: the address of key past - 1 (a page the table is known to hold); staged as zeros below
    const int kp = min(kb + pkey, past - 1);
    const uint8_t* page = reinterpret_cast<const uint8_t*>(tab[kp >> p.tpb_log2]);
    const int prow = hk * p.tpb + (kp & (p.tpb - 1));
    praw = *reinterpret_cast<const uint4*>(page + (size_t)prow * DM_PACKED_ROW + 16 * pquarter);
    const half_t* tail = reinterpret_cast<const half_t*>(page + tail_off) + prow;
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
    past_request(PKT * t_lo);
    past_commit(PKT * t_lo, ktile0, vtile0);
  } else {
    DM_DMA_TILE(ktile0, vtile0);
  }
  __syncthreads();     // (carries the vmcnt(0) of the DMA pieces / the lgkmcnt(0) of the tile writes)

  int t = 0;           // tile of this split: [0, n_past) past tiles t_lo + t, then (split 0) the fresh tile
  auto tile_step = [&](auto parity) {
    constexpr int B = decltype(parity)::value;
    const uint8_t* kt = B ? ktile1 : ktile0;
    const uint8_t* vt = B ? vtile1 : vtile0;
    uint8_t* kt_next = B ? ktile0 : ktile1;
    uint8_t* vt_next = B ? vtile0 : vtile1;
    const bool cur_past = t < n_past;
    const int kb = cur_past ? PKT * (t_lo + t) : 0;            // first key of the tile, counted inside its own phase
    const bool next_any = t + 1 < n_tiles, next_past = t + 1 < n_past;
    const int kb_next = PKT * (t_lo + t + 1);
    // the keys of a past tile end at `past`; a fresh key j is seen by the tokens >= j (and tok < len_q) -- tree form: by the
    // rows whose mask word holds bit j (klim = 0 there: the fresh tile takes the bit test below)
    const int klim = cur_past ? past : (TREE ? 0 : tok + 1);
    if (next_past) past_request(kb_next);
    v4f st[4];
    if (wave_on) {
      __builtin_amdgcn_s_setprio(1);
      stage_s16(kt, qb, l15, l4, st);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(0);
    }
    // the other buffer (every wave left it at the previous barrier): dequant + tile writes of a past tile, the LDS-DMA of
    // the fresh one
    if (next_past) past_commit(kb_next, kt_next, vt_next);
    else if (next_any) DM_DMA_TILE(kt_next, vt_next);
    __builtin_amdgcn_sched_barrier(0);
    if (wave_on) {
      const bool full = cur_past && (kb + PKT <= past);          // (workgroup-uniform) no key of the tile needs the mask
      v8h pb[2];
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
            bool ok = key < klim;
            if constexpr (TREE) {                                  // (u is a constant: keys >= 32 of the fresh tile fold to false)
              if (!cur_past) ok = u < 2 && ((mword >> (16 * u + 4 * l4 + r)) & 1u) != 0u;
            }
            okv[4 * u + r] = ok;
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
      __builtin_amdgcn_s_setprio(1);
      stage_pv16(vt, tr_a0, pb, oacc);
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();     // the next tile has landed
    ++t;
  };
  while (t < n_tiles) {
    tile_step(IntTag<0>{});
    if (t >= n_tiles) break;
    tile_step(IntTag<1>{});
  }

  if (!wave_on) return;
  const float l = rows4_sum(l_run);
  if (!row_on) return;
  if (p.nsplit == 1) {                                            // no merge: normalise and store
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    half_t* op = p.out + ((size_t)(q_begin + tok) * p.num_heads + head) * PDH + 4 * l4;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      typedef _Float16 v4h_t __attribute__((ext_vector_type(4)));
      const v4h_t o = {(half_t)(oacc[c][0] * inv), (half_t)(oacc[c][1] * inv), (half_t)(oacc[c][2] * inv),
                       (half_t)(oacc[c][3] * inv)};
      *reinterpret_cast<v4h_t*>(op + c * 16) = o;
    }
    return;
  }
  const size_t prow = (size_t)split * p.part_rows + part_slot;
  float* po = p.part_o + prow * PDH + 4 * l4;
#pragma unroll
  for (int c = 0; c < 8; ++c) *reinterpret_cast<v4f*>(po + c * 16) = oacc[c];
  if (l4 == 0) *reinterpret_cast<v2f*>(p.part_ml + prow * 2) = (v2f){m_run, l};
}
#undef DM_DMA_TILE

// Merge of the split partials, in split order: 32 threads per (sequence, token, head) row, four elements each.
__global__ __launch_bounds__(256) void kv4_decode_multi_merge_kernel(DecodeMultiArgs p) {
  const int slot = blockIdx.x * 8 + (threadIdx.x >> 5), e4 = (threadIdx.x & 31) * 4;
  if (slot >= p.part_rows) return;
  const int head = slot % p.num_heads, bt = slot / p.num_heads;
  const int tok = bt % p.max_n, b = bt / p.max_n;
  const int q_begin = p.cu_q[b];
  const int len_q = min(max(p.cu_q[b + 1] - q_begin, 0), p.max_n);
  if (tok >= len_q) return;
  float m = -1e30f;
  for (int s = 0; s < p.nsplit; ++s) {
    const v2f ml = *reinterpret_cast<const v2f*>(p.part_ml + ((size_t)s * p.part_rows + slot) * 2);
    if (ml[1] > 0.0f) m = __builtin_fmaxf(m, ml[0]);
  }
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.0f;
  for (int s = 0; s < p.nsplit; ++s) {
    const size_t prow = (size_t)s * p.part_rows + slot;
    const v2f ml = *reinterpret_cast<const v2f*>(p.part_ml + prow * 2);
    if (!(ml[1] > 0.0f)) continue;                                // an empty split: its accumulator was never written
    const float w = __builtin_amdgcn_exp2f(ml[0] - m);
    const v4f o = *reinterpret_cast<const v4f*>(p.part_o + prow * PDH + e4);
    acc = acc + o * w;
    l = l + ml[1] * w;
  }
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  typedef _Float16 v4h_t __attribute__((ext_vector_type(4)));
  const v4h_t o = {(half_t)(acc[0] * inv), (half_t)(acc[1] * inv), (half_t)(acc[2] * inv), (half_t)(acc[3] * inv)};
  *reinterpret_cast<v4h_t*>(p.out + ((size_t)(q_begin + tok) * p.num_heads + head) * PDH + e4) = o;
}

static thread_local int g_dm_override_nsplit = 0;   // tuning / test hook, see omni_decode_attention_multi_kv4_set_split_override

// Split count: DM_SLOTS workgroups where the past allows it, at least two 64-key tiles per split.
static int plan_decode_multi(int batch, int num_kv_heads, int row_groups, int max_past) {
  if (g_dm_override_nsplit > 0) return g_dm_override_nsplit < DM_MAX_SPLITS ? g_dm_override_nsplit : DM_MAX_SPLITS;
  const long long wgs = (long long)batch * num_kv_heads * row_groups;
  const long long tiles = ((long long)max_past + PKT - 1) / PKT;
  long long s = (DM_SLOTS + wgs - 1) / wgs;
  if (s > tiles / 2) s = tiles / 2;
  if (s > DM_MAX_SPLITS) s = DM_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static size_t decode_multi_bytes(int batch, int num_heads, int max_n, int nsplit) {
  return (size_t)nsplit * (size_t)batch * max_n * num_heads * (PDH + 2) * sizeof(float);
}

}  // namespace omni

using namespace omni;

extern "C" void omni_decode_attention_multi_kv4_set_split_override(int nsplit) {
  // nsplit > 0: force the KV split count of both forms (tests, tuning sweeps; at most 16); 0: the planner decides
  omni::g_dm_override_nsplit = nsplit > 0 ? nsplit : 0;
}

extern "C" size_t omni_decode_attention_multi_kv4_workspace_bytes(int batch, int num_heads, int max_seqlen_q, int max_past) {
  (void)max_past;     // the bound holds for every forced split count, which no past length limits
  if (batch < 1 || num_heads < 1 || max_seqlen_q < 1) return 0;
  const int n = max_seqlen_q < DM_MAX_Q ? max_seqlen_q : DM_MAX_Q;
  return decode_multi_bytes(batch, num_heads, n, DM_MAX_SPLITS);
}

// The two entries' argument checks, plan and launches: `max_q` = the form's bound on max_seqlen_q, `tree_mask` = the tree form's
// mask words (nullptr: the chain form).
static int decode_multi_launch(void* out_f16, const void* q_f16, const void* k_new_f16, const void* v_new_f16,
                               int64_t q_stride, int64_t k_stride, int64_t v_stride,
                               const void* cu_seqlens_q_i32, const void* past_lens_i32, const void* tree_mask_u32, bool tree,
                               const void* kv_pointers_i64, int batch, int max_blocks, int tokens_per_block,
                               int max_seqlen_q, int max_q, int num_heads, int num_kv_heads, int head_dim, int max_past,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (batch < 0 || max_seqlen_q < 0 || max_seqlen_q > max_q || max_past < 0) return OMNI_EINVAL;
  if (!prefill_layout_ok(head_dim, num_heads, num_kv_heads, q_stride, k_stride, v_stride) || q_stride < 0 ||
      tokens_per_block < 16 || (tokens_per_block & (tokens_per_block - 1)) != 0 || max_blocks < 0)
    return OMNI_EINVAL;
  if (tree && !tree_mask_u32) return OMNI_EINVAL;
  if (batch == 0 || max_seqlen_q == 0) return OMNI_OK;        // no query token: nothing to do
  if (!out_f16 || !q_f16 || !k_new_f16 || !v_new_f16 || !cu_seqlens_q_i32 || !past_lens_i32 || !kv_pointers_i64)
    return OMNI_EINVAL;
  if (batch > 65535 || (long long)batch * max_seqlen_q * num_heads > (1LL << 27)) return OMNI_EINVAL;   // (row index: int32)
  DecodeMultiArgs a;
  a.q = (const half_t*)q_f16; a.k = (const half_t*)k_new_f16; a.v = (const half_t*)v_new_f16; a.out = (half_t*)out_f16;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride;
  a.cu_q = (const int*)cu_seqlens_q_i32; a.past = (const int*)past_lens_i32;
  a.tree_mask = (const uint32_t*)tree_mask_u32;
  a.kv_pointers = (const int64_t*)kv_pointers_i64;
  a.max_blocks = max_blocks; a.tpb = tokens_per_block;
  a.tpb_log2 = 0;
  while ((1 << a.tpb_log2) < tokens_per_block) ++a.tpb_log2;
  a.num_heads = num_heads; a.num_kv_heads = num_kv_heads;
  a.max_n = max_seqlen_q;
  const int group_rows = (num_heads / num_kv_heads) * max_seqlen_q;
  a.row_groups = (group_rows + PQROWS - 1) / PQROWS;
  if ((long long)num_kv_heads * a.row_groups > 65535) return OMNI_EINVAL;
  a.nsplit = plan_decode_multi(batch, num_kv_heads, a.row_groups, max_past);
  const size_t need = decode_multi_bytes(batch, num_heads, max_seqlen_q, a.nsplit);
  if (!workspace || workspace_bytes < need) return OMNI_ENOMEM;
  if (((uintptr_t)workspace & 15) != 0) return OMNI_EINVAL;
  a.part_rows = batch * max_seqlen_q * num_heads;
  a.part_o = (float*)workspace;
  a.part_ml = a.part_o + (size_t)a.nsplit * a.part_rows * PDH;
  const dim3 grid(a.nsplit, num_kv_heads * a.row_groups, batch);
  if (tree)
    hipLaunchKernelGGL(kv4_decode_multi_kernel<true>, grid, dim3(64 * PWAVES), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(kv4_decode_multi_kernel<false>, grid, dim3(64 * PWAVES), 0, (hipStream_t)stream, a);
  if (a.nsplit > 1)
    hipLaunchKernelGGL(kv4_decode_multi_merge_kernel, dim3((a.part_rows + 7) / 8), dim3(256), 0, (hipStream_t)stream, a);
  return omni_launch_status();
}

extern "C" int omni_decode_attention_multi_kv4(void* out_f16, const void* q_f16, const void* k_new_f16, const void* v_new_f16,
                                               int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                               const void* cu_seqlens_q_i32, const void* past_lens_i32,
                                               const void* kv_pointers_i64, int batch, int max_blocks, int tokens_per_block,
                                               int max_seqlen_q, int num_heads, int num_kv_heads, int head_dim, int max_past,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  return decode_multi_launch(out_f16, q_f16, k_new_f16, v_new_f16, q_stride, k_stride, v_stride, cu_seqlens_q_i32, past_lens_i32,
                             nullptr, false, kv_pointers_i64, batch, max_blocks, tokens_per_block, max_seqlen_q, DM_MAX_Q,
                             num_heads, num_kv_heads, head_dim, max_past, workspace, workspace_bytes, stream);
}

extern "C" size_t omni_decode_attention_tree_kv4_workspace_bytes(int batch, int num_heads, int max_seqlen_q, int max_past) {
  (void)max_past;     // as omni_decode_attention_multi_kv4_workspace_bytes: every forced split count
  if (batch < 1 || num_heads < 1 || max_seqlen_q < 1) return 0;
  const int n = max_seqlen_q < DM_TREE_MAX_Q ? max_seqlen_q : DM_TREE_MAX_Q;
  return decode_multi_bytes(batch, num_heads, n, DM_MAX_SPLITS);
}

extern "C" int omni_decode_attention_tree_kv4(void* out_f16, const void* q_f16, const void* k_new_f16, const void* v_new_f16,
                                              int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                              const void* cu_seqlens_q_i32, const void* past_lens_i32,
                                              const void* tree_mask_u32, const void* kv_pointers_i64, int batch, int max_blocks,
                                              int tokens_per_block, int max_seqlen_q, int num_heads, int num_kv_heads,
                                              int head_dim, int max_past, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  return decode_multi_launch(out_f16, q_f16, k_new_f16, v_new_f16, q_stride, k_stride, v_stride, cu_seqlens_q_i32, past_lens_i32,
                             tree_mask_u32, true, kv_pointers_i64, batch, max_blocks, tokens_per_block, max_seqlen_q,
                             DM_TREE_MAX_Q, num_heads, num_kv_heads, head_dim, max_past, workspace, workspace_bytes, stream);
}
