// What the prefill attention translation units share (attn_prefill.hip: the 16-row, ping-pong and 32-row forms;
// attn_prefill_paged.hip: the form that continues from the KV4 pages): the tile geometry, the varlen argument block with its
// window arithmetic and XCD-aware workgroup order, the layout check of the host entry points, and four stages of the 16-row
// tile body (Q load, S^T = K Q^T, O^T += V^T P^T, normalise and store) that the lock-step, the ping-pong and the paged kernel call.
#pragma once
#include "common.h"

namespace omni {

constexpr int PDH = 128;              // head dim
constexpr int PKT = 64;               // keys per tile
constexpr int PROW = 256;             // bytes per key row of a K or V tile (swizzled 16-B slots)
constexpr int PTILE = PKT * PROW;     // bytes of a tile
constexpr int PWAVES = 8;             // 16-row forms: 8 waves x 16 rows: ~120 VGPRs per wave, 4 waves per SIMD hide the softmax VALU work
constexpr int PQROWS = 16 * PWAVES;   // 128 query rows per workgroup
constexpr int PPT = PKT / 4 / PWAVES; // 16-row forms: 1-KiB LDS-DMA pieces of a K (or V) tile per wave
typedef __fp16 pv4hp __attribute__((__vector_size__(4 * sizeof(__fp16))));

struct PrefillArgs {
  const half_t* q; const half_t* k; const half_t* v; half_t* out;
  int64_t q_stride, k_stride, v_stride;     // elements between consecutive tokens
  const int* cu_q; const int* cu_k;
  const int* head_mask_type;                 // [Hq] or null (all dense)
  const int* streaming_info;                 // [2*Hq] (sink, local) or null
  int num_heads, num_kv_heads;
  int causal;
  int q_tiles;                               // > 0: 1-D grid, XCD-aware order (prefill_map_block)
  int xcd_split;                             // 1-D grid: XCDs that share the query tiles of one kv head (1, 2, 4 or 8)
  int gran_log2;                             // granularity of (sink, local): 0 tokens (token_streaming_attn_func), 7 blocks of 128
};                                           // tokens (block_streaming_attn_func): see first_local_key below

// What both host entry points ask of the layout: head dim 128, GQA by whole groups, rows of whole 16-B slots, and K / V token
// strides that fit the 32-bit byte strides of the tile addressing.
static inline bool prefill_layout_ok(int head_dim, int num_heads, int num_kv_heads, int64_t q_stride, int64_t k_stride,
                                     int64_t v_stride) {
  return head_dim == PDH && num_heads >= 1 && num_kv_heads >= 1 && num_heads % num_kv_heads == 0 && q_stride % 8 == 0 &&
         k_stride % 8 == 0 && v_stride % 8 == 0 && k_stride >= 0 && v_stride >= 0 && k_stride < (1LL << 31) &&
         v_stride < (1LL << 31);
}

// Streaming heads see the keys  key < sink << g  and  key >= first_local_key(qpos): the first key of the local window of the
// query at (bottom-right aligned) position qpos.  g = 0: qpos - local + 1 (the last `local` tokens, itself included); g = 7:
// the first token of block (qpos >> 7) - local + 1 (the query's own 128-token block and the local - 1 blocks before it).
__device__ __forceinline__ int first_local_key(int qpos, int local, int g) { return ((qpos >> g) - local + 1) * (1 << g); }
// A (sink, local) entry as the kernels use it: clamped to [0, (len_k >> g) + 1] units of 1 << g tokens, once per workgroup and
// before any shift or multiply.  (len_k >> g) + 1 units already cover every key of the sequence -- sink: ((len_k >> g) + 1) << g
// > len_k; local: qpos <= len_k - 1, so first_local_key <= 0 -- hence the clamp changes no element predicate and no tile
// predicate (skipped / full / win_lo all use the clamped pair), and it keeps sink << g and first_local_key inside int32 for
// every int32 entry: |first_local_key| <= len_q + len_k + (2 << g).  Unclamped, the block form wrapped from 1 << 24 on ("everything"
// put the window behind the query: rows of zeros), the token form for queries at negative positions (len_q > len_k).  Negative
// entries count as 0: no sink; no local key at or before the query.
__device__ __forceinline__ int window_units(int entry, int len_k, int g) { return min(max(entry, 0), (len_k >> g) + 1); }

// 1-D grid: workgroups are dealt round-robin to the 8 XCDs (private L2s; the dispatch is static: workgroup w runs on XCD
// w % 8 whatever the others are doing).  All q heads of a kv head share an XCD's L2, so a K/V tile is fetched from the
// fabric once per XCD that works on the head; the query tiles of a kv head are spread over W = xcd_split XCDs (tile t of
// part t % W) so that every XCD gets the same amount of DENSE work when some kv heads are streaming heads (LServe: a dense
// head costs O(L^2), a streaming head O(L * window); with whole kv heads pinned to XCDs the XCDs that drew streaming heads
// idle for most of the launch).  kv heads are taken dense-first: sorted position pos, part j -> XCD (pos * W + j) % 8.
// Returns false for the padding workgroups of a part that has fewer tiles.
__device__ __forceinline__ bool prefill_map_block(const PrefillArgs& p, int& b, int& h, int& qt) {
  const int W = p.xcd_split, Hk = p.num_kv_heads, G = p.num_heads / Hk;
  const int P = (Hk * W) >> 3;                       // (kv head, part) pairs per XCD
  const int R = (p.q_tiles + W - 1) / W;             // tile rows of a part
  const int wid = blockIdx.x, xcd = wid & 7;
  int slot = wid >> 3;
  const int u = slot % G; slot /= G;
  const int i = slot % P; slot /= P;
  const int r = slot % R;
  b = slot / R;
  const int idx = xcd + 8 * i, pos = idx / W, j = idx - pos * W;
  qt = p.q_tiles - 1 - (r * W + j);                  // long (late) query tiles first
  int kvh = pos;
  if (p.head_mask_type != nullptr) {                 // pos-th kv head in dense-first order (Hk scalar loads, once)
    int nd = 0;
    for (int t = 0; t < Hk; ++t) nd += p.head_mask_type[t * G] >= 0;
    const bool want_dense = pos < nd;
    int left = want_dense ? pos : pos - nd;
    kvh = 0;
    for (int t = 0; t < Hk; ++t) {
      const bool dense = p.head_mask_type[t * G] >= 0;
      if (dense == want_dense) {
        if (left == 0) { kvh = t; break; }
        --left;
      }
    }
  }
  h = kvh * G + u;
  return qt >= 0;
}

// ---- the 16-row tile body ----------------------------------------------------------------------------------------------
// A wave owns 16 query rows; lane (l15, l4) = (lane & 15, lane >> 4) works on query row l15 of them.  Scalars come by
// reference on purpose: a by-value parameter is evaluated at the call, in front of the body, and that alone reorders the
// address arithmetic of the kernels that call these.

// B operand of S^T = K Q^T: Q[row][32s + 8*l4 + (0..7)]; a row behind the sequence reads the last one (and is never stored)
__device__ __forceinline__ void load_q16(const half_t* const& q, const int64_t& q_stride, const int& q_begin, const int& qrow,
                                         const int& len_q, const int& h, const int& l4, v8h (&qb)[4]) {
  const int qr_c = qrow < len_q ? qrow : (len_q - 1);
  const half_t* qp = q + (size_t)(q_begin + qr_c) * q_stride + (size_t)h * PDH + 8 * l4;
#pragma unroll
  for (int s = 0; s < 4; ++s) qb[s] = *reinterpret_cast<const v8h*>(qp + 32 * s);
}

// S^T tile: 4 blocks of 16 keys.  A = K rows from the tile (XOR-swizzled slots: conflict-free ds_read_b128), B = Q.
// st[u][r] = K[kb + 16u + 4*l4 + r] . Q[qrow]
__device__ __forceinline__ void stage_s16(const uint8_t* kt, const v8h (&qb)[4], const int& l15, const int& l4, v4f (&st)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) st[u] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int key = 16 * u + l15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const v8h a = *reinterpret_cast<const v8h*>(kt + key * PROW + (((4 * s + l4) ^ l15) << 4));
      st[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qb[s], st[u], 0, 0, 0);
    }
  }
}

// V^T operand of O^T += V^T P^T: row 4*l4 + l15/4 (+16, +32, +48 by immediates), 8 B at logical offset 32c + 8*(l15&3); the
// physical 32-B block of logical block c is c ^ (row & 7).  Returns the address of block 0; block c: tr_a0 ^ (c << 5).
__device__ __forceinline__ int pv16_lane_addr(int l15, int l4) {
  const int trow = 4 * l4 + (l15 >> 2);
  return (trow * PROW + (l15 & 3) * 8) | ((trow & 7) << 5);
}

// O^T += V^T P^T: 16 steps (kk, c), each = two transposed reads (ds_read_b64_tr_b16: the A operand V^T) + one MFMA.  The
// schedule is pinned with sched_group_barrier: the reads run three steps ahead of the MFMAs (three operand quads in flight,
// counted lgkmcnt waits).  Left alone the compiler reuses ONE operand quad: read -> lgkmcnt(0) -> MFMA sixteen times per
// tile (PMC: 44 % of the wave cycles parked on counters).
__device__ __forceinline__ void stage_pv16(const uint8_t* vt, const int& tr_a0, const v8h (&pb)[2], v4f (&oacc)[8]) {
  v8h a16[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int kk = i >> 3, c = i & 7;
    // the xor is written per step: eight addresses kept across the tile loop cost eight VGPRs, which pushes the kernels over
    // the 128 that four waves per SIMD allow
    const uint8_t* src = vt + (32 * kk) * PROW + (tr_a0 ^ (c << 5));
    const pv4hp lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
        (__attribute__((address_space(3))) pv4hp*)(__attribute__((address_space(3))) void*)(src));
    const pv4hp hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
        (__attribute__((address_space(3))) pv4hp*)(__attribute__((address_space(3))) void*)(src + 16 * PROW));
    a16[i] = (v8h){(half_t)lo[0], (half_t)lo[1], (half_t)lo[2], (half_t)lo[3],
                   (half_t)hi[0], (half_t)hi[1], (half_t)hi[2], (half_t)hi[3]};
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) oacc[i & 7] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16[i], pb[i >> 3], oacc[i & 7], 0, 0, 0);
  __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);          // DS reads of steps 0..2
#pragma unroll
  for (int i = 0; i < 13; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);        // MFMA of step i
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);        // DS reads of step i + 3
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
}

// Finish: row sum over the 4 lanes of a query row, normalise, store.  A row that saw no key (l = 0) is written as zeros.
__device__ __forceinline__ void store_rows16(half_t* const& out, const int& q_begin, const int& qrow, const int& len_q,
                                             const int& num_heads, const int& h, const int& l4, const float& l_run,
                                             const v4f (&oacc)[8]) {
  const float l = rows4_sum(l_run);
  if (qrow >= len_q) return;
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  half_t* op = out + ((size_t)(q_begin + qrow) * num_heads + h) * PDH + 4 * l4;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    typedef _Float16 v4h_t __attribute__((ext_vector_type(4)));
    const v4h_t o = {(half_t)(oacc[c][0] * inv), (half_t)(oacc[c][1] * inv), (half_t)(oacc[c][2] * inv),
                     (half_t)(oacc[c][3] * inv)};
    *reinterpret_cast<v4h_t*>(op + c * 16) = o;
  }
}

}  // namespace omni
