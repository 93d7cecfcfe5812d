"""Case builders and expected values for the prefill pair that continues from the KV4 page cache
(omni_kv4_prefill_write_at, omni_prefill_attention_paged_kv4): numpy + oracle only, shared by the CPU and GPU tests.

Expected pages:      oracle.kv4.rope_neox at position past + i, then PagedKV4.write_token.
Expected attention:  oracle.attention.varlen_attention (f64 softmax, causal, bottom-right aligned) over, per sequence and kv
                     head, K / V = concat(PagedKV4.read_tokens(table, h, past, fp16_math=True), k_new / v_new)."""
import numpy as np

from oracle import attention as oa
from oracle import kv4

D = 128
ROPE_BASE = 500000.0
FILL = 0x5A


class Case:
    """One batch: `pasts[b]` tokens of sequence b are in the pools (kc, vc: oracle.kv4.PagedKV4), `lens[b]` new tokens follow.
    qkv_raw / qkv_rot: the new tokens' fused rows before / after the RoPE at positions past + i.  Block tables are shuffled and
    non-contiguous (kidx / vidx: page indices [B, pages]); their last column is a sentinel page no token maps to."""

    def __init__(self, pairs, Hq, Hk, tpb, seed, write_past=True):
        rng = np.random.default_rng(seed)
        self.pasts = np.asarray([p for p, _ in pairs], np.int32)
        self.lens = np.asarray([n for _, n in pairs], np.int32)
        self.Hq, self.Hk, self.tpb, self.B = Hq, Hk, tpb, len(pairs)
        self.pages = int((self.pasts + self.lens).max()) // tpb + 2          # last column: sentinel
        n_pages = self.B * self.pages + 3
        self.kidx = rng.permutation(n_pages)[: self.B * self.pages].reshape(self.B, self.pages)
        self.vidx = rng.permutation(n_pages)[: self.B * self.pages].reshape(self.B, self.pages)
        self.kc = kv4.PagedKV4(n_pages, Hk, D, tpb, fill=FILL)
        self.vc = kv4.PagedKV4(n_pages, Hk, D, tpb, fill=FILL)
        width = (Hq + 2 * Hk) * D
        if write_past:
            hist = rng.standard_normal((int(self.pasts.sum()), width)).astype(np.float16)
            write_at(hist, self.pasts, np.zeros(self.B, np.int32), self)
        self.cu = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        self.T = int(self.cu[-1])
        self.qkv_raw = rng.standard_normal((self.T, width)).astype(np.float16)
        self.qkv_rot = rotate(self.qkv_raw, self.lens, self.pasts, Hq, Hk)

    def split(self, qkv):
        Hq, Hk = self.Hq, self.Hk
        T = qkv.shape[0]
        return (qkv[:, : Hq * D].reshape(T, Hq, D), qkv[:, Hq * D:(Hq + Hk) * D].reshape(T, Hk, D),
                qkv[:, (Hq + Hk) * D:].reshape(T, Hk, D))


def positions(lens, pasts):
    return np.concatenate([np.arange(int(n)) + int(p) for n, p in zip(lens, pasts)] + [np.zeros(0, np.int64)]).astype(np.int64)


def rotate(qkv_raw, lens, pasts, Hq, Hk):
    """The fused rows with q and k rotated (neox) at position past + i; v unchanged."""
    out = np.array(qkv_raw, np.float16, copy=True)
    T = out.shape[0]
    if T == 0:
        return out
    pos = positions(lens, pasts)[:, None]
    qk = out[:, : (Hq + Hk) * D].reshape(T, Hq + Hk, D)
    out[:, : (Hq + Hk) * D] = kv4.rope_neox(qk, np.broadcast_to(pos, (T, Hq + Hk)), ROPE_BASE).reshape(T, -1)
    return out


def write_at(qkv_raw, lens, pasts, case):
    """Expected effect of the writer at an offset on the case's pools; returns the rotated rows."""
    rot = rotate(qkv_raw, lens, pasts, case.Hq, case.Hk)
    _, k, v = case.split(rot)
    pos = positions(lens, pasts)
    tok = 0
    for b, n in enumerate(lens):
        for _ in range(int(n)):
            p = int(pos[tok])
            for h in range(case.Hk):
                case.kc.write_token(int(case.kidx[b][p // case.tpb]), p % case.tpb, h, k[tok, h])
                case.vc.write_token(int(case.vidx[b][p // case.tpb]), p % case.tpb, h, v[tok, h])
            tok += 1
    return rot


def expected_attention(q, k_new, v_new, cu, pasts, kc, vc, kidx, vidx):
    """q [T, Hq, D], k_new / v_new [T, Hk, D] fp16 (already rotated) -> fp16 [T, Hq, D]."""
    Hk = k_new.shape[1]
    ks, vs, cu_k = [], [], [0]
    for b in range(len(pasts)):
        past, a, e = int(pasts[b]), int(cu[b]), int(cu[b + 1])
        kb = np.empty((past + e - a, Hk, D), np.float16)
        vb = np.empty((past + e - a, Hk, D), np.float16)
        for h in range(Hk):
            kb[:past, h] = kc.read_tokens(kidx[b], h, past, fp16_math=True)      # exact fp16 values
            vb[:past, h] = vc.read_tokens(vidx[b], h, past, fp16_math=True)
        kb[past:], vb[past:] = k_new[a:e], v_new[a:e]
        ks.append(kb); vs.append(vb)
        cu_k.append(cu_k[-1] + past + e - a)
    return oa.varlen_attention(q, np.concatenate(ks), np.concatenate(vs), cu, np.asarray(cu_k), causal=True)


def case_expected_attention(case):
    q, k, v = case.split(case.qkv_rot)
    return expected_attention(q, k, v, case.cu, case.pasts, case.kc, case.vc, case.kidx, case.vidx)


def poison_from_past(case, cache, idx):
    """A copy of the pool with every slot at a position >= past of every page the tables name (the rest of the last partial
    page, the chunk's own slots, the pages behind them, the sentinel page) set to data 0xFF, scale = zero = fp16 NaN."""
    import copy
    c = copy.copy(cache)
    c.pool = cache.pool.copy()
    nan = np.float16(np.nan)
    for b in range(case.B):
        for pg in range(case.pages):
            lo = max(int(case.pasts[b]) - pg * case.tpb, 0)
            if lo >= case.tpb:
                continue
            page = int(idx[b][pg])
            c.data(page)[:, lo:] = 0xFF
            c.scales(page)[:, lo:] = nan
            c.zeros(page)[:, lo:] = nan
    return c


# (past, len_q) grid of the attention tests: past in {1, 15, 16, 17, 63, 64, 65, 127, 128, 200} x len_q in {1, 5, 16, 17, 128,
# 129, 200}, thinned to 32 pairs: every past and every len_q at least three times, the tile edges (63 / 64 / 65, 127 / 128 /
# 129) against each other.  One family per GQA ratio, tokens_per_block alternating.
ATTENTION_FAMILIES = {
    # name: (Hq, Hk, tokens_per_block, pairs)
    "gqa1_tpb16": (2, 2, 16, [(1, 1), (15, 17), (16, 128), (17, 5), (63, 129), (64, 16), (65, 200), (127, 1)]),
    "gqa4_tpb64": (8, 2, 64, [(1, 129), (16, 1), (63, 5), (64, 200), (65, 17), (128, 128), (200, 16), (200, 129)]),
    "gqa7_tpb16": (7, 1, 16, [(15, 200), (17, 128), (63, 16), (64, 1), (65, 129), (127, 17), (128, 5), (200, 200)]),
    "gqa8_tpb64": (16, 2, 64, [(1, 16), (15, 5), (16, 17), (64, 129), (127, 128), (128, 1), (128, 200), (200, 17)]),
}
MIXED_BATCH = [(0, 40), (200, 0), (65, 129), (0, 0), (130, 1)]
