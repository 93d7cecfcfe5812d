"""Case builders and expected values for the multi-token decode attention (omni_decode_attention_multi_kv4: 0 - 8 new tokens per
sequence over the KV4 pages): numpy + oracle only, shared by the CPU and GPU tests.  Built on tests/paged_prefill_cases.py: the
semantics are the paged prefill attention's, so are the case class (Case), the f64 expectation (expected_attention) and the
poisoning of the slots at positions >= past (poison_from_past)."""
import numpy as np

from tests import paged_prefill_cases as pc

D = pc.D
MAX_Q = 8

# (past, len_q) grid, PER GQA FAMILY: past in {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 200} x len_q in {1, 2, 3, 5, 8} = 55 pairs,
# thinned to 33: every past keeps three of the five lengths (so every past appears three times in every family, every len_q six
# or seven times), the kept lengths rotating with the past and with the family's shift, so that the tile edges (15 / 16 / 17, 63 /
# 64 / 65, 127 / 128) meet short and full windows and the four families together hold every one of the 55 pairs.  One family per
# GQA ratio (rows per kv head = ratio x len_q: up to 64 at ratio 8 = four 16-row tiles, 56 at ratio 7 = a ragged last tile),
# tokens_per_block alternating; the shifts put the full window n = 8 of ratios 8 and 7 on past 0, 63 / 64, 128 and 200.
PASTS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 200]
LENS = [1, 2, 3, 5, 8]


def thinned_pairs(shift):
    return [(past, LENS[(2 * i + shift + off) % 5]) for i, past in enumerate(PASTS) for off in (0, 1, 3)]


FAMILIES = {
    # name: (Hq, Hk, tokens_per_block, pairs)
    "gqa1_tpb16": (2, 2, 16, thinned_pairs(2)),
    "gqa4_tpb64": (8, 2, 64, thinned_pairs(4)),
    "gqa7_tpb16": (7, 1, 16, thinned_pairs(3)),
    "gqa8_tpb64": (16, 2, 64, thinned_pairs(1)),
}
# forced KV split counts (0 = the planner's): 7 splits at past 1 ... 17 leave splits without a past token
SPLITS = [0, 1, 2, 3, 7]
MIXED_BATCH = [(0, 8), (200, 0), (65, 3), (0, 0), (130, 1), (17, 8)]


def family(name):
    Hq, Hk, tpb, pairs = FAMILIES[name]
    return pc.Case(pairs, Hq, Hk, tpb, seed=sum(map(ord, name)) + 1000)


def mixed():
    return pc.Case(MIXED_BATCH, 8, 2, 64, seed=131)


class NeedleBatch:
    """One pool and one block table shared by B = past + n sequences (past 150, tokens_per_block 16, 8 / 2 heads, n = 3 new
    tokens, the same three for every sequence).  All q rows of sequence b equal the key at position b as the kernel sees it:
    the dequantised page key for b < past, the fresh fp16 key b - past behind it.  So every position in turn takes nearly all of
    the softmax mass of the rows that may see it, and a key that is dropped, counted twice or leaked through the causal mask
    moves the output by far more than the bar: row i of sequence past + j with j > i aims at a fresh key it must NOT see.
    Keys and values are drawn at 1.5 x the standard normal: the needle's score |k|^2 / sqrt(128) is then ~25 against ~N(0, 2.3^2)
    for the others (tests/test_decode_multi_cpu.py checks the resulting mass)."""

    def __init__(self, past=150, n=3, Hq=8, Hk=2, tpb=16, seed=77):
        rng = np.random.default_rng(seed)
        base = pc.Case([(past, n)], Hq, Hk, tpb, seed=seed, write_past=False)
        width = (Hq + 2 * Hk) * D
        hist = (1.5 * rng.standard_normal((past, width))).astype(np.float16)
        pc.write_at(hist, np.asarray([past], np.int32), np.zeros(1, np.int32), base)
        fresh = pc.rotate((1.5 * rng.standard_normal((n, width))).astype(np.float16), [n], [past], Hq, Hk)
        _, k_f, v_f = base.split(fresh)
        self.B = B = past + n
        self.past, self.n, self.Hq, self.Hk, self.tpb, self.T = past, n, Hq, Hk, tpb, B * n
        self.kc, self.vc = base.kc, base.vc
        self.kidx, self.vidx = np.repeat(base.kidx, B, axis=0), np.repeat(base.vidx, B, axis=0)
        self.pasts = np.full(B, past, np.int32)
        self.lens = np.full(B, n, np.int32)
        self.cu = (np.arange(B + 1) * n).astype(np.int32)
        # the keys as the kernel sees them: [past + n, Hk, D]
        self.keys = np.empty((past + n, Hk, D), np.float16)
        self.vals = np.empty((past + n, Hk, D), np.float16)
        for h in range(Hk):
            self.keys[:past, h] = self.kc.read_tokens(base.kidx[0], h, past, fp16_math=True)
            self.vals[:past, h] = self.vc.read_tokens(base.vidx[0], h, past, fp16_math=True)
        self.keys[past:], self.vals[past:] = k_f, v_f
        G = Hq // Hk
        q = np.repeat(self.keys[:, None], n, axis=1)                       # [B, n, Hk, D]: sequence b aims at key b
        self.q = np.ascontiguousarray(np.repeat(q, G, axis=2).reshape(B * n, Hq, D))
        self.k_new = np.ascontiguousarray(np.tile(k_f, (B, 1, 1)))
        self.v_new = np.ascontiguousarray(np.tile(v_f, (B, 1, 1)))
        # the fused rows, for the kernel's strided views
        self.qkv_rot = np.concatenate([self.q.reshape(B * n, -1), self.k_new.reshape(B * n, -1),
                                       self.v_new.reshape(B * n, -1)], axis=1)

    def expected(self):
        """f64 softmax over the visible keys, per (sequence, token, head) -> (fp16 [T, Hq, D], needle mass [B, n, Hq], NaN where the
        row may not see its needle)."""
        B, n, Hq, G, past = self.B, self.n, self.Hq, self.Hq // self.Hk, self.past
        out = np.empty((B, n, Hq, D), np.float64)
        mass = np.full((B, n, Hq), np.nan)
        K, V = self.keys.astype(np.float64), self.vals.astype(np.float64)
        q = self.q.astype(np.float64).reshape(B, n, Hq, D)
        for i in range(n):
            vis = past + i + 1
            for h in range(Hq):
                s = q[:, i, h] @ K[:vis, h // G].T / np.sqrt(D)                # [B, vis]
                p = np.exp(s - s.max(axis=1, keepdims=True))
                p /= p.sum(axis=1, keepdims=True)
                out[:, i, h] = p @ V[:vis, h // G]
                seen = np.arange(B) < vis
                mass[seen, i, h] = p[np.arange(B)[seen], np.arange(B)[seen]]
        return out.reshape(B * n, Hq, D).astype(np.float16), mass
