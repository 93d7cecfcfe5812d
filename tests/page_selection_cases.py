"""Cases for the LServe page choice (numpy and oracle only: shared by tests/test_page_selection_cpu.py and
tests/test_page_selection_gpu.py, as tests/decode_score_profiles.py is shared by the decode-profile tests).

Three families:

* TOPK: fp16 selector scores written by hand (no selector involved, no NaN) for fused_ext.select_topk_pages.  The expected
  pages are oracle.kv4.topk_pages: descending page score (maximum over the page's sub-chunks), ties to the lower page,
  -0 == +0, newest page last.  Every scores array is [B, Hq, total_pages * subs]: the newest page's sub-chunks are present
  (and must be ignored).
* SELECTOR: real pages -- keys pooled into NaN-poisoned page tails, then scored.  Histories end on, one before and one after a
  selector workgroup boundary (32 pages), sub-chunk counts per page of 8, 16, 1 and 2 (the first two give the workgroup's loop
  over its sub-chunks a second and a fourth trip).
* CHAIN: one decode step's prefill + decode inputs with planted pages, for selector -> top-k -> sparse attention.
"""
import dataclasses
import functools

import numpy as np

from oracle import kv4

D = 128
ROPE_BASE = 500000.0
F16 = np.float16
NAN_BITS = 0x7E00           # fp16 quiet NaN: poison of every statistic slot the pool must not write


# ---- fp16 helpers ------------------------------------------------------------------------------------------------------
def f16_key(x):
    """Monotone integer image of fp16 values (-0 and +0 both 0): differences are distances in ulp."""
    b = np.ascontiguousarray(np.asarray(x, F16)).view(np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def f16_from_key(key):
    key = np.asarray(key, np.int32)
    bits = np.where(key >= 0, key, 0x8000 | -key).astype(np.uint16)
    return bits.view(F16)


def f16_below(x, steps):
    """The fp16 value `steps` ulp below x (stops at -inf)."""
    return f16_from_key(np.maximum(f16_key(x) - np.asarray(steps, np.int32), -0x7C00))


def spread(page_scores, subs, rng, newest=None, position=None):
    """page scores [B, H, n] -> sub-chunk scores [B, H, (n + 1) * subs] whose per-page maximum is page_scores: one sub-chunk
    (position[b, h, p], random by default) holds the page's score, each other one the same value again, a value 1..40 ulp
    below, -65504 or -inf.  The newest page's sub-chunks (`newest`, N(0, 1) by default) close the row."""
    ps = np.asarray(page_scores, F16)
    B, H, n = ps.shape
    pos = rng.integers(0, subs, (B, H, n)) if position is None else position
    kind = rng.integers(0, 4, (B, H, n, subs))
    below = f16_below(ps[..., None], rng.integers(1, 41, (B, H, n, subs)))
    other = np.where(kind == 0, ps[..., None], np.where(kind == 1, below, np.where(kind == 2, F16(-65504.0), F16(-np.inf))))
    other = np.minimum(other, ps[..., None])        # a page of -inf (or -65504) stays one
    sc = np.where(np.arange(subs) == pos[..., None], ps[..., None], other).astype(F16)
    last = rng.standard_normal((B, H, subs)).astype(F16) if newest is None else np.broadcast_to(F16(newest), (B, H, subs))
    return np.concatenate([sc.reshape(B, H, n * subs), last], axis=-1)


@dataclasses.dataclass(frozen=True)
class TopkCase:
    name: str
    scores: np.ndarray          # fp16 [B, Hq, total_pages * subs], read-only
    subs: int
    total_pages: int
    k: int
    tail: tuple = None          # tie cases: (first slot, pages) -- out[..., first : first + len(pages)] must be `pages`

    @property
    def n(self):
        return self.total_pages - 1

    def page_scores(self):
        B, H, _ = self.scores.shape
        return self.scores[:, :, : self.n * self.subs].reshape(B, H, self.n, self.subs).max(axis=-1)

    def want(self):
        return kv4.topk_pages(self.scores, self.subs, self.total_pages, self.k)


# ---- synthetic top-k cases -----------------------------------------------------------------------------------------------
TIE_N, TIE_LO, TIE_HI, TIE_ABOVE = 2500, 100, 900, 50
TIE_K = {"straddled": 350, "whole": 850, "untouched": 50}
EQUAL_N, EQUAL_K = 700, 300
FEW_N, FEW_KS = 1500, (1, 100, 700, 1024)
FEW_VALUES = np.array([-np.inf, -65504.0, -1000.0, -3.0, -1.0, -0.5, -6.1e-5, -3e-5, -6e-8, 0.0, 6e-8, 1.2e-7, 3e-5, 6.1e-5,
                       1e-3, 0.1, 0.25, 0.5, 0.999, 1.0, 1.001, 1.5, 2.0, 3.0, 7.0, 10.0, 33.0, 100.0, 255.0, 256.0, 1000.0,
                       2048.0, 4096.0, 30000.0, 65472.0, 65504.0, np.inf]).astype(F16)
SIZES = [(0, 0), (1, 0), (1, 1), (2, 1), (255, 254), (256, 256), (2049, 1), (2049, 1024), (14336, 1024), (14336, 0)]
SUBS = (1, 2, 3, 4, 8, 16)


def tie_row(rng):
    """Page scores [TIE_N]: TIE_ABOVE pages strictly above 1.0, pages TIE_LO .. TIE_HI - 1 exactly 1.0, the rest below."""
    row = (1.0 - rng.uniform(0.001, 4.0, TIE_N)).astype(F16)
    outside = np.concatenate([np.arange(TIE_LO), np.arange(TIE_HI, TIE_N)])
    above = rng.choice(outside, TIE_ABOVE, replace=False)
    row[above] = (1.0 + rng.uniform(0.001, 3.0, TIE_ABOVE)).astype(F16)
    row[TIE_LO:TIE_HI] = 1.0
    return row


@functools.lru_cache(maxsize=None)
def topk_cases():
    cases = []

    def add(name, scores, subs, k, tail=None):
        scores = np.ascontiguousarray(scores, F16)
        scores.setflags(write=False)
        cases.append(TopkCase(name, scores, subs, scores.shape[-1] // subs, k, tail))

    # a tie group of 800 pages over / inside / outside the k-th place; two heads with different pages above the group
    for subs in (1, 4):
        rng = np.random.default_rng(11)
        rows = np.stack([tie_row(rng), tie_row(rng)])[None]
        sc = spread(rows, subs, rng)
        for what, k in TIE_K.items():
            take = min(max(k - TIE_ABOVE, 0), TIE_HI - TIE_LO)
            add("ties_%s_subs%d" % (what, subs), sc, subs, k, (TIE_ABOVE, tuple(range(TIE_LO, TIE_LO + take))))
    # all-equal rows: +0, -0, a mix of both (also inside a page)
    rng = np.random.default_rng(12)
    for subs in (2, 4):
        z = np.zeros((1, 3, (EQUAL_N + 1) * subs), np.uint16)
        z[0, 1] = 0x8000
        z[0, 2] = np.where(rng.integers(0, 2, z.shape[-1]) == 1, 0x8000, 0)
        add("all_equal_subs%d" % subs, z.view(F16), subs, EQUAL_K, (0, tuple(range(EQUAL_K))))
    # 37 distinct values: every k lands inside a tie group
    rng = np.random.default_rng(13)
    few = FEW_VALUES[rng.integers(0, FEW_VALUES.size, (1, 3, FEW_N))]
    for subs in (1, 4):
        sc = spread(few, subs, rng)
        for k in FEW_KS:
            add("few_values_k%d_subs%d" % (k, subs), sc, subs, k)
    # every finite fp16 bit pattern is a possible score
    rng = np.random.default_rng(14)
    bits = rng.integers(0, 1 << 16, (2, 2, 3000 * 4)).astype(np.uint16)
    bits = np.where((bits & 0x7C00) == 0x7C00, bits & 0x83FF, bits).astype(np.uint16)      # inf / NaN -> subnormals
    full = np.concatenate([bits.view(F16), np.zeros((2, 2, 4), F16)], axis=-1)
    add("full_range", full, 4, 512)
    # sizes, the declared limits among them (n = 14336 candidates, k = 1024)
    for n, k in SIZES:
        for subs in (1, 4):
            rng = np.random.default_rng(1000 * n + k)
            add("size_n%d_k%d_subs%d" % (n, k, subs), spread(rng.standard_normal((1, 3, n)).astype(F16), subs, rng), subs, k)
    # sub-chunks per page: the maximum of page p of head h sits alone in sub-chunk (p + h) % subs
    for subs in SUBS:
        rng = np.random.default_rng(15 + subs)
        ps = rng.standard_normal((1, 2, 600)).astype(F16)
        pos = (np.arange(600)[None, None, :] + np.arange(2)[None, :, None]) % subs
        below = f16_below(ps[..., None], rng.integers(1, 2000, (1, 2, 600, subs)))
        sc = np.where(np.arange(subs) == pos[..., None], ps[..., None], below).astype(F16).reshape(1, 2, 600 * subs)
        sc = np.concatenate([sc, rng.standard_normal((1, 2, subs)).astype(F16)], axis=-1)
        add("subs%d" % subs, sc, subs, 100)
    # the newest page scores +inf in every sub-chunk: it is appended, never ranked
    for subs in (2, 4):
        rng = np.random.default_rng(16 + subs)
        add("newest_inf_subs%d" % subs, spread(rng.standard_normal((2, 2, 300)).astype(F16), subs, rng, newest=np.inf), subs, 10)
    return tuple(cases)


def topk_case(name):
    return next(c for c in topk_cases() if c.name == name)


# ---- selector cases ------------------------------------------------------------------------------------------------------
SEL_PAGES = 32              # pages per selector workgroup (csrc/sparse_utils.hip: SEL_PB)
SEL_FLAGS = (1, 0, 1)       # kv heads: retrieval, streaming, retrieval
SEL_SHAPES = [(64, 8), (64, 4), (64, 64), (16, 8)]


@dataclasses.dataclass(frozen=True)
class SelectorSpec:
    name: str
    tpb: int
    sub: int
    group: int              # q heads per kv head
    hist: tuple             # history length per sequence (current token excluded)
    rope_scale: float = 1.0  # rotary_embedding_scale of the product call; the oracle's rope_scale is its inverse


def _selector_specs():
    specs = []
    for tpb, sub in SEL_SHAPES:
        for m, group in ((1, 2), (2, 3)):
            edge = SEL_PAGES * tpb * m
            specs.append(SelectorSpec("tpb%d_sub%d_m%d" % (tpb, sub, m), tpb, sub, group,
                                      (edge - 1, sub - 1, edge, 0, edge + 1)))
    specs.append(SelectorSpec("tpb64_sub8_rope_scale4", 64, 8, 2, (2049, 0, 700), 4.0))
    return specs


SELECTOR_SPECS = _selector_specs()


class SelectorCase:
    """Keys, q, page table and the oracle's results of one spec.  `pool0` is the poisoned pool before pooling, `pool` after
    (oracle.kv4.paged_min_max_pool), `want` the oracle's scores.  All read-only."""

    def __init__(self, spec):
        self.spec = spec
        tpb, sub = spec.tpb, spec.sub
        rng = np.random.default_rng(sum(map(ord, spec.name)))
        self.flags = np.asarray(SEL_FLAGS, np.int32)
        self.pooled = [h for h, f in enumerate(SEL_FLAGS) if f]
        self.H, self.Hk = len(self.pooled), len(SEL_FLAGS)
        self.Hq = self.Hk * spec.group
        self.rank = np.asarray(kv4.head_classes(self.flags, self.Hq)["head_rank_table"], np.int32)
        self.B = len(spec.hist)
        self.lengths = (np.asarray(spec.hist) + 1).astype(np.int32)
        self.cu = np.concatenate([[0], np.cumsum(spec.hist)]).astype(np.int32)
        self.pages = max(spec.hist) // tpb + 2
        self.table = rng.permutation(self.B * self.pages).reshape(self.B, self.pages)
        self.page_bytes = kv4.stats_page_bytes(self.H, D, tpb, sub)
        self.stats_off = self.H * tpb * (D // 2 + 4)
        self.pool0 = np.full((self.B * self.pages, self.page_bytes), 0x11, np.uint8)
        self.pool0[:, self.stats_off:].view(np.uint16)[:] = NAN_BITS
        self.k = rng.standard_normal((int(self.cu[-1]), self.Hk, D)).astype(F16)
        self.q = rng.standard_normal((self.B, self.Hq, D)).astype(F16)
        self.pool = self.pool0.copy()
        kv4.paged_min_max_pool(self.k, self.cu, self.pooled, self.pool, self.table, tpb, sub)
        self.want = kv4.page_selector(self.q, self.lengths, self.flags, self.rank, self.pool, self.table, self.Hk, self.H,
                                      tpb, sub, ROPE_BASE, 1.0 / spec.rope_scale)
        for a in (self.table, self.pool0, self.pool, self.k, self.q, self.want):
            a.setflags(write=False)

    def n_sub(self, b):
        return (self.spec.hist[b] + self.spec.sub - 1) // self.spec.sub


@functools.lru_cache(maxsize=None)
def selector_case(name):
    return SelectorCase(next(s for s in SELECTOR_SPECS if s.name == name))


# ---- chain case ----------------------------------------------------------------------------------------------------------
CHAIN_TPB, CHAIN_SUB, CHAIN_BUDGET_PAGES = 64, 16, 6
CHAIN_HIST = 40 * CHAIN_TPB + 20        # 40 whole candidate pages + 20 tokens in the newest one, both sequences
CHAIN_FLAGS = (1, 0, 0, 1)
CHAIN_HQ = 8
CHAIN_SINK, CHAIN_LOCAL = 128, 256
NEEDLE_AMPS = (8.0, 5.5)                # two planted pages per retrieval q head
DECOY_GAINS = (1.55, 1.25)              # two louder pages per retrieval kv head
MARGIN_ULP = 8                          # the selector's 2 ulp on either side of a gap, twice


class ChainCase:
    """Inputs of prefill + one decode step (2 sequences of CHAIN_HIST tokens, Hq 8 over kv heads 1 0 0 1) with planted pages.

    A needle of retrieval q head h is one history key of h's kv head equal (after RoPE at its own position) to
    amp * RoPE(q_h, CHAIN_HIST) / rms: the page's statistics then bound q_h . k by ~128 * amp against ~180 for an N(0, 1) page.
    The other q head of the kv head sees about 0.4 of that.  A decoy is a page whose keys are all louder by a gain.  Each
    retrieval q head so has two needles of its own, the sibling's two and two decoys well apart from each other and from the
    rest: the six best pages are decided by margins far above the selector's tolerance (proved in test_page_selection_cpu.py)."""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.seq_lens = [CHAIN_HIST, CHAIN_HIST]
        self.flags = np.asarray(CHAIN_FLAGS, np.int32)
        Hq, Hk, T, B = CHAIN_HQ, len(CHAIN_FLAGS), CHAIN_HIST, 2
        g = Hq // Hk
        self.Hq, self.Hk, self.B = Hq, Hk, B
        self.total_pages = T // CHAIN_TPB + 1
        self.k_best = CHAIN_BUDGET_PAGES - 1
        self.retrieval_q_heads = [h for h in range(Hq) if CHAIN_FLAGS[h // g]]
        self.qkv_decode = rng.standard_normal((B, (Hq + 2 * Hk) * D)).astype(F16)
        qkv = rng.standard_normal((B * T, (Hq + 2 * Hk) * D)).astype(F16)
        q_rot = kv4.rope_neox(self.qkv_decode[:, : Hq * D].reshape(B, Hq, D), np.full((B, Hq), T), ROPE_BASE)
        keys = qkv[:, Hq * D:(Hq + Hk) * D].reshape(B, T, Hk, D)      # a view: edits land in qkv
        self.needles = {}
        for b in range(B):
            for hk in range(Hk):
                if not CHAIN_FLAGS[hk]:
                    continue
                pages = rng.permutation(self.total_pages - 1)[: 2 * g + len(DECOY_GAINS)]
                for j, gain in enumerate(DECOY_GAINS):
                    p = int(pages[2 * g + j])
                    keys[b, p * CHAIN_TPB:(p + 1) * CHAIN_TPB, hk] *= F16(gain)
                for i in range(g):
                    h = hk * g + i
                    u = q_rot[b, h].astype(np.float64)
                    u /= np.sqrt((u * u).mean())
                    self.needles[(b, h)] = []
                    for j, amp in enumerate(NEEDLE_AMPS):
                        p = int(pages[2 * i + j])
                        t = p * CHAIN_TPB + int(rng.integers(0, CHAIN_TPB))
                        keys[b, t, hk] = kv4.rope_neox((amp * u).astype(F16), np.asarray(-t), ROPE_BASE)   # inverse rotation
                        self.needles[(b, h)].append(p)
        self.qkv_prefill = qkv
        for a in (self.qkv_prefill, self.qkv_decode):
            a.setflags(write=False)

    def q(self):
        return self.qkv_decode[:, : self.Hq * D].reshape(self.B, self.Hq, D)

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        """(scores fp16 [B, Hq, 41 * 4], pages int32 [B, Hq, 6]) of the oracle's chain on a statistics-only pool."""
        Hq, Hk, T, B = self.Hq, self.Hk, CHAIN_HIST, self.B
        pos = np.tile(np.arange(T), B)
        k_post = kv4.rope_neox(self.qkv_prefill[:, Hq * D:(Hq + Hk) * D].reshape(B * T, Hk, D), pos[:, None], ROPE_BASE)
        heads = [h for h in range(Hk) if CHAIN_FLAGS[h]]
        rank = kv4.head_classes(self.flags, Hq)["head_rank_table"]
        pool = np.zeros((B * self.total_pages, kv4.stats_page_bytes(len(heads), D, CHAIN_TPB, CHAIN_SUB)), np.uint8)
        table = np.arange(B * self.total_pages).reshape(B, self.total_pages)
        cu = np.asarray([0, T, 2 * T], np.int32)
        kv4.paged_min_max_pool(k_post, cu, heads, pool, table, CHAIN_TPB, CHAIN_SUB)
        scores = kv4.page_selector(self.q(), np.full(B, T + 1, np.int32), self.flags, rank, pool, table, Hk, len(heads),
                                   CHAIN_TPB, CHAIN_SUB, ROPE_BASE)
        pages = kv4.select_topk_pages(scores, CHAIN_TPB, CHAIN_SUB, CHAIN_BUDGET_PAGES * CHAIN_TPB, T)
        return scores, pages


@functools.lru_cache(maxsize=None)
def chain_case():
    return ChainCase()
