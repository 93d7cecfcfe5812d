"""Decode-attention cases with a CONTROLLED score profile (numpy and oracle only: shared by tests/test_decode_profiles_cpu.py and
tests/test_decode_profiles_gpu.py, as tests/paged_prefill_cases.py is shared by the paged-prefill tests).

Every other decode parity test draws q, k, v from N(0, 1): the scores are about N(0, 1), the softmax is nearly flat, every
rescale factor and every merge weight is of order 1.  Here the history keys are written so that the score of token t is a chosen
a[t] (natural-log units):

* the decode kernel rotates q and the current k at position tlen; history keys sit in the pages post-RoPE.  u = rope_neox(q0, tlen)
  of the FIRST q head of a kv head is built as a +-c sign pattern with u.u / sqrt(128) = 1 (q0 is the inverse rotation of the
  pattern, rounded to fp16), and history key t is written as a[t] * u + small noise: its score against that head is ~a[t];
* a two-level row survives the 4-bit page format almost unchanged (codes 0 and 15), so the profile keeps its shape up to ~1e-3
  relative per score -- the reference reads the same pages, only the shape matters;
* the other q heads of the GQA group are q0 times a per-head gain (GAINS): the heads of one workgroup see different sharpness, the
  gain -1 head sees the reversed profile (a climb becomes a descent, an offset +c becomes -c);
* V rows are N(0, 1); a needle's V row is a fixed +-4 sign pattern, so a lost or mis-weighted needle is unmistakable;
* block tables are shuffled.

The expected values are an f64 softmax and P.V over `PagedKV4.read_tokens(..., fp16_math=True)` plus the un-quantised current
token, normalised with the reference kernel's 1 / (sum + 1e-6) and rounded ONCE to fp16: oracle/kv4.py::decode_attention with its
f32 score / softmax arithmetic replaced by f64 (same keys, values, RoPE, append).

Fairness (tests/test_decode_profiles_cpu.py::test_every_case_is_fair): a case may only sit in a table below if
oracle.kv4.decode_attention(emulate_fp16=False) -- f32 scores, f32 softmax -- lands within 5e-4 (tests.util.attention_errors, half
the project's 1e-3 bar) of the f64 expected values.  The measured distance of every case (rel L2 / max |d| per head max) is
recorded in FAIRNESS at the end of this file; the largest is 1.7e-5 / 1.7e-5 (an offset of 200), so no spread had to shrink.
"""
import copy
import functools

import numpy as np

from oracle import kv4

D = 128
ROPE_BASE = 500000.0
GAINS = (1.0, 0.5, -1.0, 0.25, -0.5, 0.75, -0.25, 0.125)
NEEDLE = 20.0          # a needle's score above a N(0, 1) background
NEEDLE_V = 4.0
SQRT_D = float(np.sqrt(D))


def split_tokens(context, nsplit):
    """Tokens per KV split as the planner rounds them (csrc/kv_cache.hip: plan_decode): a multiple of 16, not of 32."""
    return ((context + nsplit - 1) // nsplit + 15) & ~15


# ---- score profiles: (kind, arg) -> a[0..T-1], score of the current token, index of the planted token (or None) ---------
def profile_scores(kind, arg, T, rng):
    bg = rng.standard_normal(T)
    cur = float(rng.standard_normal())
    needle = None

    def sink_recency():
        a = bg.copy()
        n = min(8, max(T - 1, 0))
        if T > 0:
            a[0] = 12.0
        if n:
            a[T - n:] = np.linspace(3.0, 10.0, 8)[8 - n:]
        return a

    if kind == "needle":                       # arg: token index, "last" or "current"
        a = bg
        if arg == "current":
            cur, needle = NEEDLE, T
        else:
            needle = T - 1 if arg == "last" else int(arg)
            assert 0 <= needle < T, (arg, T)
            a[needle] = NEEDLE
    elif kind == "sink_recency":
        a = sink_recency()
    elif kind == "climb":                      # total range arg: every tile of every wave rescales, early tiles / splits underflow
        a = -arg + arg * np.arange(T) / max(T - 1, 1) + 0.1 * bg
        cur = 0.0
    elif kind == "descend":                    # the maximum is in the first tile; later splits merge with weight ~0
        a = -arg * np.arange(T) / max(T - 1, 1) + 0.1 * bg
        cur = -arg
    elif kind == "current":                    # arg: score of the current token against a flat history
        a = 0.5 * bg
        cur = float(arg)
    elif kind == "offset":                     # sink_recency with every score (the current token's too) shifted by arg
        a = sink_recency() + arg
        cur = cur + arg
    elif kind == "flat_exact":                 # identical history rows: exactly equal weights
        a = np.ones(T)
        cur = 1.0
    else:
        raise ValueError(kind)
    return a, cur, needle


class Seq:
    def __init__(self, T, kind, arg=None):
        self.T, self.kind, self.arg = int(T), kind, arg

    def __repr__(self):
        return "%s(%s)@%d" % (self.kind, self.arg, self.T) if self.arg is not None else "%s@%d" % (self.kind, self.T)


def needle_v_row(hk):
    sign = np.where((np.arange(D) * (hk + 3)) % 7 < 3, 1.0, -1.0)
    return (NEEDLE_V * sign).astype(np.float16)


def unit_query(rng, tlen, rope_scale=1.0):
    """(q0 fp16 [D], u f64 [D]): u = rope_neox(q0, tlen) is a +-c sign pattern (up to fp16 rounding) with u.u / sqrt(D) ~ 1."""
    c = np.sqrt(SQRT_D / D)
    target = (c * rng.choice([-1.0, 1.0], size=D)).astype(np.float16)
    q0 = kv4.rope_neox(target[None, :], np.asarray([-tlen]), ROPE_BASE, rope_scale)[0]
    u = kv4.rope_neox(q0[None, :], np.asarray([tlen]), ROPE_BASE, rope_scale)[0].astype(np.float64)
    return q0, u


def softmax_pv_f64(qr, kr, vr, Kc, Vc):
    """f64 restatement of the inner part of oracle/kv4.py::decode_attention for one q head: scores of the cached tokens and of the
    current one, softmax with 1 / (sum + 1e-6), P.V.  -> (unrounded output f64 [D], weights f64 [n + 1])."""
    qf = qr.astype(np.float64)
    s = np.concatenate([Kc.astype(np.float64) @ qf, [np.dot(qf, kr.astype(np.float64))]]) / SQRT_D
    e = np.exp(s - s.max())
    p = e / (e.sum() + 1e-6)
    vals = np.concatenate([Vc.astype(np.float64), vr[None, :].astype(np.float64)], axis=0)
    return p @ vals, p


class ProfileCase:
    """One dense KV4 decode call: sequences `seqs` (one Seq each), Hq / Hk heads, pages of tpb tokens, nsplit forced (0: planner).

    q, k, v       fp16 inputs of the call (raw: the kernel rotates q and k)
    lens          int32 context lengths including the current token
    kc0, vc0      the pools BEFORE the call (to upload);  kc, vc: after it (the current token appended, as the oracle appends)
    want          fp16 [B, Hq, D] expected output;  want64: the same before the rounding
    weights       {(b, hq): f64 [T + 1]} softmax weights (gain-1 heads only)
    needles       [(b, token index)] planted tokens (index T = the current token)
    """

    def __init__(self, name, seqs, Hq, Hk, tpb=64, nsplit=0, seed=0):
        self.name, self.seqs, self.Hq, self.Hk, self.tpb, self.nsplit = name, seqs, Hq, Hk, tpb, nsplit
        rng = np.random.default_rng(seed)
        B, g = len(seqs), Hq // Hk
        assert g <= len(GAINS)
        self.B, self.g = B, g
        self.context = max(s.T for s in seqs) + 1
        pages = self.context // tpb + 2
        n = B * pages
        self.kidx = rng.permutation(n).reshape(B, pages)
        self.vidx = rng.permutation(n).reshape(B, pages)
        kc, vc = kv4.PagedKV4(n, Hk, D, tpb, fill=0x5A), kv4.PagedKV4(n, Hk, D, tpb, fill=0x5A)
        self.q = np.zeros((B, Hq, D), np.float16)
        self.k = np.zeros((B, Hk, D), np.float16)
        self.v = rng.standard_normal((B, Hk, D)).astype(np.float16)
        self.lens = np.asarray([s.T + 1 for s in seqs], np.int32)
        self.needles, self.needle_v = [], {}
        for b, s in enumerate(seqs):
            T = s.T
            a, cur, needle = profile_scores(s.kind, s.arg, T, rng)
            if needle is not None:
                self.needles.append((b, needle))
            for hk in range(Hk):
                q0, u = unit_query(rng, T)
                for j in range(g):
                    self.q[b, hk * g + j] = (np.float32(GAINS[j]) * q0.astype(np.float32)).astype(np.float16)
                noise = 0.0 if s.kind == "flat_exact" else 0.02
                K = (a[:, None] * u[None, :] + noise * rng.standard_normal((T, D))).astype(np.float16)
                V = rng.standard_normal((T, D)).astype(np.float16)
                # the current k enters raw and is rotated by the kernel: cur * q0 rotates to ~cur * u
                self.k[b, hk] = (cur * q0.astype(np.float64) + noise * rng.standard_normal(D)).astype(np.float16)
                if needle is not None:
                    nv = needle_v_row(hk)
                    if needle == T:
                        self.v[b, hk] = nv
                    else:
                        V[needle] = nv
                for t in range(T):
                    kc.write_token(int(self.kidx[b][t // tpb]), t % tpb, hk, K[t])
                    vc.write_token(int(self.vidx[b][t // tpb]), t % tpb, hk, V[t])
        self.kc0, self.vc0 = copy.copy(kc), copy.copy(vc)
        self.kc0.pool, self.vc0.pool = kc.pool.copy(), vc.pool.copy()
        self.kc, self.vc = kc, vc
        self._expected()

    def _expected(self):
        """oracle/kv4.py::decode_attention with f64 scores, softmax and P.V (reads kc0 / vc0, appends to kc / vc)."""
        B, Hq, Hk, g = self.B, self.Hq, self.Hk, self.g
        self.want64 = np.zeros((B, Hq, D), np.float64)
        self.weights = {}
        for b in range(B):
            tlen = int(self.lens[b]) - 1
            qr = kv4.rope_neox(self.q[b], np.full((Hq,), tlen), ROPE_BASE)
            kr = kv4.rope_neox(self.k[b], np.full((Hk,), tlen), ROPE_BASE)
            for hk in range(Hk):
                Kc = self.kc0.read_tokens(self.kidx[b], hk, tlen, fp16_math=True)
                Vc = self.vc0.read_tokens(self.vidx[b], hk, tlen, fp16_math=True)
                for hq in range(hk * g, (hk + 1) * g):
                    o, p = softmax_pv_f64(qr[hq], kr[hk], self.v[b, hk], Kc, Vc)
                    self.want64[b, hq] = o
                    if hq == hk * g:
                        self.weights[(b, hq)] = p
                        for nb, nt in self.needles:       # the planted token's V row as the attention reads it
                            if nb == b:
                                self.needle_v[(b, hq)] = self.v[b, hk].astype(np.float32) if nt == tlen else Vc[nt]
                self.kc.write_token(int(self.kidx[b][tlen // self.tpb]), tlen % self.tpb, hk, kr[hk])
                self.vc.write_token(int(self.vidx[b][tlen // self.tpb]), tlen % self.tpb, hk, self.v[b, hk])
        self.want = self.want64.astype(np.float16)

    def oracle_f32(self):
        """oracle.kv4.decode_attention(emulate_fp16=False) on copies of the pools before the call -> (fp16 output, the f32
        values before that rounding)."""
        kc, vc = copy.copy(self.kc0), copy.copy(self.vc0)
        kc.pool, vc.pool = self.kc0.pool.copy(), self.vc0.pool.copy()
        raw = np.zeros((self.B, self.Hq, D), np.float32)
        out = kv4.decode_attention(self.q, self.k, self.v, self.lens, kc, vc, self.kidx, self.vidx, ROPE_BASE,
                                   emulate_fp16=False, out_f32=raw)
        assert np.array_equal(kc.pool, self.kc.pool) and np.array_equal(vc.pool, self.vc.pool)
        return out, raw


# ---- the case tables --------------------------------------------------------------------------------------------------
# geometry name -> (T, tpb, forced split count).  context = T + 1.
#   pipe1     one split of 701 tokens: DIRECT with PIPE
#   short7    7 splits of 112 tokens: a ragged last 32-token tile in every split, the short sweep form, the merge kernel
#   pipe2     2 splits of 704 tokens: PIPE with the merge
#   window2   pages of 16 tokens, 2 splits of 608 = 38 pages: 38 of the 40 window pointers
#   tile95 / tile33   the planner's choice (one split): single-tile sweeps per wave
GEOMETRIES = {
    "pipe1": (700, 64, 1),
    "short7": (700, 64, 7),
    "pipe2": (1400, 64, 2),
    "window2": (1200, 16, 2),
    "tile95": (95, 64, 0),
    "tile33": (33, 64, 0),
}
CLIMB, OFFSET = 60.0, 200.0


def needle_positions(T, tpb, nsplit):
    pos = [0, 31, 32, tpb - 1, tpb]
    if nsplit > 1:
        st = split_tokens(T + 1, nsplit)
        pos += [st - 1, st, 2 * st - 1]
    pos = sorted({p for p in pos if 0 <= p < T - 1})
    return pos + ["last", "current"]


def all_profiles(T, tpb, nsplit):
    prof = [("needle", p) for p in needle_positions(T, tpb, nsplit)]
    prof += [("sink_recency", None), ("climb", CLIMB), ("descend", CLIMB), ("current", 40.0), ("current", -40.0),
             ("offset", OFFSET), ("offset", -OFFSET), ("flat_exact", None)]
    return prof


def edge_profiles(T, tpb, nsplit):
    """The subset the other head layouts get: needle at the split edge, climb, descend, offset."""
    st = split_tokens(T + 1, nsplit)
    return [("needle", st - 1), ("needle", st), ("climb", CLIMB), ("descend", CLIMB), ("offset", OFFSET), ("offset", -OFFSET)]


def _chunks(items, n):
    return [items[i:i + n] for i in range(0, len(items), n)]


def dense_specs():
    """[(name, seqs, Hq, Hk, tpb, nsplit)]: at most 3 sequences per call."""
    specs = []
    for gname, (T, tpb, ns) in GEOMETRIES.items():
        for i, chunk in enumerate(_chunks(all_profiles(T, tpb, ns), 3)):
            specs.append(("%s-8x2-%d" % (gname, i), [Seq(T, k, a) for k, a in chunk], 8, 2, tpb, ns))
    for Hq, Hk in ((16, 2), (7, 1), (2, 2), (4, 2)):
        for gname in ("short7", "pipe2"):
            T, tpb, ns = GEOMETRIES[gname]
            for i, chunk in enumerate(_chunks(edge_profiles(T, tpb, ns), 3)):
                specs.append(("%s-%dx%d-%d" % (gname, Hq, Hk, i), [Seq(T, k, a) for k, a in chunk], Hq, Hk, tpb, ns))
    # a peaked long sequence next to a short one whose splits are empty but the last (forced 2 splits of 704 tokens)
    st = split_tokens(1401, 2)
    specs.append(("mixed-8x2-0", [Seq(1400, "needle", st - 1), Seq(5, "sink_recency"), Seq(1400, "climb", CLIMB)], 8, 2, 64, 2))
    specs.append(("mixed-8x2-1", [Seq(5, "needle", 0), Seq(1400, "descend", CLIMB), Seq(5, "offset", OFFSET)], 8, 2, 64, 2))
    return specs


def merge_specs():
    """The in-launch merge (8 / 2 heads, forced 2 and 7 splits): climb, descend, needle at the split edges, offset."""
    specs = []
    for T, ns in ((1400, 2), (700, 7)):
        st = split_tokens(T + 1, ns)
        prof = [("climb", CLIMB), ("descend", CLIMB), ("needle", st - 1), ("needle", st), ("offset", OFFSET), ("offset", -OFFSET)]
        for i, chunk in enumerate(_chunks(prof, 3)):
            specs.append(("merge%d-8x2-%d" % (ns, i), [Seq(T, k, a) for k, a in chunk], 8, 2, 64, ns))
    return specs


RANDOM_SPECS = [("random-8x2", [Seq(200, "random"), Seq(65, "random"), Seq(1, "random")], 8, 2, 64, 0),
                ("random-16x2", [Seq(700, "random"), Seq(130, "random")], 16, 2, 64, 0)]

DENSE = {s[0]: s for s in dense_specs()}
MERGE = {s[0]: s for s in merge_specs()}


@functools.lru_cache(maxsize=None)
def case(name):
    """The built case (inputs, pools, expected values): built once per process, shared by every test that names it."""
    spec = DENSE.get(name) or MERGE[name]
    n, seqs, Hq, Hk, tpb, ns = spec
    return ProfileCase(n, seqs, Hq, Hk, tpb, ns, seed=abs(hash_name(n)))


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def random_case(spec):
    """An ordinary N(0, 1) case (q, k, v and history all random) with the same expected-value builder."""
    name, seqs, Hq, Hk, tpb, ns = spec
    c = ProfileCase.__new__(ProfileCase)
    c.name, c.seqs, c.Hq, c.Hk, c.tpb, c.nsplit = name, seqs, Hq, Hk, tpb, ns
    rng = np.random.default_rng(hash_name(name))
    B = len(seqs)
    c.B, c.g = B, Hq // Hk
    c.context = max(s.T for s in seqs) + 1
    pages = c.context // tpb + 2
    n = B * pages
    c.kidx, c.vidx = rng.permutation(n).reshape(B, pages), rng.permutation(n).reshape(B, pages)
    kc, vc = kv4.PagedKV4(n, Hk, D, tpb, fill=0x5A), kv4.PagedKV4(n, Hk, D, tpb, fill=0x5A)
    c.q = rng.standard_normal((B, Hq, D)).astype(np.float16)
    c.k = rng.standard_normal((B, Hk, D)).astype(np.float16)
    c.v = rng.standard_normal((B, Hk, D)).astype(np.float16)
    c.lens = np.asarray([s.T + 1 for s in seqs], np.int32)
    c.needles, c.needle_v = [], {}
    for b, s in enumerate(seqs):
        for hk in range(Hk):
            K = rng.standard_normal((s.T, D)).astype(np.float16)
            V = rng.standard_normal((s.T, D)).astype(np.float16)
            for t in range(s.T):
                kc.write_token(int(c.kidx[b][t // tpb]), t % tpb, hk, K[t])
                vc.write_token(int(c.vidx[b][t // tpb]), t % tpb, hk, V[t])
    c.kc0, c.vc0 = copy.copy(kc), copy.copy(vc)
    c.kc0.pool, c.vc0.pool = kc.pool.copy(), vc.pool.copy()
    c.kc, c.vc = kc, vc
    c._expected()
    return c



# Measured by tests/test_decode_profiles_cpu.py::test_every_case_is_fair: distance of oracle.kv4.decode_attention(emulate_fp16=False)
# from the f64 expected values, rel L2 / max |d| per head max, before each side's rounding to fp16 (the condition: <= 5e-4) and,
# in brackets, after it (a single fp16 rounding-boundary flip at a head's largest element reads up to 9.8e-4 there).
FAIRNESS = """
pipe1-8x2-0      2.38e-07 / 2.54e-07   (fp16: 4.46e-05 / 5.04e-04)  [needle(0)@700, needle(31)@700, needle(32)@700]
pipe1-8x2-1      4.70e-07 / 4.71e-07   (fp16: 0.00e+00 / 0.00e+00)  [needle(63)@700, needle(64)@700, needle(last)@700]
pipe1-8x2-2      3.53e-06 / 4.16e-06   (fp16: 2.21e-05 / 8.00e-05)  [needle(current)@700, sink_recency@700, climb(60.0)@700]
pipe1-8x2-3      2.71e-06 / 3.00e-06   (fp16: 3.00e-07 / 1.17e-06)  [descend(60.0)@700, current(40.0)@700, current(-40.0)@700]
pipe1-8x2-4      1.08e-05 / 8.96e-06   (fp16: 1.23e-04 / 4.38e-04)  [offset(200.0)@700, offset(-200.0)@700, flat_exact@700]
short7-8x2-0     2.56e-07 / 2.85e-07   (fp16: 2.20e-06 / 9.36e-06)  [needle(0)@700, needle(31)@700, needle(32)@700]
short7-8x2-1     2.53e-07 / 2.76e-07   (fp16: 0.00e+00 / 0.00e+00)  [needle(63)@700, needle(64)@700, needle(111)@700]
short7-8x2-2     2.85e-07 / 2.96e-07   (fp16: 8.93e-08 / 4.21e-07)  [needle(112)@700, needle(223)@700, needle(last)@700]
short7-8x2-3     2.82e-06 / 2.72e-06   (fp16: 1.50e-05 / 7.41e-05)  [needle(current)@700, sink_recency@700, climb(60.0)@700]
short7-8x2-4     2.01e-06 / 1.98e-06   (fp16: 2.67e-05 / 1.14e-04)  [descend(60.0)@700, current(40.0)@700, current(-40.0)@700]
short7-8x2-5     1.67e-05 / 1.73e-05   (fp16: 1.22e-04 / 4.87e-04)  [offset(200.0)@700, offset(-200.0)@700, flat_exact@700]
pipe2-8x2-0      3.08e-07 / 3.33e-07   (fp16: 5.54e-05 / 1.98e-04)  [needle(0)@1400, needle(31)@1400, needle(32)@1400]
pipe2-8x2-1      2.36e-07 / 2.50e-07   (fp16: 1.99e-07 / 9.26e-07)  [needle(63)@1400, needle(64)@1400, needle(703)@1400]
pipe2-8x2-2      4.29e-07 / 4.57e-07   (fp16: 5.10e-07 / 2.08e-06)  [needle(704)@1400, needle(last)@1400, needle(current)@1400]
pipe2-8x2-3      3.42e-06 / 3.67e-06   (fp16: 1.77e-05 / 6.90e-05)  [sink_recency@1400, climb(60.0)@1400, descend(60.0)@1400]
pipe2-8x2-4      5.48e-06 / 5.81e-06   (fp16: 1.15e-04 / 3.71e-04)  [current(40.0)@1400, current(-40.0)@1400, offset(200.0)@1400]
pipe2-8x2-5      5.21e-06 / 6.76e-06   (fp16: 6.93e-05 / 3.31e-04)  [offset(-200.0)@1400, flat_exact@1400]
window2-8x2-0    2.22e-07 / 2.45e-07   (fp16: 5.41e-06 / 2.43e-05)  [needle(0)@1200, needle(15)@1200, needle(16)@1200]
window2-8x2-1    2.27e-07 / 2.59e-07   (fp16: 4.56e-05 / 5.15e-04)  [needle(31)@1200, needle(32)@1200, needle(607)@1200]
window2-8x2-2    4.94e-07 / 4.90e-07   (fp16: 4.96e-05 / 4.94e-04)  [needle(608)@1200, needle(last)@1200, needle(current)@1200]
window2-8x2-3    1.85e-06 / 2.28e-06   (fp16: 3.07e-06 / 1.24e-05)  [sink_recency@1200, climb(60.0)@1200, descend(60.0)@1200]
window2-8x2-4    1.12e-05 / 1.05e-05   (fp16: 4.42e-05 / 1.36e-04)  [current(40.0)@1200, current(-40.0)@1200, offset(200.0)@1200]
window2-8x2-5    8.49e-06 / 8.57e-06   (fp16: 7.87e-05 / 2.16e-04)  [offset(-200.0)@1200, flat_exact@1200]
tile95-8x2-0     2.39e-07 / 2.69e-07   (fp16: 0.00e+00 / 0.00e+00)  [needle(0)@95, needle(31)@95, needle(32)@95]
tile95-8x2-1     2.24e-07 / 2.52e-07   (fp16: 3.22e-05 / 1.15e-04)  [needle(63)@95, needle(64)@95, needle(last)@95]
tile95-8x2-2     1.28e-06 / 1.39e-06   (fp16: 1.93e-05 / 8.23e-05)  [needle(current)@95, sink_recency@95, climb(60.0)@95]
tile95-8x2-3     2.61e-06 / 2.42e-06   (fp16: 4.35e-05 / 1.80e-04)  [descend(60.0)@95, current(40.0)@95, current(-40.0)@95]
tile95-8x2-4     1.61e-05 / 1.71e-05   (fp16: 1.36e-04 / 4.80e-04)  [offset(200.0)@95, offset(-200.0)@95, flat_exact@95]
tile33-8x2-0     1.51e-07 / 1.65e-07   (fp16: 6.54e-07 / 2.65e-06)  [needle(0)@33, needle(31)@33, needle(last)@33]
tile33-8x2-1     5.47e-07 / 6.28e-07   (fp16: 1.60e-06 / 4.64e-06)  [needle(current)@33, sink_recency@33, climb(60.0)@33]
tile33-8x2-2     1.29e-06 / 1.15e-06   (fp16: 1.12e-04 / 5.09e-04)  [descend(60.0)@33, current(40.0)@33, current(-40.0)@33]
tile33-8x2-3     1.07e-05 / 1.08e-05   (fp16: 1.20e-04 / 5.09e-04)  [offset(200.0)@33, offset(-200.0)@33, flat_exact@33]
short7-16x2-0    2.37e-06 / 2.36e-06   (fp16: 4.32e-05 / 4.88e-04)  [needle(111)@700, needle(112)@700, climb(60.0)@700]
short7-16x2-1    1.16e-05 / 1.42e-05   (fp16: 1.67e-04 / 5.34e-04)  [descend(60.0)@700, offset(200.0)@700, offset(-200.0)@700]
pipe2-16x2-0     2.28e-06 / 2.09e-06   (fp16: 3.80e-05 / 1.84e-04)  [needle(703)@1400, needle(704)@1400, climb(60.0)@1400]
pipe2-16x2-1     9.79e-06 / 1.37e-05   (fp16: 1.07e-04 / 3.98e-04)  [descend(60.0)@1400, offset(200.0)@1400, offset(-200.0)@1400]
short7-7x1-0     1.54e-06 / 1.31e-06   (fp16: 8.69e-07 / 3.22e-06)  [needle(111)@700, needle(112)@700, climb(60.0)@700]
short7-7x1-1     1.26e-05 / 1.59e-05   (fp16: 5.95e-05 / 2.50e-04)  [descend(60.0)@700, offset(200.0)@700, offset(-200.0)@700]
pipe2-7x1-0      1.19e-06 / 1.07e-06   (fp16: 1.10e-06 / 4.35e-06)  [needle(703)@1400, needle(704)@1400, climb(60.0)@1400]
pipe2-7x1-1      7.21e-06 / 5.91e-06   (fp16: 1.07e-04 / 3.56e-04)  [descend(60.0)@1400, offset(200.0)@1400, offset(-200.0)@1400]
short7-2x2-0     2.46e-07 / 2.75e-07   (fp16: 0.00e+00 / 0.00e+00)  [needle(111)@700, needle(112)@700, climb(60.0)@700]
short7-2x2-1     3.51e-06 / 4.35e-06   (fp16: 5.71e-05 / 2.20e-04)  [descend(60.0)@700, offset(200.0)@700, offset(-200.0)@700]
pipe2-2x2-0      1.73e-07 / 1.54e-07   (fp16: 0.00e+00 / 0.00e+00)  [needle(703)@1400, needle(704)@1400, climb(60.0)@1400]
pipe2-2x2-1      2.54e-06 / 2.48e-06   (fp16: 3.01e-05 / 1.19e-04)  [descend(60.0)@1400, offset(200.0)@1400, offset(-200.0)@1400]
short7-4x2-0     2.84e-07 / 3.12e-07   (fp16: 3.45e-08 / 1.38e-07)  [needle(111)@700, needle(112)@700, climb(60.0)@700]
short7-4x2-1     3.85e-06 / 3.72e-06   (fp16: 3.50e-06 / 9.90e-06)  [descend(60.0)@700, offset(200.0)@700, offset(-200.0)@700]
pipe2-4x2-0      1.87e-07 / 2.16e-07   (fp16: 3.34e-07 / 1.36e-06)  [needle(703)@1400, needle(704)@1400, climb(60.0)@1400]
pipe2-4x2-1      3.59e-06 / 3.49e-06   (fp16: 1.06e-04 / 4.39e-04)  [descend(60.0)@1400, offset(200.0)@1400, offset(-200.0)@1400]
mixed-8x2-0      2.35e-06 / 2.63e-06   (fp16: 1.96e-05 / 8.44e-05)  [needle(703)@1400, sink_recency@5, climb(60.0)@1400]
mixed-8x2-1      6.10e-06 / 7.26e-06   (fp16: 8.14e-05 / 4.88e-04)  [needle(0)@5, descend(60.0)@1400, offset(200.0)@5]
merge2-8x2-0     3.80e-06 / 3.40e-06   (fp16: 5.54e-05 / 5.35e-04)  [climb(60.0)@1400, descend(60.0)@1400, needle(703)@1400]
merge2-8x2-1     8.44e-06 / 6.51e-06   (fp16: 8.22e-05 / 2.18e-04)  [needle(704)@1400, offset(200.0)@1400, offset(-200.0)@1400]
merge7-8x2-0     2.57e-06 / 2.69e-06   (fp16: 5.36e-05 / 2.55e-04)  [climb(60.0)@700, descend(60.0)@700, needle(111)@700]
merge7-8x2-1     1.09e-05 / 8.67e-06   (fp16: 8.73e-05 / 3.18e-04)  [needle(112)@700, offset(200.0)@700, offset(-200.0)@700]
"""
