"""Inputs of the prefill-attention edge cases, shared by the CPU oracle tests (tests/test_oracle_kat_cpu.py) and the GPU tests
(tests/test_prefill_attn_edges_gpu.py): unequal q / k lengths (bottom-right aligned mask), non-causal, per-head windows and
classes, windows that mean "everything", inputs that stress the online softmax, launch geometry.  numpy only.

A case is a dict: name, pairs [(len_q, len_k), ...], Hq, Hk, causal, hm / si (int32 tables or None), block (1 token form, 128
block form), seed, and for the softmax family qscale / ramp.  `inputs` builds q, k, v, cu_q, cu_k from it; `reference` is the f64
oracle of the case, computed once per process and handed out read-only."""
import functools

import numpy as np

from oracle import attention as oa

D = 128
I32_MAX = 2 ** 31 - 1

# (len_q, len_k) of one sequence, family a
UNEQUAL_PAIRS = [(1, 200), (40, 200), (129, 257), (64, 64), (50, 20), (5, 0)]
# lengths on and next to the 64-key tile and the 128-row query tile, each with a key side that puts the diagonal at an offset
STRADDLE_PAIRS = [(63, 64), (64, 127), (65, 129), (127, 128), (128, 200), (129, 129)]


def _tables(classes, windows):
    hm = np.asarray(classes, np.int32)
    si = np.asarray([x for w in windows for x in w], np.int64)
    assert si.min() >= 0 and si.max() <= I32_MAX
    return hm, si.astype(np.int32)


def _case(name, pairs, Hq, Hk, causal=True, classes=None, windows=None, block=1, seed=0, qscale=1.0, ramp=None):
    hm = si = None
    if classes is not None:
        hm, si = _tables(classes, windows)
        assert len(hm) == Hq and len(si) == 2 * Hq
    return dict(name=name, pairs=[tuple(p) for p in pairs], Hq=Hq, Hk=Hk, causal=causal, hm=hm, si=si, block=block, seed=seed,
                qscale=qscale, ramp=ramp)


def _modes(name, pairs, seed, causal=True):
    """One batch as dense heads, token-streaming heads and block-streaming heads (kv heads dense / streaming, Hq = 4, Hk = 2).
    Token window (4, 33): shorter than a key tile.  Block window (1, 1): the sink block and the query's own block, so with
    len_k = 257 the key block 1 is masked for the queries of block 2."""
    return [_case(name + "-dense", pairs, 4, 2, causal, seed=seed),
            _case(name + "-token", pairs, 4, 2, causal, [0, 0, -1, -1], [(0, 0), (0, 0), (4, 33), (4, 33)], 1, seed + 1),
            _case(name + "-block", pairs, 4, 2, causal, [-1, -1, 0, 0], [(1, 1), (1, 1), (0, 0), (0, 0)], 128, seed + 2)]


def family_a():
    out = []
    for n, p in enumerate(UNEQUAL_PAIRS):
        out += _modes("a-q%d-k%d" % p, [p], 100 + 10 * n)
    out += _modes("a-mixed", UNEQUAL_PAIRS, 170)
    out += _modes("a-straddle", STRADDLE_PAIRS, 180)
    return out


def family_b():
    eq = [(n, n) for n in (200, 65, 1, 128, 63)]
    return [_case("b-equal", eq, 4, 2, False, seed=200),
            _case("b-q130-k70", [(130, 70)], 4, 2, False, seed=201),
            _case("b-q70-k130", [(70, 130)], 4, 2, False, seed=202),
            _case("b-mixed", [(130, 70), (70, 130), (1, 200), (5, 0), (64, 129), (129, 64)], 4, 2, False, seed=203)]


# family c: Hq = 8, Hk = 4, a class from {0, -1, -2} and a window of its own per q head.  kv head 1 has one dense and one
# streaming q head; the dense heads carry (0, 0), which would blank them if a kernel applied it.
C_CLASSES = [-1, -2, 0, -1, -2, -2, 0, 0]
C_TOKEN = [(0, 1), (1, 2), (0, 0), (4, 33), (64, 64), (65, 127), (0, 0), (0, 0)]
C_TOKEN_2 = [(128, 256), (3, 5), (0, 0), (0, 20), (7, 200), (1, 1), (0, 0), (0, 0)]
C_BLOCK = [(0, 1), (1, 1), (0, 0), (1, 2), (2, 1), (0, 3), (0, 0), (0, 0)]
C_PAIRS = [(700, 700), (129, 129), (1, 1)]


def family_c():
    return [_case("c-token", C_PAIRS, 8, 4, True, C_CLASSES, C_TOKEN, 1, 300),
            _case("c-token2", C_PAIRS, 8, 4, True, C_CLASSES, C_TOKEN_2, 1, 301),
            _case("c-block", C_PAIRS, 8, 4, True, C_CLASSES, C_BLOCK, 128, 302)]


# family d: every window below lets every causal key through, so the result is dense causal attention
D_TOKEN_VALUES = [1 << 24, 1 << 30, I32_MAX]
D_BLOCK_VALUES = [1 << 24, (1 << 24) + 3, 1 << 25, 1 << 30, I32_MAX]
D_PAIRS = [(300, 300), (129, 129)]


def family_d():
    out = []
    for block, values in ((1, D_TOKEN_VALUES), (128, D_BLOCK_VALUES)):
        for v in values:      # per q head: everything through the sink, through the window, through both, window beside a sink
            out.append(_case("d-%s-%d" % ("token" if block == 1 else "block", v), D_PAIRS, 4, 2, True, [-1] * 4,
                             [(v, 1), (0, v), (v, v), (1, v)], block, 400))       # one seed: one dense-causal answer
    return out


def family_d_noncausal():
    """Non-causal with token windows (the C entry takes both): len_q 50 against len_k 20 puts the first 30 queries at negative
    positions, where position - local + 1 leaves int32 for local = 2**31 - 1.  Equals dense non-causal attention."""
    return [_case("d-noncausal-token", [(50, 20), (70, 130)], 4, 2, False, [-1] * 4,
                  [(0, I32_MAX), (0, 1 << 30), (I32_MAX, I32_MAX), (1, I32_MAX)], 1, 410)]


def family_e():
    """Q scaled by 8 and keys with a norm ramp along a common direction: see `inputs`.  Dense heads and token-streaming heads
    with no sink and a window (20) shorter than a key tile: the first tile a query tile visits is then fully masked for its late
    rows."""
    cl, w = [0, 0, -1, -1], [(0, 0), (0, 0), (0, 20), (0, 20)]
    return [_case("e-flat", [(700, 700)], 4, 2, True, cl, w, 1, 500, qscale=8.0),
            _case("e-ascending", [(700, 700)], 4, 2, True, cl, w, 1, 501, qscale=8.0, ramp="ascending"),
            _case("e-descending", [(700, 700)], 4, 2, True, cl, w, 1, 502, qscale=8.0, ramp="descending")]


def family_f():
    z = [(0, 0), (65, 65), (0, 0), (0, 0), (130, 130), (0, 0)]
    return _modes("f-zero-lengths", z, 600) + _modes("f-70-130", [(70, 70), (130, 130)], 610)


def family_g():
    return _modes("g-130-65", [(130, 130), (65, 65)], 700) + _modes("g-65-1", [(65, 65), (1, 1)], 710)


def all_cases():
    return family_a() + family_b() + family_c() + family_d() + family_d_noncausal() + family_e() + family_f() + family_g()


RAMP_STEP = 15.0 / 64      # per key: 15 per 64-key tile


def inputs(case):
    """q [Lq, Hq, D], k, v [Lk, Hk, D] fp16, cu_q, cu_k int32.  Plain cases: i.i.d. N(0, 1).  Softmax family: with d a fixed
    unit vector, q = qscale * (n + 8 d) and k_j = n + r_j d with r_j = RAMP_STEP * j ascending (or the same ramp descending).
    q.d >= 8 * 4 for every row (checked), so a step of 64 keys moves the natural-log score by >= 15 * 32 / sqrt(128) = 42 while
    the noise term has a standard deviation of about 10: every tile's row maximum beats the previous tile's by more than 20
    (ascending), or the first tile holds it (descending).  tests/test_oracle_kat_cpu.py asserts that on the f64 scores."""
    rng = np.random.default_rng(case["seed"])
    Lq = sum(p[0] for p in case["pairs"]); Lk = sum(p[1] for p in case["pairs"])
    Hq, Hk = case["Hq"], case["Hk"]
    q = rng.standard_normal((Lq, Hq, D))
    k = rng.standard_normal((Lk, Hk, D))
    v = rng.standard_normal((Lk, Hk, D))
    if case["ramp"] is not None:
        d = np.where(np.arange(D) % 2 == 0, 1.0, -1.0) / np.sqrt(D)
        q = q + 8.0 * d
        r = RAMP_STEP * np.arange(Lk, dtype=np.float64)
        if case["ramp"] == "descending":
            r = r[::-1]
        k = k + r[:, None, None] * d
    q = q * case["qscale"]
    cu_q = np.concatenate([[0], np.cumsum([p[0] for p in case["pairs"]])]).astype(np.int32)
    cu_k = np.concatenate([[0], np.cumsum([p[1] for p in case["pairs"]])]).astype(np.int32)
    return q.astype(np.float16), k.astype(np.float16), v.astype(np.float16), cu_q, cu_k


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = {c["name"]: c for c in all_cases()}[name]
    q, k, v, cu_q, cu_k = inputs(case)
    ref = oa.varlen_attention(q, k, v, cu_q, cu_k, case["causal"], case["hm"], case["si"], block=case["block"])
    ref.flags.writeable = False
    return ref


def reference(case):
    """fp16 [Lq, Hq, D]: the f64 oracle of the case (cached, read-only)."""
    return _reference(case["name"])


def zero_rows(case):
    """bool [Lq, Hq]: (row, head) pairs that see no key at all, from the mask rule itself (not from the oracle's output)."""
    Lq = sum(p[0] for p in case["pairs"])
    out = np.zeros((Lq, case["Hq"]), bool)
    q0 = 0
    for lq, lk in case["pairs"]:
        qi = np.arange(lq)[:, None] + (lk - lq)
        ki = np.arange(lk)[None, :]
        for h in range(case["Hq"]):
            m = np.ones((lq, lk), bool)
            if case["causal"]:
                m &= ki <= qi
            if case["hm"] is not None and case["hm"][h] < 0:
                m &= oa.streaming_mask(qi, ki, int(case["si"][2 * h]), int(case["si"][2 * h + 1]), case["block"])
            out[q0:q0 + lq, h] = ~m.any(axis=1)
        q0 += lq
    return out
