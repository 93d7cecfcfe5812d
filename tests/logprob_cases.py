"""Log-probabilities: the f64 oracle of fused_ext.logprobs' contract, the case grid of the GPU tests and
the error bound they share.  Pure numpy: importable without a GPU."""
from dataclasses import dataclass

import numpy as np

from sampling_cases import KEY_NEG_INF, KEY_POS_INF, keys_of

DELTA = 2e-5             # DESIGN 4.6's slack for the same exp / sum chain (budget about 4e-6)
REL = 2.0 ** -22         # the f32 rounding of x - lse (and of max + ln sum) at large magnitudes

MAX_TOP = 20
CHUNKS, VEC = 32, 8      # fused_ext.LOGPROB_CHUNKS / LOGPROB_VEC (test_logprob_cpu asserts that they agree)


def chunk_cols(cols):
    """fused_ext.logprob_chunk_cols: columns per chunk, a function of cols only."""
    return ((cols + CHUNKS - 1) // CHUNKS + VEC - 1) // VEC * VEC


def order_of(x16):
    """The canonical order of a row: value descending by the 16-bit key (-0 == +0), then index ascending."""
    keys = keys_of(x16)
    idx = np.arange(len(keys))
    return idx[np.lexsort((idx, -keys))]


def is_degenerate(x16):
    mk = int(keys_of(x16).max())
    return mk >= KEY_POS_INF or mk <= KEY_NEG_INF


@dataclass
class RowOracle:
    lse: float                 # f64; NaN for a degenerate row
    logprob: np.ndarray        # f64 [cols]: x - lse (-inf for -inf; NaN everywhere for a degenerate row)
    order: np.ndarray          # int64 [cols]: the canonical order
    rank: np.ndarray           # int64 [cols]: 1-based position of every token in it

    def top(self, n):
        """(tokens int64 [n], logprobs f64 [n]): the first n of the order, -1 / -inf behind the last column."""
        cols = len(self.order)
        tok = np.full(n, -1, dtype=np.int64)
        lp = np.full(n, -np.inf, dtype=np.float64)
        m = min(n, cols)
        tok[:m] = self.order[:m]
        lp[:m] = self.logprob[self.order[:m]]
        return tok, lp

    def target(self, t):
        """(logprob, rank) of token t: NaN / 0 outside [0, cols)."""
        if not 0 <= t < len(self.order):
            return np.nan, 0
        return float(self.logprob[t]), int(self.rank[t])


def oracle_row(x16):
    """The contract in f64 for one row (x16: float16 [cols])."""
    x16 = np.ascontiguousarray(x16, dtype=np.float16)
    cols = x16.shape[0]
    order = order_of(x16)
    rank = np.empty(cols, dtype=np.int64)
    rank[order] = np.arange(1, cols + 1)
    if is_degenerate(x16):      # the maximum is NaN or +inf, or nothing but -inf
        return RowOracle(np.nan, np.full(cols, np.nan), order, rank)
    xv = x16.astype(np.float64)
    finite = keys_of(x16) > KEY_NEG_INF
    vmax = xv[order[0]]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(finite, np.exp(xv - vmax), 0.0)
        lse = vmax + np.log(w.sum())
        logprob = xv - lse      # (-inf stays -inf; a negative NaN below a finite maximum stays NaN)
    return RowOracle(float(lse), logprob, order, rank)


def bound(ref):
    """|err| allowed against the f64 reference value(s): DELTA + 2^-22 |ref| (non-finite references must match exactly)."""
    return DELTA + REL * np.abs(ref)


def value_errors(got, ref):
    """got f32 / ref f64 arrays -> (exact: the non-finite entries of ref are matched in kind, worst |err| / bound over the finite
    ones, worst |err|)."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    fin = np.isfinite(ref)
    exact = bool(np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
                 and np.isfinite(got[fin]).all())
    if not fin.any() or not exact:
        return exact, 0.0, 0.0
    err = np.abs(got[fin] - ref[fin])
    return exact, float((err / bound(ref[fin])).max()), float(err.max())


# ---- profiles: f(cols, rng, n_top, edges) -> float16 [cols] ------------------------------------------------------------------
def _gaussian(cols, rng, n_top, edges):
    return (rng.standard_normal(cols) * 3.0).astype(np.float16)


def _peaked(cols, rng, n_top, edges):
    x = rng.standard_normal(cols)
    x[int(rng.integers(cols))] += 30.0
    return x.astype(np.float16)


def _all_equal(cols, rng, n_top, edges):
    return np.full(cols, -1.25, dtype=np.float16)


def _two_valued(cols, rng, n_top, edges):
    """Two values, n_hi tokens of the upper one: with n_top >= 2 the top list ends inside the run of the lower value (n_hi <
    n_top), with n_top <= 1 inside the run of the upper one (n_hi = 2) -- either way the boundary lies INSIDE a tie run, where a
    row is long enough to have one."""
    x = np.full(cols, -0.5, dtype=np.float16)
    n_hi = n_top // 2 + 1 if n_top > 1 else 2
    x[rng.permutation(cols)[: min(cols, n_hi)]] = np.float16(2.0)
    return x


def _tie_across_edge(cols, rng, n_top, edges):
    """The maximum repeated on both sides of every chunk edge (and at both ends of the row): ties across chunks resolve by index."""
    x = (rng.standard_normal(cols) * 0.5).astype(np.float16)
    for e in [0, cols - 1] + [c for edge in edges for c in (edge - 1, edge)]:
        if 0 <= e < cols:
            x[e] = np.float16(4.0)
    return x


def _signed_zeros(cols, rng, n_top, edges):
    x = np.where(rng.random(cols) < 0.5, 0.0, -0.0).astype(np.float16)
    if cols >= 3:
        x[rng.permutation(cols)[: cols // 3]] = np.float16(-1.0)
    if cols >= 2:
        x[0], x[1] = np.float16(-0.0), np.float16(0.0)      # -0 first: it ties with +0 and wins on the index
    return x


def _extremes(cols, rng, n_top, edges):
    x = np.where(rng.random(cols) < 0.5, 65504.0, -65504.0).astype(np.float16)
    x[int(rng.integers(cols))] = np.float16(65504.0)
    return x


def _mostly_neg_inf(cols, rng, n_top, edges):
    """More -inf than cols - n_top: a top list of n_top (where cols allows) reaches -inf entries."""
    x = np.full(cols, -np.inf, dtype=np.float16)
    keep = max(1, min(cols, n_top) // 2)
    x[rng.permutation(cols)[:keep]] = (rng.standard_normal(keep) * 2.0).astype(np.float16)
    return x


def _all_neg_inf(cols, rng, n_top, edges):
    return np.full(cols, -np.inf, dtype=np.float16)


def _with_nan(cols, rng, n_top, edges):
    x = (rng.standard_normal(cols) * 2.0).astype(np.float16)
    x[int(rng.integers(cols))] = np.float16(np.nan)
    return x


def _with_pos_inf(cols, rng, n_top, edges):
    x = (rng.standard_normal(cols) * 2.0).astype(np.float16)
    x[int(rng.integers(cols))] = np.float16(np.inf)
    return x


PROFILES = {"gaussian": _gaussian, "peaked": _peaked, "all_equal": _all_equal, "two_valued": _two_valued,
            "tie_across_edge": _tie_across_edge, "signed_zeros": _signed_zeros, "extremes": _extremes,
            "mostly_neg_inf": _mostly_neg_inf, "all_neg_inf": _all_neg_inf, "nan": _with_nan, "pos_inf": _with_pos_inf}
PROFILE_NAMES = list(PROFILES)

# one below / at / one above: a chunk per column (32 columns), the vector load (8 per chunk: 256 -- in the list already --, and
# 8 columns as such), the first cols whose chunk is 16 columns (257 .. : chunk_cols jumps from 8 to 16 behind 256), and a
# workgroup's stride of 8 * 256 columns per chunk (32 * 2048 = 65536)
SMALL_COLS = (1, 2, 7, 8, 9, 31, 32, 33, 255, 256, 257)
STRIDE_COLS = (65535, 65536, 65537)
BIG_COLS = 128256
ROWS = (1, 3, 16)
LAYOUTS = ("dense", "strided", "misaligned")      # the sampler cases': row stride == cols; > cols and odd; a 2-byte aligned base
N_TOPS = (0, 1, 5, 20)
TARGET_CLASSES = ("first", "last", "edge_lo", "edge_hi", "minus_one", "cols", "argmax", "random")


def chunk_edges(cols):
    per = chunk_cols(cols)
    return [e for e in range(per, cols, per)]


@dataclass
class Case:
    name: str
    cols: int
    rows: int
    layout: str
    n_top: int
    logits: np.ndarray          # float16 [rows, cols]
    target: np.ndarray          # int64 [rows]
    profiles: list
    target_classes: list


def _target(cls, cols, edges, x16, rng):
    edge = edges[int(rng.integers(len(edges)))] if edges else 0
    return {"first": 0, "last": cols - 1, "edge_lo": max(edge - 1, 0), "edge_hi": min(edge, cols - 1), "minus_one": -1, "cols": cols,
            "argmax": int(np.argmax(keys_of(x16))), "random": int(rng.integers(cols))}[cls]


def _case(n, cols, rows, layout, n_top):
    rng = np.random.default_rng(4000 + n)
    edges = chunk_edges(cols)
    profiles = [PROFILE_NAMES[(n + r) % len(PROFILE_NAMES)] for r in range(rows)]
    logits = np.stack([PROFILES[p](cols, rng, n_top, edges) for p in profiles])
    classes = [TARGET_CLASSES[(3 * n + r) % len(TARGET_CLASSES)] for r in range(rows)]
    target = np.array([_target(classes[r], cols, edges, logits[r], rng) for r in range(rows)], dtype=np.int64)
    return Case("c%d_r%d_%s_top%d" % (cols, rows, layout, n_top), cols, rows, layout, n_top, logits, target, profiles, classes)


def _build_cases():
    cases = []
    n = 0
    for cols in SMALL_COLS:
        for rows in ROWS:
            for layout in LAYOUTS:
                cases.append(_case(n, cols, rows, layout, N_TOPS[n % len(N_TOPS)]))
                n += 1
    for cols in STRIDE_COLS:      # wide rows: one shape each, the layouts and the top sizes in turn
        cases.append(_case(n, cols, 3, LAYOUTS[n % 3], N_TOPS[1 + n % 3]))
        n += 1
    cases.append(_case(n, BIG_COLS, 3, "dense", 20))      # the full vocabulary once
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


_ORACLES = {}


def case_oracles(case):
    """The rows' oracles, computed once per case and shared by the tests."""
    if case.name not in _ORACLES:
        _ORACLES[case.name] = [oracle_row(case.logits[r]) for r in range(case.rows)]
    return _ORACLES[case.name]
