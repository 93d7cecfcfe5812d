"""Sampled decoding: the f64 oracle of fused_ext.sample's contract, the case table of the GPU tests, the
fairness predicates that make those cases decidable by the oracle alone, and the reference's rule (the HF warpers of
omniserve/modeling/layers/sampler.py) restated in numpy.  Pure numpy: importable without a GPU."""
import itertools
from dataclasses import dataclass

import numpy as np

DELTA = 2e-5            # slack on the normalised CDF (the issue's error budget: ~4e-6, so a 5x margin)
FAIR_MARGIN = 1e-4      # no key boundary's cumulative mass may lie this close to top_p

KEY_POS_INF, KEY_NEG_INF = 0xFC00, 0x03FF


def keys_of(x16):
    """The orderable 16-bit key of the arg-max kernel: -0 == +0, positive NaN above +inf, negative NaN below -inf."""
    h = np.ascontiguousarray(x16, dtype=np.float16).view(np.uint16).astype(np.int64)
    h = np.where(h == 0x8000, 0, h)
    return np.where(h & 0x8000, ~h & 0xFFFF, h | 0x8000)


def argmax_ref(x16):
    """fused_ext.argmax's answer: the first maximum by key."""
    return int(np.argmax(keys_of(x16)))


def is_greedy(x16, temperature, top_k, top_p):
    mk = int(keys_of(x16).max())
    return bool(np.float32(temperature) < np.float32(1e-5) or np.float32(top_p) < np.float32(1e-8) or int(top_k) == 1 or
                mk >= KEY_POS_INF or mk <= KEY_NEG_INF)


@dataclass
class RowOracle:
    greedy: bool
    argmax: int
    kept: np.ndarray = None        # bool [cols]: x >= max(t_p, t_k), -inf never
    prob: np.ndarray = None        # f64 [cols]: w / Z_kept on the kept set, 0 elsewhere (no exclusion)
    order: np.ndarray = None       # the kept tokens less `exclude` in canonical order (value descending, index ascending)
    cdf_lo: np.ndarray = None      # f64, aligned with `order`: the tokens' intervals of the normalised cumulative weight
    cdf_hi: np.ndarray = None
    boundaries: np.ndarray = None  # cumulative mass / Z at every key boundary (fairness)
    kth_key: int = None            # the key of the k-th largest value when top-k is on and k <= cols

    def interval(self, token):
        pos = np.nonzero(self.order == token)[0]
        return (float(self.cdf_lo[pos[0]]), float(self.cdf_hi[pos[0]])) if len(pos) else None


def oracle_row(x16, temperature, top_k, top_p, exclude=-1):
    """The contract in f64 for one row (x16: float16 [cols])."""
    x16 = np.ascontiguousarray(x16, dtype=np.float16)
    cols = x16.shape[0]
    keys = keys_of(x16)
    amax = int(np.argmax(keys))
    if is_greedy(x16, temperature, top_k, top_p):
        return RowOracle(True, amax)
    T, p, k = float(np.float32(temperature)), float(np.float32(top_p)), int(top_k)
    xv = x16.astype(np.float64)
    finite = keys > KEY_NEG_INF
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(finite, np.exp((xv - xv[amax]) / T), 0.0)
    Z = float(w.sum())
    # per distinct key, descending
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    uk, cnt = uk[::-1], cnt[::-1]
    mass = np.bincount(inv, weights=w, minlength=len(uk))[::-1]
    m_incl, c_incl = np.cumsum(mass), np.cumsum(cnt)
    m_above = m_incl - mass
    thr = 0
    if p < 1.0:        # kept iff the mass strictly above the value is < p * Z; the set always holds the maximum
        thr = max(thr, int(uk[np.nonzero(m_above < p * Z)[0].max()]))
    kth = None
    if 0 < k <= cols:  # kept iff the value is >= the k-th largest
        kk = int(uk[np.nonzero(c_incl >= k)[0].min()])
        thr = max(thr, kk)
        kth = kk
    kept = (keys >= thr) & finite
    zk = float(w[kept].sum())
    prob = np.where(kept, w / zk, 0.0)
    draw = kept.copy()
    if 0 <= exclude < cols:
        draw[exclude] = False
    idx = np.nonzero(draw)[0]
    order = idx[np.lexsort((idx, -keys[idx]))]
    wz = w[order]
    tot = float(wz.sum())
    hi = np.cumsum(wz) / tot if tot > 0 else np.zeros(0)
    lo = hi - wz / tot if tot > 0 else np.zeros(0)
    return RowOracle(False, amax, kept, prob, order if tot > 0 else order[:0], lo, hi, m_incl / Z, kth)


def row_is_fair(x16, temperature, top_k, top_p):
    """The oracle decides the row's kept set without a tolerance: no key boundary's cumulative mass within FAIR_MARGIN of top_p
    (the boundary at the whole row excepted when it IS the row: mass 1 > top_p + margin needs top_p < 1 - margin, which every
    case parameter satisfies), and the k-th largest value is found exactly (integer counts over the keys)."""
    o = oracle_row(x16, temperature, top_k, top_p)
    if o.greedy:
        return True
    p = float(np.float32(top_p))
    if p < 1.0 and np.any(np.abs(o.boundaries - p) <= FAIR_MARGIN):
        return False
    if o.kth_key is not None:       # against a plain descending sort of the values
        kth = np.sort(np.ascontiguousarray(x16, dtype=np.float16).astype(np.float64))[::-1][int(top_k) - 1]
        if int(keys_of(np.float16(kth).reshape(1))[0]) != o.kth_key:
            return False
    return True


def hf_kept(x16, temperature, top_k, top_p):
    """The reference's rule: TemperatureLogitsWarper, then TopPLogitsWarper, then TopKLogitsWarper (min_tokens_to_keep = 1) as
    prepare_logits_processor chains them, restated in numpy f64 with a STABLE ascending sort.  -> bool [cols] kept."""
    s = np.ascontiguousarray(x16, dtype=np.float16).astype(np.float64) / float(np.float32(temperature))
    p, k = float(np.float32(top_p)), int(top_k)
    if 1e-8 <= p < 1.0:
        srt = np.argsort(s, kind="stable")
        e = np.exp(s[srt] - s[srt].max())
        cum = np.cumsum(e / e.sum())
        remove = cum <= 1.0 - p
        remove[-1:] = False
        s = s.copy()
        s[srt[remove]] = -np.inf
    if k > 0:
        kk = min(k, s.shape[0])
        s = np.where(s < np.sort(s)[-kk], -np.inf, s)
    return s > -np.inf


# ---- profiles ---------------------------------------------------------------------------------------------------------
def _normal(scale):
    def f(cols, rng):
        return (rng.standard_normal(cols) * scale).astype(np.float16)
    return f


def _one_hot(cols, rng):
    x = rng.standard_normal(cols) * 0.5
    x[int(rng.integers(cols))] += 12.0
    return x.astype(np.float16)


def _two_valued(cols, rng):
    x = np.where(rng.random(cols) < 0.3, 1.5, -0.75)
    x[int(rng.integers(cols))] = 1.5
    return x.astype(np.float16)


def _constant(cols, rng):
    return np.full(cols, 0.375, dtype=np.float16)


def _half_neg_inf(cols, rng):
    x = rng.standard_normal(cols) * 2.0
    x[rng.permutation(cols)[: cols // 2]] = -np.inf
    return x.astype(np.float16)


def _zero_straddle(cols, rng):
    vals = np.array([-0.5, -0.0, 0.0, 0.25, -6e-5, 6e-5, -2.0], dtype=np.float16)
    x = vals[rng.integers(len(vals), size=cols)]
    if cols >= 2:
        a, b = rng.permutation(cols)[:2]
        x[a], x[b] = np.float16(0.0), np.float16(-0.0)
    return x


def tie_at_top_k(cols, rng, ties=1000, above=20):
    """`above` distinct values on top, then a `ties`-way tie, the rest below: a top_k inside (above, above + ties] cuts in the tie."""
    ties, above = min(ties, max(1, cols // 2)), min(above, max(0, cols // 4))
    x = -3.0 - np.abs(rng.standard_normal(cols))
    perm = rng.permutation(cols)
    x[perm[:above]] = 2.0 + 0.125 * np.arange(above)
    x[perm[above:above + ties]] = 1.0
    return x.astype(np.float16)


def split_bins(cols, rng):
    """Three tokens near 8 (key high byte 0xC8) and a bulk of four values 0.5 .. 0.875, one per high byte 0xB8 .. 0xBB: a small
    top_k cuts in the first bin while top_p crosses in one of the bulk's at T = 2.5, and the other way round with top_k = cols / 2
    and a small top_p.  (Four bulk values, not a continuum: the cumulative mass then has six boundaries, none near top_p.)"""
    x = 0.5 + 0.125 * rng.integers(4, size=cols)
    x[rng.permutation(cols)[: min(3, cols)]] = 8.0 + 0.25 * np.arange(min(3, cols))
    return x.astype(np.float16)


PROFILES = {"normal_x1": _normal(1.0), "normal_x8": _normal(8.0), "one_hot": _one_hot, "two_valued": _two_valued,
            "constant": _constant, "half_neg_inf": _half_neg_inf, "zero_straddle": _zero_straddle,
            "tie_at_top_k": tie_at_top_k, "split_bins": split_bins}
PROFILE_NAMES = list(PROFILES)

TEMPERATURES = (0.3, 1.0, 2.5)
TOP_KS = ("0", "1", "2", "50", "cols", "cols+5")
TOP_PS = (1.0, 0.9, 0.5, 1e-9)
COMBOS = list(itertools.product(TEMPERATURES, TOP_KS, TOP_PS))      # 72


def _k_of(name, cols):
    return {"cols": cols, "cols+5": cols + 5}[name] if name in ("cols", "cols+5") else int(name)


COLS = (1, 7, 255, 256, 257, 4099, 32000)
ROWS = (1, 3, 17)
LAYOUTS = ("dense", "strided", "misaligned")      # row stride == cols; > cols; a view whose base is only 2-byte aligned


@dataclass
class Case:
    name: str
    cols: int
    rows: int
    layout: str
    logits: np.ndarray          # float16 [rows, cols]
    temperature: np.ndarray     # f32 [rows]
    top_k: np.ndarray           # i32 [rows]
    top_p: np.ndarray           # f32 [rows]
    u: np.ndarray               # f32 [rows]
    probe: np.ndarray           # i64 [rows]
    exclude: np.ndarray         # i64 [rows]
    profiles: list


def _finish(name, cols, rows, layout, logits, params, profiles, rng):
    t = np.array([q[0] for q in params], dtype=np.float32)
    k = np.array([q[1] for q in params], dtype=np.int32)
    p = np.array([q[2] for q in params], dtype=np.float32)
    u = rng.random(rows).astype(np.float32)
    u[u >= 1.0] = 0.5
    probe = np.empty(rows, dtype=np.int64)
    exclude = np.empty(rows, dtype=np.int64)
    for r in range(rows):       # none / the maximum / a random token, in turn and out of step with each other
        top = argmax_ref(logits[r])
        probe[r] = (-1, top, int(rng.integers(cols)))[(r + 1) % 3]
        exclude[r] = (top, int(rng.integers(cols)), -1, top)[r % 4]
    return Case(name, cols, rows, layout, logits, t, k, p, u, probe, exclude, profiles)


def _fair_top_p(x16, T, k, p):
    """A flat row of many tokens has key boundaries closer together than 2 * FAIR_MARGIN, so no top_p inside it is fair: such a
    row takes the next value of the parameter set that is (1.0, top-p off, always is)."""
    for q in (p,) + tuple(q for q in (0.5, 0.9, 1.0) if q != p):
        if row_is_fair(x16, T, k, q):
            return q
    raise AssertionError("no fair top_p")


def _build_cases():
    cases = []
    n = 0
    for cols in COLS:
        for rows in ROWS:
            for layout in LAYOUTS:
                rng = np.random.default_rng(1000 + n)
                profiles = [PROFILE_NAMES[(n + r) % len(PROFILE_NAMES)] for r in range(rows)]
                logits = np.stack([PROFILES[pr](cols, rng) for pr in profiles])
                params = []
                for r in range(rows):
                    T, kn, p = COMBOS[(7 * n + 5 * r) % len(COMBOS)]
                    params.append((T, _k_of(kn, cols), _fair_top_p(logits[r], T, _k_of(kn, cols), p)))
                cases.append(_finish("c%d_r%d_%s" % (cols, rows, layout), cols, rows, layout, logits, params, profiles, rng))
                n += 1
    # the full vocabulary once
    rng = np.random.default_rng(77)
    profiles = ["normal_x8", "normal_x1", "half_neg_inf"]
    logits = np.stack([PROFILES[pr](128256, rng) for pr in profiles])
    cases.append(_finish("c128256_r3_dense", 128256, 3, "dense", logits,
                         [(1.0, 50, 0.9), (2.5, 2000, 1.0), (0.3, 128256 + 5, 0.5)], profiles, rng))
    # a 1000-way tie at the top-k threshold (k inside the tie, at its first and last member, and with top-p beside it), and
    # rows whose top-p crossing and top-k crossing fall in different high-byte bins, both ways round
    rng = np.random.default_rng(78)
    profiles = ["tie_at_top_k"] * 4 + ["split_bins"] * 4
    logits = np.stack([PROFILES[pr](4099, rng) for pr in profiles])
    params = [(1.0, 500, 1.0), (1.0, 21, 1.0), (1.0, 1020, 1.0), (2.5, 500, 0.5),
              (2.5, 2, 0.9), (2.5, 2000, 0.01), (1.0, 3, 0.5), (2.5, 0, 0.9)]
    cases.append(_finish("special_c4099_r8", 4099, 8, "dense", logits, params, profiles, rng))
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
        _ORACLES[case.name] = [oracle_row(case.logits[r], case.temperature[r], case.top_k[r], case.top_p[r], int(case.exclude[r]))
                               for r in range(case.rows)]
    return _ORACLES[case.name]


def outside_interval(oracle, token, u):
    """How far u lies outside the token's interval [cdf_lo, cdf_hi) (0 inside); None if the token is not in the draw set."""
    iv = oracle.interval(token)
    if iv is None:
        return None
    lo, hi = iv
    return max(lo - float(u), float(u) - hi, 0.0) if not (lo <= float(u) < hi) else 0.0
