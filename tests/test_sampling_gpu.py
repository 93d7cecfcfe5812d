"""fused_ext.sample on the MI355X against the f64 oracle of its contract (tests/sampling_cases.py)."""
import numpy as np
import pytest
import torch

import sampling_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _device_logits(case):
    x = torch.from_numpy(case.logits)
    if case.layout == "dense":
        return x.to(DEV)
    if case.layout == "strided":
        buf = torch.full((case.rows, case.cols + 24), float("nan"), dtype=torch.float16, device=DEV)
        buf[:, : case.cols] = x.to(DEV)
        return buf[:, : case.cols]
    flat = torch.empty((case.rows * case.cols + 1,), dtype=torch.float16, device=DEV)      # base pointer 2-byte aligned only
    view = flat[1:].view(case.rows, case.cols)
    view.copy_(x.to(DEV))
    assert view.data_ptr() % 4 == 2
    return view


def _sample(logits, t, k, p, u, probe=None, exclude=None, want_prob=True):
    from omniserve_amd.backend import fused_ext
    rows = logits.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a      # noqa: E731
    out = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    prob = torch.full((rows,), -7.0, dtype=torch.float32, device=DEV) if want_prob and probe is not None else None
    fused_ext.sample(out, logits, dev(t), dev(k), dev(p), dev(u), probe=dev(probe), exclude=dev(exclude), probe_prob=prob)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if prob is None else prob.cpu().numpy())


def _argmax(logits):
    from omniserve_amd.backend import fused_ext
    out = torch.empty((logits.shape[0],), dtype=torch.int64, device=DEV)
    fused_ext.argmax(out, logits)
    return out.cpu().numpy()


def test_case_grid_against_the_oracle():
    """Every row of every case (sampling_cases.cases(): cols 1 .. 128256, 1 / 3 / 17 rows, dense / strided / 2-byte-aligned rows,
    nine profiles, the parameter grid mixed within a launch, probe and exclude set).  Greedy rows: fused_ext.argmax's token, probe
    probability 1 / 0.  Every other row, none left out: the token is in the oracle's kept set less `exclude`, and u lies within
    DELTA = 2e-5 of its interval of the canonical-order CDF; probe_prob within 2e-5 * ref + 1e-9 of the oracle's, exactly 0 for a
    filtered-out token.  Measured on the MI355X: largest distance outside the interval 0 (every u inside its token's interval as
    the oracle computes it); largest probe_prob error 1.2 % of its bound."""
    worst, worst_prob, failures, checked = 0.0, 0.0, [], 0
    for case in sc.cases():
        logits = _device_logits(case)
        tok, prob = _sample(logits, case.temperature, case.top_k, case.top_p, case.u, case.probe, case.exclude)
        greedy_tok = _argmax(logits)
        for r, o in enumerate(sc.case_oracles(case)):
            where = "%s row %d (%s, T %g k %d p %g)" % (case.name, r, case.profiles[r], case.temperature[r], case.top_k[r],
                                                       case.top_p[r])
            t, pr = int(tok[r]), int(case.probe[r])
            if o.greedy:
                if t != int(greedy_tok[r]) or t != o.argmax:
                    failures.append("%s: greedy token %d, arg-max %d / %d" % (where, t, int(greedy_tok[r]), o.argmax))
                if prob[r] != (1.0 if pr == t else 0.0):
                    failures.append("%s: greedy probe_prob %g" % (where, prob[r]))
                continue
            checked += 1
            if len(o.order) == 0:      # the excluded token was the whole kept set
                if t != int(case.exclude[r]):
                    failures.append("%s: emptied kept set must hand back the excluded token, got %d" % (where, t))
            else:
                dist = sc.outside_interval(o, t, case.u[r])
                if dist is None:
                    failures.append("%s: token %d is not in the kept set less exclude" % (where, t))
                else:
                    worst = max(worst, dist)
                    if dist > sc.DELTA:
                        failures.append("%s: u %.8g lies %.3g outside token %d's interval" % (where, case.u[r], dist, t))
            ref = float(o.prob[pr]) if pr >= 0 else 0.0
            if ref == 0.0:
                if prob[r] != 0.0:
                    failures.append("%s: probe_prob %g for a filtered-out token" % (where, prob[r]))
            else:
                worst_prob = max(worst_prob, abs(float(prob[r]) - ref) / (2e-5 * ref + 1e-9))
                if abs(float(prob[r]) - ref) > 2e-5 * ref + 1e-9:
                    failures.append("%s: probe_prob %.9g, oracle %.9g" % (where, prob[r], ref))
    print("non-greedy rows checked: %d; largest distance outside the interval: %.3g (delta %.3g); largest probe_prob error as a "
          "share of its bound: %.3g" % (checked, worst, sc.DELTA, worst_prob))
    assert not failures, "\n".join(failures[:20])
    assert checked > 200


def test_greedy_rows_are_argmax_bit_for_bit():
    """The three parameter triggers, and rows whose maximum is NaN / +inf or that hold nothing but -inf, on one launch with
    ordinary parameters beside them; ties, -0 / +0 and several NaNs so that `first maximum` matters."""
    rng = np.random.default_rng(9)
    cols = 4099
    x = (rng.standard_normal((9, cols)) * 2).astype(np.float16)
    x[:, 100] = x[:, 3000] = 9.0                       # a tied maximum: the first one counts
    x[3, 77] = x[3, 2000] = np.float16("nan")
    x[4, 500] = x[4, 20] = np.float16("inf")
    x[5, :] = -np.inf
    x[6, :] = np.where(rng.random(cols) < 0.5, np.float16(-0.0), np.float16(0.0))       # maximum 0 with both signs
    t = np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 9e-6, 1.0, 1.0], dtype=np.float32)
    k = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.int32)
    p = np.array([1.0, 1e-9, 1.0, 0.9, 0.9, 0.9, 0.9, 1e-9, 0.0], dtype=np.float32)
    u = rng.random(9).astype(np.float32)
    logits = torch.from_numpy(x).to(DEV)
    want = _argmax(logits)
    probe = want.copy()
    probe[::2] = 5
    tok, prob = _sample(logits, t, k, p, u, probe, None)
    assert np.array_equal(tok, want)
    assert np.array_equal(want, [sc.argmax_ref(x[r]) for r in range(9)])
    assert np.array_equal(prob, (probe == want).astype(np.float32))


def test_exclusion():
    """The excluded token is never returned while another token is kept (every u of a sweep); with a kept set of one it is
    returned, and its probe probability is 1.  Without probe / exclude the call equals the one with -1 everywhere."""
    rows = 64
    x = np.tile(np.array([3.0, 1.0, 2.5, -1.0, 2.5, 0.0, -np.inf], dtype=np.float16), (rows, 1))
    u = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    logits = torch.from_numpy(x).to(DEV)
    for excl in (0, 2, 6):
        e = np.full(rows, excl, dtype=np.int64)
        tok, prob = _sample(logits, 1.0, 0, 1.0, u, e, e)
        assert not (tok == excl).any() and not (tok == 6).any()
        o = sc.oracle_row(x[0], 1.0, 0, 1.0, exclude=excl)
        assert all(sc.outside_interval(o, int(tok[r]), u[r]) <= sc.DELTA for r in range(rows))
        assert np.allclose(prob, sc.oracle_row(x[0], 1.0, 0, 1.0).prob[excl], rtol=2e-5, atol=1e-9)
    e = np.zeros(rows, dtype=np.int64)
    tok, prob = _sample(logits, 1.0, 0, 0.3, u, e, e)          # top-p 0.3 keeps the maximum alone
    assert (tok == 0).all() and (prob == 1.0).all()
    one = torch.from_numpy(np.full((3, 1), 0.5, dtype=np.float16)).to(DEV)      # one column
    tok, prob = _sample(one, 1.0, 0, 1.0, u[:3], e[:3], e[:3])
    assert (tok == 0).all() and (prob == 1.0).all()
    none = np.full(rows, -1, dtype=np.int64)
    a, _ = _sample(logits, 1.0, 3, 0.9, u, none, none)
    b, _ = _sample(logits, 1.0, 3, 0.9, u)
    assert np.array_equal(a, b)


def test_stratified_draw():
    """4096 rows of the same 8-token logits with u_i = (i + 0.5) / 4096: every token's count is within 1 of p * 4096 and the rows'
    tokens are monotone in canonical order."""
    n = 4096
    row = np.array([0.25, 2.0, -1.0, 1.0, 2.0, -0.5, 0.5, 1.5], dtype=np.float16)
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    tok, _ = _sample(torch.from_numpy(np.tile(row, (n, 1))).to(DEV), 0.8, 0, 1.0, u)
    o = sc.oracle_row(row, 0.8, 0, 1.0)
    counts = np.bincount(tok, minlength=8)
    assert np.abs(counts - o.prob * n).max() <= 1.0, (counts, o.prob * n)
    rank = np.empty(8, dtype=np.int64)
    rank[o.order] = np.arange(8)
    assert o.order.tolist() == [1, 4, 7, 3, 6, 0, 5, 2]
    assert (np.diff(rank[tok]) >= 0).all()


def test_determinism_and_slices():
    """Two launches give equal bits; rows 0..7 and 8..16 sampled separately (other grids, other base pointers, other workspace
    offsets) give the bits of the whole call."""
    case = next(c for c in sc.cases() if c.name == "c4099_r17_strided")
    logits = _device_logits(case)
    args = (case.temperature, case.top_k, case.top_p, case.u, case.probe, case.exclude)
    tok, prob = _sample(logits, *args)
    tok2, prob2 = _sample(logits, *args)
    assert np.array_equal(tok, tok2) and np.array_equal(prob.view(np.uint32), prob2.view(np.uint32))
    for lo, hi in ((0, 8), (8, 17)):
        t, q = _sample(logits[lo:hi], *[a[lo:hi] for a in args])
        assert np.array_equal(t, tok[lo:hi]) and np.array_equal(q.view(np.uint32), prob[lo:hi].view(np.uint32))
