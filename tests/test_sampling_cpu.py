"""Sampled decoding without a GPU: the f64 oracle against the reference's rule, the fairness of every GPU case, accept_sampled,
exact distribution preservation of the rejection rule, and the mirror's argument errors."""
import itertools

import numpy as np
import pytest
import torch

import sampling_cases as sc


def _hf_rows():
    rng = np.random.default_rng(3)
    rows = []
    for cols in (2, 7, 64, 500):
        for _ in range(6):
            x = np.unique((rng.standard_normal(4 * cols) * 3).astype(np.float16))      # tie-free
            rows.append(rng.permutation(x)[:cols])
    return [x for x in rows if len(x) >= 2]


def test_oracle_kept_set_is_the_reference_rule_on_tie_free_rows():
    n = 0
    for x in _hf_rows():
        for T, k, p in itertools.product((0.3, 1.0, 2.5), (0, 2, 50, len(x), len(x) + 5), (1.0, 0.9, 0.5)):
            if not sc.row_is_fair(x, T, k, p):
                continue
            o = sc.oracle_row(x, T, k, p)
            assert not o.greedy
            assert np.array_equal(o.kept, sc.hf_kept(x, T, k, p)), (len(x), T, k, p)
            n += 1
    assert n > 500


def test_oracle_kept_set_is_a_superset_by_ties_only():
    """Rows with ties at the threshold: the reference's top-p warper cuts inside the run of equal logits (wherever its sort left
    them); the contract keeps the whole run.  Every token the oracle keeps beyond the reference's set ties with the smallest value
    the reference kept."""
    rng = np.random.default_rng(4)
    extra = 0
    for cols in (8, 64, 500):
        for _ in range(8):
            x = rng.choice(np.array([-1.0, 0.0, 0.5, 0.75, 2.0], dtype=np.float16), size=cols)
            for T, k, p in itertools.product((0.3, 1.0, 2.5), (0, 2, 50, cols), (1.0, 0.9, 0.5)):
                o = sc.oracle_row(x, T, k, p)
                if not sc.row_is_fair(x, T, k, p):
                    continue
                ref = sc.hf_kept(x, T, k, p)
                assert not (ref & ~o.kept).any()
                more = o.kept & ~ref
                if more.any():
                    assert (x[more] == x[ref].min()).all()
                    extra += 1
    assert extra > 0


def test_every_gpu_case_is_fair():
    """A condition on the cases, not a tolerance: the oracle alone decides every row's kept set (sampling_cases.row_is_fair)."""
    cases = sc.cases()
    seen_profiles, seen_combos, seen_layouts, non_greedy = set(), set(), set(), 0
    for c in cases:
        seen_layouts.add(c.layout)
        for r in range(c.rows):
            assert sc.row_is_fair(c.logits[r], c.temperature[r], c.top_k[r], c.top_p[r]), (c.name, r)
            assert 0.0 <= c.u[r] < 1.0
            seen_profiles.add(c.profiles[r])
            seen_combos.add((float(c.temperature[r]), float(c.top_p[r])))
            non_greedy += not sc.is_greedy(c.logits[r], c.temperature[r], c.top_k[r], c.top_p[r])
    assert seen_profiles == set(sc.PROFILE_NAMES) and seen_layouts == set(sc.LAYOUTS)
    assert {c.cols for c in cases} == set(sc.COLS) | {128256} and {c.rows for c in cases} >= set(sc.ROWS)
    assert len(seen_combos) >= len(sc.TEMPERATURES) * len(sc.TOP_PS) and non_greedy > 200
    special = sc.cases()[-1]
    keys = [sc.keys_of(special.logits[r]) for r in range(special.rows)]
    o = sc.case_oracles(special)
    assert int(o[0].kept.sum()) == 1020 and int(o[1].kept.sum()) == 1020      # the 1000-way tie is kept whole
    # top-k cuts in the high byte of the three top tokens, top-p (alone) in one of the bulk's: different bins
    assert int(keys[4][o[4].kept].min()) >> 8 != int(keys[7][o[7].kept].min()) >> 8


def _accept_loop(prob, u, drawn):
    m, nxt = [], []
    for b in range(len(prob)):
        a = 0
        while a < len(prob[b]) - 1 and u[b][a] < prob[b][a]:
            a += 1
        m.append(1 + a)
        nxt.append(drawn[b][a])
    return m, nxt


def test_accept_sampled_against_a_loop():
    from omniserve_amd.runtime import accept_sampled
    g = torch.Generator().manual_seed(5)
    for n in (1, 2, 4, 8):
        prob = torch.rand((64, n), generator=g)
        prob[::3] = torch.round(prob[::3])          # probabilities 0 and 1
        u = torch.rand((64, n), generator=g)
        drawn = torch.randint(0, 1000, (64, n), generator=g)
        m, nxt = accept_sampled(prob, u, drawn)
        rm, rn = _accept_loop(prob.tolist(), u.tolist(), drawn.tolist())
        assert m.dtype == torch.int64 and m.tolist() == rm and nxt.tolist() == rn
    # an accept behind a rejection does not count; probability 1 always accepts, 0 never (u = 0 included)
    prob = torch.tensor([[0.9, 0.0, 1.0, 0.3], [1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 1.0, 1.0]])
    u = torch.tensor([[0.1, 0.0, 0.0, 0.0], [0.999, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    drawn = torch.arange(12).view(3, 4)
    m, nxt = accept_sampled(prob, u, drawn)
    assert m.tolist() == [2, 4, 1] and nxt.tolist() == [1, 7, 8]


def test_rejection_rule_preserves_the_filtered_distribution_exactly():
    """Accept the drafted token x with p(x), else draw from p without x: the marginal over the emitted token is p, to 1e-12, with
    p and the draw-without-x distribution both taken from the oracle -- p(x) = 1 and p(x) = 0 (x filtered out) included."""
    rng = np.random.default_rng(6)
    checked = set()
    for V in range(2, 7):
        for T, k, p in ((1.0, 0, 1.0), (0.7, 2, 1.0), (2.5, 0, 0.6), (1.0, 1 + V // 2, 0.9), (1.0, 0, 0.05)):
            x = (rng.standard_normal(V) * 2).astype(np.float16)
            base = sc.oracle_row(x, T, k, p)
            for drafted in range(V):
                px = float(base.prob[drafted])
                o = sc.oracle_row(x, T, k, p, exclude=drafted)
                marg = np.zeros(V)
                marg[drafted] += px
                if len(o.order):
                    marg[o.order] += (1.0 - px) * (o.cdf_hi - o.cdf_lo)
                else:
                    assert px == 1.0
                assert np.abs(marg - base.prob).max() <= 1e-12, (V, T, k, p, drafted)
                checked.add("one" if px == 1.0 else ("zero" if px == 0.0 else "mid"))
    assert checked == {"one", "zero", "mid"}


def test_mirror_argument_errors():
    from omniserve_amd.backend import fused_ext
    lg = torch.zeros((3, 16), dtype=torch.float16)
    out = torch.zeros((3,), dtype=torch.int64)
    u = torch.zeros((3,), dtype=torch.float32)

    def call(**kw):
        a = dict(out=out, logits=lg, temperature=1.0, top_k=0, top_p=1.0, u=u)
        a.update(kw)
        fused_ext.sample(**a)

    for bad, what in ((dict(logits=lg.float()), "logits"), (dict(out=out.int()), "out"), (dict(out=out[:2]), "out"),
                      (dict(u=u.double()), "u"), (dict(u=u[:2]), "u"), (dict(u=0.5), "u"),
                      (dict(temperature=torch.ones(2)), "temperature"), (dict(top_k=torch.zeros(3, dtype=torch.int64)), "top_k"),
                      (dict(top_p=torch.ones(3, dtype=torch.float16)), "top_p"),
                      (dict(probe_prob=torch.zeros(3)), "probe_prob needs probe"),
                      (dict(probe=torch.zeros(3, dtype=torch.int32)), "probe"),
                      (dict(probe=torch.zeros(3, dtype=torch.int64), probe_prob=torch.zeros(2)), "probe_prob"),
                      (dict(exclude=torch.zeros(4, dtype=torch.int64)), "exclude")):
        with pytest.raises(RuntimeError, match=what):
            call(**bad)
    with pytest.raises(RuntimeError, match="device tensors"):      # all checks passed: no CPU fallback
        call()


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    from omniserve_amd import _lib
    h = _lib.lib()
    need = h.omni_sample_workspace_bytes(3, 16)
    assert need > 0 and h.omni_sample_workspace_bytes(0, 16) == 0
    ok = (1, None, 1, 16, 3, 16, 1, 1, 1, 1, None, None, 1, need, None)

    def call(**kw):
        names = ("tok", "pp", "lg", "stride", "rows", "cols", "t", "k", "p", "u", "probe", "excl", "ws", "wsb", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return h.omni_sample_f16(*[a[n] for n in names])

    assert call(tok=None) == -22 and call(lg=None) == -22 and call(u=None) == -22 and call(ws=None) == -22
    assert call(stride=8) == -22 and call(cols=0) == -22 and call(rows=-1) == -22
    assert call(pp=1) == -22                                  # probe_prob without probe
    assert call(wsb=need - 1) == -12
    assert call(rows=0) == 0
