"""Log-probabilities without a GPU: the f64 oracle against torch, the case grid's coverage, the C entry's
and the mirror's argument errors, perplexity, and the runner's new surface."""
import inspect

import numpy as np
import pytest
import torch

import logprob_cases as lc
from sampling_cases import keys_of


def _tie_free_rows():
    rng = np.random.default_rng(3)
    rows = []
    for cols in (2, 7, 64, 500):
        for _ in range(4):
            x = np.unique((rng.standard_normal(4 * cols) * 3).astype(np.float16))
            x = x[x != 0]      # (+0 / -0 would tie by key)
            rows.append(rng.permutation(x)[:cols])
    return [x for x in rows if len(x) >= 2]


def test_oracle_is_log_softmax_in_f64_and_topk_on_tie_free_rows():
    for x in _tie_free_rows():
        o = lc.oracle_row(x)
        ref = torch.log_softmax(torch.from_numpy(x.astype(np.float64)), dim=-1)
        assert np.abs(o.logprob - ref.numpy()).max() <= 1e-12
        assert abs(o.lse - float(torch.logsumexp(torch.from_numpy(x.astype(np.float64)), dim=-1))) <= 1e-12
        n = min(20, len(x))
        tok, lp = o.top(n)
        tv, ti = torch.topk(ref, n)
        assert np.array_equal(tok, ti.numpy()) and np.abs(lp - tv.numpy()).max() <= 1e-12
        for t in (0, len(x) - 1, int(tok[0])):
            assert o.target(t) == (float(o.logprob[t]), 1 + int((ref > ref[t]).sum()))
    x = np.array([1.0, -np.inf, 0.5, -np.inf], dtype=np.float16)      # -inf weighs 0 and its log-probability is -inf
    o = lc.oracle_row(x)
    ref = torch.log_softmax(torch.from_numpy(x.astype(np.float64)), dim=-1).numpy()
    assert np.array_equal(np.isneginf(o.logprob), np.isneginf(ref)) and np.abs(o.logprob[[0, 2]] - ref[[0, 2]]).max() <= 1e-12


def test_oracle_tie_order_padding_targets_and_degenerate_rows():
    x = np.array([0.5, 2.0, -0.0, 2.0, 0.0, 0.5, 2.0], dtype=np.float16)
    o = lc.oracle_row(x)
    assert o.order.tolist() == [1, 3, 6, 0, 5, 2, 4]       # ties by index ascending; -0 == +0
    assert o.rank.tolist() == [4, 1, 6, 2, 7, 5, 3]
    tok, lp = o.top(9)
    assert tok.tolist() == [1, 3, 6, 0, 5, 2, 4, -1, -1] and np.isneginf(lp[7:]).all() and np.isfinite(lp[:7]).all()
    assert lc.oracle_row(np.full(5, 3.0, dtype=np.float16)).top(3)[0].tolist() == [0, 1, 2]
    for t in (-1, 7):
        lp_t, rank_t = o.target(t)
        assert np.isnan(lp_t) and rank_t == 0
    for bad in (np.array([1.0, np.nan, 2.0]), np.array([1.0, np.inf, 2.0]), np.array([-np.inf] * 3)):
        d = lc.oracle_row(bad.astype(np.float16))
        assert np.isnan(d.lse) and np.isnan(d.logprob).all()
        assert d.order.tolist() == [1, 2, 0] or d.order.tolist() == [0, 1, 2]      # still the key's
        assert d.target(int(d.order[0]))[1] == 1 and np.isnan(d.target(0)[0])
        assert d.top(4)[0].tolist() == d.order.tolist() + [-1]
    assert lc.oracle_row(np.array([-np.inf] * 3, dtype=np.float16)).order.tolist() == [0, 1, 2]


def test_case_grid_covers_what_the_contract_names():
    """A condition on the cases: every profile, layout, n_top and target class; the column counts around the kernel's
    granularities (taken from the constants the mirror exports); n_top > cols; top lists that reach -inf entries; a top-list
    boundary inside a tie run; a tie run across a chunk edge."""
    from omniserve_amd.backend import fused_ext
    assert (lc.CHUNKS, lc.VEC, lc.MAX_TOP) == (fused_ext.LOGPROB_CHUNKS, fused_ext.LOGPROB_VEC, fused_ext.LOGPROB_MAX_TOP)
    for cols in (1, 8, 9, 256, 257, 65537, 128256, 1 << 22):
        assert lc.chunk_cols(cols) == fused_ext.logprob_chunk_cols(cols)
        assert lc.chunk_cols(cols) % lc.VEC == 0 and lc.chunk_cols(cols) * lc.CHUNKS >= cols
    cases = lc.cases()
    all_cols = {c.cols for c in cases}
    assert all_cols >= {1, 2, 7, 255, 256, 257, 128256}
    chunk, stride = lc.CHUNKS * lc.VEC, lc.CHUNKS * lc.VEC * 256
    for g in (lc.VEC, lc.CHUNKS, chunk, stride):      # one below / at / one above
        assert {g - 1, g, g + 1} <= all_cols, g
    assert lc.chunk_cols(chunk) == lc.VEC and lc.chunk_cols(chunk + 1) == 2 * lc.VEC
    assert {c.rows for c in cases} == set(lc.ROWS) and {c.layout for c in cases} == set(lc.LAYOUTS)
    assert {c.n_top for c in cases} == set(lc.N_TOPS)
    assert any(c.n_top > c.cols for c in cases)
    seen_profiles, seen_targets, by_profile = set(), set(), {}
    for c in cases:
        assert c.logits.dtype == np.float16 and c.logits.shape == (c.rows, c.cols) and c.target.shape == (c.rows,)
        seen_profiles.update(c.profiles)
        seen_targets.update(c.target_classes)
        for r in range(c.rows):
            by_profile.setdefault(c.profiles[r], []).append((c, r))
    assert seen_profiles == set(lc.PROFILE_NAMES) and seen_targets == set(lc.TARGET_CLASSES)
    for name in lc.PROFILE_NAMES:      # each profile meets every layout and a top list
        assert {c.layout for c, _ in by_profile[name]} == set(lc.LAYOUTS), name
        assert any(c.n_top > 0 for c, _ in by_profile[name]), name
    edge_targets = 0
    for c in cases:
        edges = lc.chunk_edges(c.cols)
        for r in range(c.rows):
            cls, t = c.target_classes[r], int(c.target[r])
            assert {"first": t == 0, "last": t == c.cols - 1, "minus_one": t == -1, "cols": t == c.cols}.get(cls, True)
            if edges and cls == "edge_lo":
                assert t + 1 in edges
                edge_targets += 1
            if edges and cls == "edge_hi":
                assert t in edges
                edge_targets += 1
    assert edge_targets >= 20
    reaches_neg_inf = tie_at_boundary = tie_across_edge = 0
    for c, r in by_profile["mostly_neg_inf"]:
        if 0 < c.n_top <= c.cols:
            reaches_neg_inf += bool(np.isneginf(lc.case_oracles(c)[r].top(c.n_top)[1]).any())
    for c, r in by_profile["two_valued"]:
        if 0 < c.n_top < c.cols:
            o, k = lc.case_oracles(c)[r], keys_of(c.logits[r])
            tie_at_boundary += bool(k[o.order[c.n_top - 1]] == k[o.order[c.n_top]])
    for c, r in by_profile["tie_across_edge"]:
        k = keys_of(c.logits[r])
        for e in lc.chunk_edges(c.cols):
            tie_across_edge += bool(k[e - 1] == k[e] == k.max())
    assert reaches_neg_inf > 0 and tie_at_boundary > 0 and tie_across_edge > 0
    for name, pred in (("all_neg_inf", True), ("nan", True), ("pos_inf", True), ("gaussian", False), ("extremes", False)):
        assert all(lc.is_degenerate(c.logits[r]) == pred for c, r in by_profile[name]), name


def test_c_entries_are_exported_and_reject_bad_arguments_without_a_gpu():
    from omniserve_amd import _lib
    h = _lib.lib()
    assert "omni_logprob_workspace_bytes" in _lib.PROTOTYPES and "omni_logprob_f16" in _lib.PROTOTYPES
    need0, need = h.omni_logprob_workspace_bytes(3, 16, 0), h.omni_logprob_workspace_bytes(3, 16, 5)
    assert 0 < need0 < need and h.omni_logprob_workspace_bytes(0, 16, 5) == 0
    assert h.omni_logprob_workspace_bytes(3, 16, 21) == 0 and h.omni_logprob_workspace_bytes(3, 0, 0) == 0
    assert h.omni_abi_version() == 4
    names = ("lse", "tlp", "rank", "tt", "tl", "lg", "stride", "rows", "cols", "target", "n_top", "ws", "wsb", "stream")
    ok = (1, 1, 1, 1, 1, 1, 16, 3, 16, 1, 5, 1, need, None)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return h.omni_logprob_f16(*[a[n] for n in names])

    assert call(lg=None) == -22 and call(ws=None) == -22
    assert call(stride=8) == -22 and call(cols=0) == -22 and call(cols=(1 << 22) + 1) == -22
    assert call(rows=-1) == -22 and call(rows=65536) == -22
    assert call(n_top=-1) == -22 and call(n_top=21) == -22
    assert call(tt=None) == -22 and call(tl=None) == -22                  # a top list needs both outputs
    assert call(target=None) == -22 and call(target=None, tlp=None) == -22      # token_logprob / rank need the target
    assert call(wsb=need - 1) == -12 and call(n_top=0, wsb=need0 - 1) == -12
    assert call(rows=0) == 0 and call(rows=0, n_top=0, tt=None, tl=None, target=None, tlp=None, rank=None, lse=None) == 0


def test_mirror_argument_errors():
    from omniserve_amd.backend import fused_ext
    lg = torch.zeros((3, 16), dtype=torch.float16)
    tgt = torch.zeros((3,), dtype=torch.int64)

    def call(**kw):
        a = dict(logits=lg, target=tgt, n_top=5)
        a.update(kw)
        return fused_ext.logprobs(**a)

    for bad, what in ((dict(logits=lg.float()), "logits"), (dict(logits=lg.t()), "logits"), (dict(logits=lg[0]), "logits"),
                      (dict(target=tgt.int()), "target"), (dict(target=tgt[:2]), "target"),
                      (dict(target=torch.zeros((6,), dtype=torch.int64)[::2]), "target"),
                      (dict(target=None, token_logprob=torch.zeros(3)), "need target"),
                      (dict(target=None, rank=torch.zeros(3, dtype=torch.int32)), "need target"),
                      (dict(n_top=0, top_tokens=torch.zeros((3, 0), dtype=torch.int64)), "need n_top"),
                      (dict(lse=torch.zeros(3, dtype=torch.float64)), "lse"), (dict(lse=torch.zeros(4)), "lse"),
                      (dict(token_logprob=torch.zeros(2)), "token_logprob"), (dict(rank=torch.zeros(3, dtype=torch.int64)), "rank"),
                      (dict(top_tokens=torch.zeros((3, 4), dtype=torch.int64)), "top_tokens"),
                      (dict(top_tokens=torch.zeros((3, 5), dtype=torch.int32)), "top_tokens"),
                      (dict(top_logprobs=torch.zeros((3, 10))[:, ::2]), "top_logprobs")):
        with pytest.raises(RuntimeError, match=what):
            call(**bad)
    for n in (-1, 21):
        with pytest.raises(ValueError, match="n_top"):
            call(n_top=n)
    with pytest.raises(RuntimeError, match="device tensors"):      # all checks passed: no CPU fallback
        call()


def test_perplexity():
    from omniserve_amd.runtime import perplexity
    lp = torch.tensor([[-1.0, -2.0, -3.0], [-0.5, -0.5, -0.5], [0.0, -float("inf"), -1.0]], dtype=torch.float32)
    ppl = perplexity(lp)
    assert ppl.dtype == torch.float64 and ppl.shape == (3,)
    assert torch.allclose(ppl[:2], torch.tensor([np.exp(2.0), np.exp(0.5)], dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.isinf(ppl[2]) and ppl[2] > 0
    mask = torch.tensor([[True, True, False], [False, True, False], [True, False, True]])
    masked = perplexity(lp, mask)
    assert torch.allclose(masked, torch.tensor([np.exp(1.5), np.exp(0.5), np.exp(0.5)], dtype=torch.float64), rtol=1e-12, atol=0)
    g = torch.Generator().manual_seed(1)
    lp = -torch.rand((4, 37), generator=g) * 9
    assert torch.allclose(perplexity(lp), torch.exp(-lp.double().mean(dim=1)), rtol=1e-12, atol=0)


def test_runner_surface():
    from omniserve_amd import runtime
    sig = inspect.signature(runtime.DecodeRunner.__init__)
    assert sig.parameters["logprobs"].default is None
    score = inspect.signature(runtime.DecodeRunner.score)
    assert list(score.parameters) == ["self", "tokens", "chunk", "top", "block_rows"]
    assert (score.parameters["chunk"].default, score.parameters["top"].default, score.parameters["block_rows"].default) == (None, 0, 1024)
    assert runtime.ScoreResult._fields == ("logprob", "rank", "top_tokens", "top_logprobs")
    for bad in (-1, 21, 2.0, "5", True):      # checked before anything touches a device
        with pytest.raises(ValueError, match="logprobs"):
            runtime.DecodeRunner(runtime.LlamaConfig.tiny(), 1, 8, 8, torch.device("cpu"), logprobs=bad)
