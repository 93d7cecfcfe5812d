"""Log-probabilities through DecodeRunner (tests/runner_cases.py's shape: LlamaConfig.tiny, B = 3, L = 150, eager unless said):
score() is prefill() plus the prompt's log-probabilities, the `logprobs` buffers describe the pending token after every method
that sets it, and the feature only reads.  A spy around fused_ext.logprobs records the logits blocks and targets it is handed, so
the oracle (tests/logprob_cases.py) is applied to the very rows the runner scored."""
import contextlib

import numpy as np
import pytest
import torch

import logprob_cases as lc
import runner_cases as rc
from runner_cases import B, L, N

pytestmark = pytest.mark.gpu


def _runner(use_graph=False, sampling=False, logprobs=None):
    from omniserve_amd.runtime import DecodeRunner, LlamaConfig
    return DecodeRunner(LlamaConfig.tiny(), B, 70, 100, torch.device("cuda:0"), seed=11, use_graph=use_graph, fused=2,
                        sampling=sampling, logprobs=logprobs)


@contextlib.contextmanager
def _spy():
    """calls: one (logits fp16 [rows, vocab] on the host, targets int64 [rows], n_top, result) per fused_ext.logprobs call."""
    from omniserve_amd.backend import fused_ext
    real, calls = fused_ext.logprobs, []

    def wrapped(logits, target=None, n_top=0, **kw):
        out = real(logits, target=target, n_top=n_top, **kw)
        calls.append((logits.cpu().numpy().copy(), None if target is None else target.cpu().numpy().copy(), n_top,
                      type(out)(*[None if t is None else t.clone() for t in out])))
        return out

    fused_ext.logprobs = wrapped
    try:
        yield calls
    finally:
        fused_ext.logprobs = real


def _state(r):
    torch.cuda.synchronize()
    return dict(lengths=r.lengths.clone(), tokens=r.tokens.clone(), x=r.x.clone(), normed=r.normed.clone(), pools=rc.pools(r))


def _same_state(a, b):
    assert torch.equal(a["lengths"], b["lengths"]) and torch.equal(a["tokens"], b["tokens"])
    assert torch.equal(a["x"].view(torch.int16), b["x"].view(torch.int16))
    assert torch.equal(a["normed"].view(torch.int16), b["normed"].view(torch.int16))
    for pa, pb in zip(a["pools"], b["pools"]):
        for u, v in zip(pa, pb):
            assert torch.equal(u, v)


_WORST = {"frac": 0.0}


def _check_rows(logits, targets, n_top, logprob, rank, top_tokens=None, top_logprobs=None, what=""):
    """The kernel test's bounds on rows the runner scored: ranks / tokens equal, values within 2e-5 + 2^-22 |ref|."""
    for i in range(logits.shape[0]):
        o = lc.oracle_row(logits[i])
        ref_lp, ref_rank = o.target(int(targets[i]))
        assert int(rank[i]) == ref_rank, (what, i)
        vals, refs = [float(logprob[i])], [ref_lp]
        if n_top:
            tok, lp = o.top(n_top)
            assert np.array_equal(np.asarray(top_tokens[i]), tok), (what, i)
            vals += list(np.asarray(top_logprobs[i], dtype=np.float64))
            refs += list(lp)
        exact, frac, err = lc.value_errors(np.array(vals), np.array(refs))
        _WORST["frac"] = max(_WORST["frac"], frac)
        assert exact and frac <= 1.0, "%s row %d: |err| %.3g is %.3g of the bound" % (what, i, err, frac)


@pytest.mark.parametrize("chunk", [None, 64], ids=["whole", "chunk64"])
def test_score_is_prefill_plus_the_prompts_logprobs(chunk):
    fresh = _runner()
    tokens = rc.prompt(fresh)
    fresh.prefill(L, tokens.reshape(-1), chunk=chunk)
    want = _state(fresh)
    r = _runner()
    with _spy() as calls:
        res = r.score(tokens, chunk=chunk, top=5)
    _same_state(_state(r), want)
    assert res.logprob.shape == (B, L - 1) and res.rank.shape == (B, L - 1) and res.rank.dtype == torch.int32
    assert res.top_tokens.shape == (B, L - 1, 5) and res.top_logprobs.shape == (B, L - 1, 5)
    # the blocks: chunk by chunk, sequence after sequence inside a chunk; together each of the B * (L - 1) rows exactly once
    step = L if chunk is None else chunk
    assert len(calls) == -(-L // step)
    tk = tokens.cpu().numpy()
    lp, rk = res.logprob.cpu().numpy(), res.rank.cpu().numpy()
    tt, tl = res.top_tokens.cpu().numpy(), res.top_logprobs.cpu().numpy()
    covered = np.zeros((B, L - 1), dtype=np.int64)
    for (logits, targets, n_top, _), s in zip(calls, range(0, L, step)):
        k = min(step, L - 1 - s)
        assert n_top == 5 and logits.shape == (B * k, r.cfg.vocab)
        assert np.array_equal(targets.reshape(B, k), tk[:, s + 1:s + 1 + k])
        covered[:, s:s + k] += 1
        sel = (slice(None), slice(s, s + k))
        _check_rows(logits, targets, 5, lp[sel].reshape(-1), rk[sel].reshape(-1), tt[sel].reshape(B * k, 5),
                    tl[sel].reshape(B * k, 5), what="score chunk at %d" % s)
    assert (covered == 1).all()
    # block_rows: more calls, the same bits; top = 0: no lists, the same bits
    r2 = _runner()
    with _spy() as calls2:
        res2 = r2.score(tokens, chunk=chunk, block_rows=64)
    assert len(calls2) > len(calls) and all(c[0].shape[0] <= 64 for c in calls2)
    assert sum(c[0].shape[0] for c in calls2) == B * (L - 1)
    assert res2.top_tokens is None and res2.top_logprobs is None
    assert torch.equal(res2.logprob.view(torch.int32), res.logprob.view(torch.int32)) and torch.equal(res2.rank, res.rank)
    _same_state(_state(r2), want)
    from omniserve_amd.runtime import perplexity
    ppl = perplexity(res.logprob)
    assert ppl.shape == (B,) and bool(torch.isfinite(ppl).all()) and bool((ppl > 1).all())
    print("score(chunk=%s): worst |err| / bound so far %.3g; perplexity %s" % (chunk, _WORST["frac"], ppl.tolist()))


def _check_buffers(r, call, what):
    """The runner's buffers describe r.tokens on the spied call's rows (one row per sequence, gathered by the caller)."""
    logits, targets = call
    torch.cuda.synchronize()
    assert np.array_equal(targets, r.tokens.cpu().numpy()), what
    n = r.logprobs
    _check_rows(logits, targets, n, r.token_logprob.cpu().numpy(), r.token_rank.cpu().numpy(),
                r.top_tokens.cpu().numpy() if n else None, r.top_logprobs.cpu().numpy() if n else None, what=what)


def _kept_rows(call, kept):
    """Of a spied call over B * n rows: the row of each sequence's kept position."""
    logits, targets = call[0], call[1]
    n = logits.shape[0] // B
    idx = np.arange(B) * n + np.asarray(kept)
    return logits[idx], targets[idx]


def test_greedy_runner_buffers_follow_every_method_that_sets_the_token():
    r = _runner(logprobs=5)
    tokens = rc.prompt(r)
    g = torch.Generator(device=r.device)
    g.manual_seed(6)
    more = torch.randint(0, r.cfg.vocab, (B, 3), device=r.device, generator=g)

    def greedy(what):
        assert torch.equal(r.top_tokens[:, 0], r.tokens) and bool((r.token_rank == 1).all()), what

    with _spy() as calls:
        r.prefill(L, tokens.reshape(-1))
        assert len(calls) == 1
        _check_buffers(r, calls[-1][:2], "prefill")
        greedy("prefill")
        r.extend(3, more.reshape(-1))
        assert len(calls) == 2
        _check_buffers(r, calls[-1][:2], "extend")
        greedy("extend")
        for i in range(4):
            r.step()
            assert len(calls) == 3 + i
            _check_buffers(r, calls[-1][:2], "step %d" % i)
            greedy("step")
        draft = rc.random_draft(r, 9)
        pred, m = r.verify(draft)
        assert len(calls) == 7 and calls[-1][0].shape[0] == B * N
        assert np.array_equal(calls[-1][1], pred.reshape(-1).cpu().numpy())
        _check_buffers(r, _kept_rows(calls[-1], (m - 1).cpu().numpy()), "verify")
        greedy("verify")
        tree = torch.cat([r.tokens.view(B, 1), more, more[:, :2]], dim=1)
        pred, path, m = r.verify_tree(tree, [-1, 0, 0, 1, 1, 2])
        assert len(calls) == 8 and calls[-1][0].shape[0] == B * 6
        kept = path.gather(1, (m - 1).view(B, 1)).squeeze(1).cpu().numpy()
        _check_buffers(r, _kept_rows(calls[-1], kept), "verify_tree")
        greedy("verify_tree")


def test_captured_steps_leave_the_eager_runners_buffers_bit_for_bit():
    runs = []
    for use_graph in (False, True):
        r = _runner(use_graph=use_graph, logprobs=5)
        r.prefill(L, rc.prompt(r).reshape(-1))
        seq = []
        for _ in range(4):
            r.step()
            torch.cuda.synchronize()
            seq.append((r.tokens.clone(), r.token_logprob.view(torch.int32).clone(), r.token_rank.clone(), r.top_tokens.clone(),
                        r.top_logprobs.view(torch.int32).clone()))
        runs.append(seq)
        assert (r.graph is not None) == use_graph
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_sampled_runner_records_the_raw_logprob_of_the_drawn_token():
    r = _runner(sampling=True, logprobs=0)
    r.set_sampling(temperature=1.0, top_k=0, top_p=0.9, seed=3)
    with _spy() as calls:
        r.prefill(L, rc.prompt(r).reshape(-1))
        _check_buffers(r, calls[-1][:2], "sampled prefill")
        ranks = [r.token_rank.clone()]
        for i in range(4):
            r.step()
            _check_buffers(r, calls[-1][:2], "sampled step %d" % i)      # the RAW log-probability: no top-p in the oracle
            ranks.append(r.token_rank.clone())
        drawn, m = r.verify(rc.random_draft(r, 9))
        _check_buffers(r, _kept_rows(calls[-1], (m - 1).cpu().numpy()), "sampled verify")
        ranks.append(r.token_rank.clone())
    assert all(c[2] == 0 for c in calls) and r.top_tokens.shape == (B, 0)
    ranks = torch.stack(ranks)
    assert int(ranks.min()) >= 1 and int(ranks.max()) > 1, "temperature 1 never left the arg-max in 18 draws"


def test_the_feature_only_reads():
    on, off = _runner(logprobs=5), _runner(logprobs=None)
    for name in ("token_logprob", "token_rank", "top_tokens", "top_logprobs"):
        assert hasattr(on, name) and not hasattr(off, name)
    tokens = rc.prompt(on)
    with _spy() as calls:
        off.prefill(L, tokens.reshape(-1))
        toks_off, x_off = rc.four_steps(off)
        assert calls == []
        on.prefill(L, tokens.reshape(-1))
        toks_on, x_on = rc.four_steps(on)
        assert len(calls) == 5
    assert torch.equal(toks_on, toks_off) and torch.equal(x_on.view(torch.int16), x_off.view(torch.int16))
    _same_state(_state(on), _state(off))


def test_entry_errors():
    r = _runner()
    tokens = rc.prompt(r)
    for bad, what in ((tokens.int(), "int64"), (tokens[:2], "int64"), (tokens.reshape(-1), "int64"), (tokens[:, :1], "two tokens"),
                      (torch.zeros((B, 171), dtype=torch.int64), "KV pools")):
        with pytest.raises(ValueError, match=what):
            r.score(bad)
    for kw, what in ((dict(top=21), "top"), (dict(top=-1), "top"), (dict(block_rows=0), "block_rows"), (dict(chunk=0), "chunk")):
        with pytest.raises(ValueError, match=what):
            r.score(tokens, **kw)
    for bad in (-1, 21, 1.5):
        with pytest.raises(ValueError, match="logprobs"):
            _runner(logprobs=bad)
