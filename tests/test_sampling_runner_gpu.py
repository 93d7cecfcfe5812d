"""Sampled decoding through the runners (LlamaConfig.tiny, B = 3, prompt 150, as tests/test_verify_runner_gpu.py): the defaults
stay greedy bit for bit, set_sampling() reaches a captured step, sampled verify() follows the rejection rule."""
import pytest
import torch

import sampling_cases as sc
from runner_cases import B, L, N, prefilled as _prefilled, random_draft as _random_draft, restore as _restore

pytestmark = pytest.mark.gpu

def _steps(r, n, logits=None):
    toks = []
    for _ in range(n):
        r.step()
        toks.append(r.tokens.clone())
        if logits is not None:
            logits.append(torch.matmul(r.normed, r.lm_head.t()).cpu().numpy())
    torch.cuda.synchronize()
    return torch.stack(toks)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graphed", "eager"])
def test_default_parameters_are_greedy_bit_for_bit(use_graph):
    s, _ = _prefilled(True, use_graph)
    g, _ = _prefilled(False, use_graph)
    assert torch.equal(s.tokens, g.tokens)
    assert torch.equal(_steps(s, 4), _steps(g, 4))
    assert torch.equal(s.lengths, g.lengths)
    for ps, pg in zip(s.pools, g.pools):
        for a, b in zip(ps, pg):
            assert torch.equal(a, b)


def test_sampled_steps_are_reproducible_graph_equals_eager_tokens_are_kept():
    params = dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)
    a, _ = _prefilled(True, False, **params)
    b, _ = _prefilled(True, False, **params)
    c, _ = _prefilled(True, True, **params)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.tokens, c.tokens)
    logits = []
    ta, tb, tc = _steps(a, 8, logits), _steps(b, 8), _steps(c, 8)
    assert torch.equal(ta, tb), "two runners from one seed differ"
    assert torch.equal(ta, tc), "the captured step differs from the eager one"
    ta = ta.cpu().numpy()
    kept_sizes = []
    for step in range(8):
        for row in range(B):
            o = sc.oracle_row(logits[step][row], 0.8, 50, 0.9)
            assert not o.greedy and o.kept[ta[step, row]], (step, row)
            kept_sizes.append(int(o.kept.sum()))
    assert max(kept_sizes) > 1
    # the parameters reach the CAPTURED step without a new capture, and so does the seed
    for r in (a, c):
        r.set_sampling(temperature=2.5, top_k=0, top_p=1.0, seed=2)
    graph = c.graph
    t2a, t2c = _steps(a, 8), _steps(c, 8)
    assert c.graph is graph and torch.equal(t2a, t2c)
    d, _ = _prefilled(True, False, **params)
    _steps(d, 8)
    d.set_sampling(temperature=2.5, top_k=0, top_p=1.0, seed=3)
    assert not torch.equal(_steps(d, 8), t2a), "another seed drew the same 24 tokens at T = 2.5"


def test_sampled_verify_at_temperature_zero_is_the_greedy_verify():
    s, _ = _prefilled(True)
    g, _ = _prefilled(False)
    draft = _random_draft(g, 9)
    pred_g, m_g = g.verify(draft)
    # make the first drafted tokens right so that some are accepted
    draft2 = torch.cat([draft[:, :1], pred_g[:, :2], draft[:, 3:]], dim=1)
    for r in (s, g):
        _restore(r, (torch.full_like(r.lengths, L), draft[:, 0]))
    pred_g, m_g = g.verify(draft2)
    pred_s, m_s = s.verify(draft2)
    assert int(m_g.max()) > 1
    assert torch.equal(m_s, m_g) and torch.equal(pred_s, pred_g)
    assert torch.equal(s.lengths, g.lengths) and torch.equal(s.tokens, g.tokens)
    with pytest.raises(RuntimeError, match="sampling=True"):
        g.verify(draft2, sampled=True)


def test_sampled_verify_keeps_the_state_and_rolls_back():
    """Draft = the runner's own next three sampled tokens.  verify() grows lengths by m and leaves drawn[b, m - 1] pending; behind a
    rolled-back call (lengths / tokens restored, generator reseeded) four steps give the plain run's tokens and hidden state."""
    r, state = _prefilled(True, temperature=0.8, top_k=50, top_p=0.9)
    r.set_sampling(seed=4)
    toks = _steps(r, 4)
    x_plain = r.x.clone()
    _restore(r, state)
    r.set_sampling(seed=4)
    toks_again = _steps(r, 4)
    plain_runs_identical = torch.equal(r.x.view(torch.int16), x_plain.view(torch.int16))
    assert torch.equal(toks, toks_again)
    _restore(r, state)
    draft = torch.cat([state[1].view(B, 1), toks[:3].t()], dim=1).contiguous()
    drawn, m = r.verify(draft)
    torch.cuda.synchronize()
    assert drawn.shape == (B, N) and m.shape == (B,) and int(m.min()) >= 1 and int(m.max()) <= N
    assert torch.equal(r.lengths, state[0] + m.to(torch.int32))
    assert torch.equal(r.tokens, drawn.gather(1, (m - 1).view(B, 1)).squeeze(1))
    rejected = m < N
    wrong = drawn.gather(1, (m - 1).view(B, 1)).squeeze(1) == draft.gather(1, m.clamp(max=N - 1).view(B, 1)).squeeze(1)
    assert not bool((rejected & wrong).any()), "a rejected token was drawn again"
    _restore(r, state)
    r.set_sampling(seed=4)
    toks_b = _steps(r, 4)
    assert torch.equal(toks_b, toks)
    if plain_runs_identical:
        assert torch.equal(r.x.view(torch.int16), x_plain.view(torch.int16))


def test_a_filtered_out_draft_is_rejected_whatever_u_acc_is():
    r, state = _prefilled(True, temperature=1.0, top_k=2, top_p=1.0, seed=4)
    draft = _random_draft(r, 21)
    zeros = torch.zeros((B, N), dtype=torch.float32, device=r.device)
    u_draw = torch.full((B, N), 0.25, dtype=torch.float32, device=r.device)
    drawn, m = r.verify(draft, uniforms=(u_draw, zeros))
    from omniserve_amd.backend import layernorm_ops
    x = r._prefill_bufs["x"][: B * N]
    normed = torch.empty_like(x)
    layernorm_ops.rms_norm(normed, x, r.final_norm, r.cfg.eps, False)
    logits = torch.matmul(normed, r.lm_head.t()).view(B, N, -1).cpu().numpy()
    for b in range(B):
        o = sc.oracle_row(logits[b, 0], 1.0, 2, 1.0)
        assert not o.kept[int(draft[b, 1])], "the random draft hit the top two: pick another seed"
        assert o.kept[int(drawn[b, 0])]
    assert m.tolist() == [1] * B
    assert torch.equal(r.lengths, state[0] + 1) and torch.equal(r.tokens, drawn[:, 0])


def test_verify_tree_on_a_sampling_runner_is_a_named_error():
    r, _ = _prefilled(True)
    tokens = torch.cat([r.tokens.view(B, 1), torch.zeros((B, 2), dtype=torch.int64, device=r.device)], dim=1)
    with pytest.raises(NotImplementedError, match="sampling runner"):
        r.verify_tree(tokens, [-1, 0, 0])


def test_lserve_runner_has_the_same_switch():
    """LServeDecodeRunner(sampling=True): greedy until set_sampling(), then reproducible draws that leave the arg-max path."""
    from omniserve_amd.lserve_runtime import LServeDecodeRunner
    from omniserve_amd.runtime import LlamaConfig

    def run(sampling, params=None, steps=5):
        r = LServeDecodeRunner(LlamaConfig.tiny(), batch=2, context=700, max_new=16, device=torch.device("cuda:0"), seed=11,
                               sink=64, local=128, budget_tokens=256, selector_interval=4, use_graph=True, sampling=sampling)
        if params:
            r.set_sampling(**params)
        seq = []
        for _ in range(steps):
            r.step()
            seq.append(r.tokens.clone())
        torch.cuda.synchronize()
        return torch.stack(seq)

    greedy = run(False)
    assert torch.equal(run(True), greedy)
    hot = dict(temperature=2.5, top_k=0, top_p=1.0, seed=3)
    a, b = run(True, hot), run(True, hot)
    assert torch.equal(a, b) and not torch.equal(a, greedy)
    assert int(a.min()) >= 0 and int(a.max()) < 512
