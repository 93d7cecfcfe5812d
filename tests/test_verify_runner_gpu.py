"""DecodeRunner.verify: the multi-token decode step through the runner (LlamaConfig.tiny, B = 3, prompt 150, n = 4 positions)."""
import pytest
import torch

from runner_cases import (B, N, four_steps as _four_steps, prefilled as _prefilled, random_draft as _random_draft,
                          rel_l2 as _rel_l2, restore as _restore)

pytestmark = pytest.mark.gpu

# The noise floor of "the same mathematics through another kernel" that tests/test_paged_prefill_runner_gpu.py pins (the parent's
# decode kernel forced to 1 against 4 KV splits, final-norm hidden states, relative L2: DESIGN.md section 4.5a), and its factor:
# two changed summation orders, S and P.V.
NOISE_FLOOR = 0.0517
FACTOR = 4.0


def test_verify_converges_on_its_own_predictions_and_matches_extend():
    """(a) verify on a random continuation, lengths / tokens restored after each call and the draft rebuilt from the returned
    pred: pred[:, j] never changes once the draft's columns <= j are fixed (causality, by exact token equality), after at most
    n - 1 rebuilt drafts every position is accepted, and then lengths grew by n and tokens == pred[:, n - 1].
    (c) the final-norm hidden state the fully accepted verify leaves against extend(n, the same tokens) from the same state:
    relative L2 within 4 x the project's two-kernel noise floor.  Measured on the MI355X: 0 (floor 0.0517, bar 0.207; at past
    150 the planner keeps one split, which runs the paged kernel's tile sequence): DESIGN.md section 4.5b."""
    from omniserve_amd.runtime import accept_lengths
    r, state = _prefilled()
    draft = _random_draft(r, 9)
    pred, m = r.verify(draft)
    assert pred.shape == (B, N) and pred.dtype == torch.int64 and m.shape == (B,)
    assert torch.equal(m, accept_lengths(draft, pred))
    assert torch.equal(r.lengths, state[0] + m.to(torch.int32))
    assert torch.equal(r.tokens, pred.gather(1, (m - 1).view(B, 1)).squeeze(1))
    rounds = 0
    while int(m.min()) < N:
        assert rounds < N - 1, "no convergence: %s" % m.tolist()
        rounds += 1
        _restore(r, state)
        prev = pred
        draft = torch.cat([state[1].view(B, 1), prev[:, : N - 1]], dim=1)
        pred, m = r.verify(draft)
        assert torch.equal(pred[:, :rounds], prev[:, :rounds]), "pred changed under fixed draft columns (round %d)" % rounds
        assert int(m.min()) >= min(rounds + 1, N)
    torch.cuda.synchronize()
    assert torch.equal(r.lengths, state[0] + N)
    assert torch.equal(r.tokens, pred[:, N - 1])
    e, _ = _prefilled()
    e.extend(N, draft.reshape(-1))
    torch.cuda.synchronize()
    assert torch.equal(e.lengths, r.lengths)
    dist = _rel_l2(r.normed, e.normed)
    msg = "final-norm hidden states, rel L2: verify(%d) vs extend(%d) %.3g; floor %.3g, bar %.3g" % (
        N, N, dist, NOISE_FLOOR, FACTOR * NOISE_FLOOR)
    print(msg)
    assert dist <= FACTOR * NOISE_FLOOR, msg


def test_verify_column_zero_must_be_the_pending_token():
    r, _ = _prefilled()
    draft = _random_draft(r, 9)
    draft[0, 0] = (draft[0, 0] + 1) % r.cfg.vocab
    with pytest.raises(ValueError):
        r.verify(draft)
    with pytest.raises(ValueError):
        r.verify(torch.zeros((B, 9), dtype=torch.int64, device=r.device))


def test_rollback_is_harmless():
    """(b) From the state S after prefill: four eager steps; S again (lengths and tokens restored: the steps' page slots lie at
    positions >= lengths), verify on a random draft, S again, four eager steps.  The tokens are identical.  Two plain runs from
    S were bit-identical in their hidden state on the MI355X (checked first, below), so the hidden state after the run behind
    the rolled-back verify must be bit-identical too."""
    r, state = _prefilled()
    toks_a, x_a = _four_steps(r)
    _restore(r, state)
    toks_a2, x_a2 = _four_steps(r)
    plain_runs_identical = torch.equal(x_a.view(torch.int16), x_a2.view(torch.int16))
    print("two plain runs from S bit-identical: %s" % plain_runs_identical)
    assert torch.equal(toks_a, toks_a2)
    _restore(r, state)
    pred, m = r.verify(_random_draft(r, 13))
    assert int(m.max()) < N, "the random draft was accepted whole: pick another seed"
    _restore(r, state)
    toks_b, x_b = _four_steps(r)
    assert torch.equal(toks_b, toks_a)
    if plain_runs_identical:
        assert torch.equal(x_b.view(torch.int16), x_a.view(torch.int16))


def _all_rows_normed(r):
    """The final-norm hidden states of ALL B * n rows of the runner's last extend() / verify() (the rows' buffer outlives the call)."""
    from omniserve_amd.backend import layernorm_ops
    x = r._prefill_bufs["x"][: B * N]
    out = torch.empty_like(x)
    layernorm_ops.rms_norm(out, x, r.final_norm, r.cfg.eps, False)
    return out


def test_verify_through_the_split_and_merge_path_matches_extend():
    """At past 150 the planner keeps ONE split, which runs the paged kernel's tile sequence: check (c) above measures 0 and never
    reaches the split partials and the merge launch.  Here the same comparison with the split count forced to 3 (one 64-key tile
    of the past per split, the fresh keys in split 0, the merge launch behind), and over all B * n rows' final-norm hidden states,
    accepted or not -- every row is the model's state behind draft[b, :j + 1] on both sides, so the draft need not be accepted.
    Bar: 4 x the project's two-kernel noise floor, as above."""
    from omniserve_amd.backend import fused_ext
    r, _ = _prefilled()
    draft = _random_draft(r, 9)
    fused_ext.decode_attention_multi_kv4_set_split_override(3)
    try:
        r.verify(draft)
        torch.cuda.synchronize()
    finally:
        fused_ext.decode_attention_multi_kv4_set_split_override(0)
    rows_v = _all_rows_normed(r)
    e, _ = _prefilled()
    e.extend(N, draft.reshape(-1))
    rows_e = _all_rows_normed(e)
    torch.cuda.synchronize()
    assert not torch.equal(rows_v.view(torch.int16), rows_e.view(torch.int16)), "the forced split count changed nothing"
    for a, b in zip(r.pools[0], e.pools[0]):            # layer 0: the written keys / values do not depend on the attention
        assert torch.equal(a, b)
    dist = _rel_l2(rows_v, rows_e)
    msg = "final-norm hidden states of all rows, rel L2: verify(%d) under 3 forced splits vs extend(%d) %.3g; floor %.3g, bar %.3g" % (
        N, N, dist, NOISE_FLOOR, FACTOR * NOISE_FLOOR)
    print(msg)
    assert dist <= FACTOR * NOISE_FLOOR, msg
