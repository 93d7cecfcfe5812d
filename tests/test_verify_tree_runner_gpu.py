"""DecodeRunner.verify_tree: the tree verify step through the runner (LlamaConfig.tiny, B = 3, prompt 150), against verify() and
step() from the same restored state."""
import pytest
import torch

from runner_cases import (B, N, four_steps as _four_steps, pools as _pools, prefilled as _prefilled,
                          random_draft as _random_draft, rel_l2 as _rel_l2, restore as _restore)

pytestmark = pytest.mark.gpu

# The bar of tests/test_verify_runner_gpu.py for "the same mathematics through another kernel / another summation order":
# final-norm hidden states, relative L2 <= 4 x the noise floor that DESIGN.md section 4.5a pins.
NOISE_FLOOR = 0.0517
FACTOR = 4.0


def _layer0_rows(r, pools, past, count):
    """Codes, scale and zero point of layer 0's K and V rows at positions [past[b], past[b] + count) of every sequence and kv head,
    read from `pools` (the runner's, or a clone of them) through the runner's block table -> uint8 [B, 2, count, heads, 68]."""
    tpb, hk = r.tpb, r.kl
    data = hk * tpb * 64
    out = torch.empty((B, 2, count, hk, 68), dtype=torch.uint8, device=r.device)
    for b in range(B):
        for kv in range(2):
            for j in range(count):
                pos = int(past[b]) + j
                page = (int(r.block_tables[0][b, kv, pos // tpb]) - r.pools[0][kv].data_ptr()) // r.page_bytes
                for h in range(hk):
                    row = h * tpb + pos % tpb
                    pg = pools[kv][page]
                    out[b, kv, j, h] = torch.cat([pg[row * 64:(row + 1) * 64], pg[data + 2 * row: data + 2 * row + 2],
                                                  pg[data + 2 * hk * tpb + 2 * row: data + 2 * hk * tpb + 2 * row + 2]])
    return out


def _accepted_chain(r, state):
    """A draft that verify() accepts whole (rebuilt from its own predictions, as tests/test_verify_runner_gpu.py does); the runner
    is left behind that fully accepting verify().  -> (draft, pred)."""
    draft = _random_draft(r, 9)
    for _ in range(N):
        _restore(r, state)
        pred, m = r.verify(draft)
        if int(m.min()) == N:
            return draft, pred
        draft = torch.cat([state[1].view(B, 1), pred[:, : N - 1]], dim=1)
    raise AssertionError("verify() did not converge on its own predictions")


def test_chain_tree_equals_verify():
    """verify_tree(draft, chain parents) and verify(draft) from the same restored state: pred, m, lengths, tokens and x equal, and
    every layer's K / V pools byte for byte (chain masks are the chain entry's bits, depth = slot, the path is in place)."""
    r, state = _prefilled()
    draft = _random_draft(r, 9)
    pred_v, m_v = r.verify(draft)
    torch.cuda.synchronize()
    after_v = (r.lengths.clone(), r.tokens.clone(), r.x.clone(), r.normed.clone(), _pools(r))
    _restore(r, state)
    pred_t, path, m_t = r.verify_tree(draft, list(range(-1, N - 1)))
    torch.cuda.synchronize()
    assert torch.equal(pred_t, pred_v) and torch.equal(m_t, m_v)
    assert path.shape == (B, N) and path.dtype == torch.int64
    for b in range(B):
        assert path[b].tolist() == list(range(int(m_t[b]))) + [-1] * (N - int(m_t[b]))
    assert torch.equal(r.lengths, after_v[0]) and torch.equal(r.tokens, after_v[1])
    assert torch.equal(r.x.view(torch.int16), after_v[2].view(torch.int16))
    assert torch.equal(r.normed.view(torch.int16), after_v[3].view(torch.int16))
    for li, (layer, want) in enumerate(zip(r.pools, after_v[4])):
        for a, w in zip(layer, want):
            assert torch.equal(a, w), "layer %d pools differ" % li


def test_a_true_path_among_decoys():
    """g1 .. g3 from a fully accepting chain verify(); the 7-node tree root -> {decoy, g1}, g1 -> {decoy, g2}, g2 -> {g3, decoy}:
    path [0, 2, 4, 5], m = 4.  Layer 0's rows at [past, past + 4) are byte-identical to the chain run's (layer-0 K / V depend on
    token and position only: this pins the RoPE depth and the compaction through the runner), and the last accepted node's
    final-norm hidden state agrees with the chain run's within 4 x the section 4.5a floor = 0.207.  Measured on the MI355X:
    DESIGN.md section 4.5c."""
    r, state = _prefilled()
    draft, pred_c = _accepted_chain(r, state)
    torch.cuda.synchronize()
    chain = (r.lengths.clone(), r.tokens.clone(), r.normed.clone(), _pools(r))
    g = draft[:, 1:]                                         # g1 .. g3 [B, 3]
    decoy = (pred_c[:, :3] + 1) % r.cfg.vocab                # never what the model says at that node
    tokens = torch.stack([draft[:, 0], decoy[:, 0], g[:, 0], decoy[:, 1], g[:, 1], g[:, 2], decoy[:, 2]], dim=1)
    parents = [-1, 0, 0, 2, 2, 4, 4]
    _restore(r, state)
    pred, path, m = r.verify_tree(tokens, parents)
    torch.cuda.synchronize()
    assert m.tolist() == [4] * B
    assert path.tolist() == [[0, 2, 4, 5, -1, -1, -1]] * B
    assert torch.equal(r.lengths, chain[0])
    assert torch.equal(pred[:, [0, 2, 4]], pred_c[:, :3])
    rows_t, rows_c = _layer0_rows(r, r.pools[0], state[0], 4), _layer0_rows(r, chain[3][0], state[0], 4)
    assert torch.equal(rows_t, rows_c), "layer 0 rows at [past, past + 4) differ from the chain run's"
    dist = _rel_l2(r.normed, chain[2])
    msg = "final-norm hidden state of the last accepted node, rel L2: tree (7 nodes) vs chain verify(4) %.3g; floor %.3g, bar %.3g" % (
        dist, NOISE_FLOOR, FACTOR * NOISE_FLOOR)
    print(msg)
    assert dist <= FACTOR * NOISE_FLOOR, msg
    assert torch.equal(r.tokens, chain[1]) or dist > 0       # (the next token may only differ where the hidden states do)


def test_all_drafts_wrong():
    """A star of 6 wrong children: m = 1, lengths + 1; four plain step()s afterwards are bit-identical between two runs from that
    state, and the hidden state agrees with the plain step() path (step() in place of the rejected tree) within the bar."""
    r, state = _prefilled()
    r.step()
    torch.cuda.synchronize()
    plain = (r.lengths.clone(), r.tokens.clone(), r.normed.clone())
    toks_p, _ = _four_steps(r)
    _restore(r, state)
    # children that cannot match: pred[:, 0] is the plain step's token
    kids = torch.stack([(plain[1] + 1 + j) % r.cfg.vocab for j in range(6)], dim=1)
    tokens = torch.cat([state[1].view(B, 1), kids], dim=1)
    pred, path, m = r.verify_tree(tokens, [-1, 0, 0, 0, 0, 0, 0])
    torch.cuda.synchronize()
    assert m.tolist() == [1] * B and path[:, 0].tolist() == [0] * B and bool((path[:, 1:] == -1).all())
    assert torch.equal(r.lengths, state[0] + 1) and torch.equal(r.lengths, plain[0])
    assert torch.equal(r.tokens, pred[:, 0])
    dist = _rel_l2(r.normed, plain[2])
    msg = "final-norm hidden state behind a rejected tree vs a plain step(), rel L2 %.3g; floor %.3g, bar %.3g" % (
        dist, NOISE_FLOOR, FACTOR * NOISE_FLOOR)
    print(msg)
    assert dist <= FACTOR * NOISE_FLOOR, msg
    after = (r.lengths.clone(), r.tokens.clone())
    toks_a, x_a = _four_steps(r)
    _restore(r, after)
    toks_b, x_b = _four_steps(r)
    assert torch.equal(toks_a, toks_b) and torch.equal(x_a.view(torch.int16), x_b.view(torch.int16))
    if torch.equal(after[1], plain[1]):
        print("tokens behind the rejected tree follow the plain path: %s" % torch.equal(toks_a, toks_p))


def test_errors():
    r, _ = _prefilled()
    draft = _random_draft(r, 9)
    chain = list(range(-1, N - 1))
    bad = draft.clone()
    bad[0, 0] = (bad[0, 0] + 1) % r.cfg.vocab
    with pytest.raises(ValueError):
        r.verify_tree(bad, chain)                                                  # column 0 is not the pending token
    wide = torch.cat([r.tokens.view(B, 1), torch.zeros((B, 32), dtype=torch.int64, device=r.device)], dim=1)
    with pytest.raises(ValueError):
        r.verify_tree(wide, [-1] + list(range(32)))                                # n = 33
    for parents in ([-1, 0, 2, 1], [-1, 1, 0, 0], [0, 0, 1, 2], [-1, 0, 1], [-1, 0, 1, 3]):
        with pytest.raises(ValueError):
            r.verify_tree(draft, parents)
    lengths = r.lengths.clone()
    r.verify_tree(draft, torch.tensor(chain))                                      # (and a tensor of parents is fine)
    torch.cuda.synchronize()
    assert bool((r.lengths > lengths).all())
