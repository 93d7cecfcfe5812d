"""DecodeRunner.extend and prefill(chunk=...): chunked / multi-turn prefill through the runner (LlamaConfig.tiny, B = 3, L = 150)."""
import pytest
import torch

from runner_cases import B, L, pools as _pools, prompt as _prompt, rel_l2 as _rel_l2, runner as _runner

pytestmark = pytest.mark.gpu

# Relative L2 distance of the final-norm hidden states between two summation orders of the EXISTING decode attention kernel
# (path A below with omni_kv4_decode_set_split_override(1) and (4)), measured on the MI355X on the parent commit: the
# noise floor of "the same mathematics through another kernel".  See test_one_token_through_decode_and_through_extend.
NOISE_FLOOR = 0.0517
FACTOR = 4.0


def _same_pools(a, b):
    return all(torch.equal(pa, pb) for la, lb in zip(a, b) for pa, pb in zip(la, lb))


def test_one_chunk_is_the_whole_prompt_pass_bit_for_bit():
    r = _runner()
    prompt = _prompt(r)
    r.prefill(L, prompt.reshape(-1))
    want = (r.x.clone(), r.tokens.clone(), _pools(r))
    r2 = _runner()
    r2.prefill(L, prompt.reshape(-1), chunk=200)
    torch.cuda.synchronize()
    assert torch.equal(r2.x.view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(r2.tokens, want[1])
    assert _same_pools(_pools(r2), want[2])
    assert r2.lengths.tolist() == [L] * B


def test_chunked_prefill_puts_every_token_where_the_whole_prompt_pass_does():
    """Layer 0's keys and values depend on no attention: its K and V pools after prefill(L, chunk=64) (chunks of 64, 64, 22 at
    pasts 0, 64, 128) are byte-identical to prefill(L)'s -- positions, RoPE rows and page slots through the runner."""
    r = _runner()
    prompt = _prompt(r)
    r.prefill(L, prompt.reshape(-1))
    want = _pools(r)[0]
    r2 = _runner()
    r2.prefill(L, prompt.reshape(-1), chunk=64)
    torch.cuda.synchronize()
    assert r2._prefill_bufs["T"] == B * 64                  # activation buffers sized by the chunk
    for a, b in zip(_pools(r2)[0], want):
        assert torch.equal(a, b)
    assert r2.lengths.tolist() == [L] * B
    assert torch.isfinite(r2.x.float()).all() and torch.isfinite(r2.normed.float()).all()
    assert int(r2.tokens.min()) >= 0 and int(r2.tokens.max()) < r2.cfg.vocab
    r2.step()                                               # the pages are readable by the decode path
    torch.cuda.synchronize()
    assert torch.isfinite(r2.x.float()).all() and r2.lengths.tolist() == [L + 1] * B


def _path_a(prompt, nsplit=0):
    """prefill(L - 1), then the prompt's last token through one eager DECODE step."""
    from omniserve_amd import _lib
    r = _runner()
    r.prefill(L - 1, prompt[:, : L - 1].reshape(-1))
    shared = _pools(r)
    r.tokens.copy_(prompt[:, L - 1])
    _lib.lib().omni_kv4_decode_set_split_override(nsplit)
    try:
        r.step()
        torch.cuda.synchronize()
    finally:
        _lib.lib().omni_kv4_decode_set_split_override(0)
    return r, shared


def test_one_token_through_decode_and_through_extend():
    """The same mathematics through two kernels.  (A) prefill(L - 1), the prompt's last token as one eager decode step;
    (B) prefill(L - 1), then extend(1) with that token.  Both see 149 quantised past tokens and the fresh current one; the pools
    after the shared first part are byte-identical; what remains is the order of the sums in S and in P.V.
    Bar: 4 x the noise floor, the floor being A against itself with the decode kernel forced to 1 and to 4 KV splits (two
    summation orders of the existing kernel); 4 x leaves room for two such changes.
    Measured on the MI355X: floor NOISE_FLOOR (above), B vs A printed below and recorded in DESIGN.md section 4.5a."""
    r0 = _runner()
    prompt = _prompt(r0)
    a1, shared_a = _path_a(prompt, 1)
    a4, _ = _path_a(prompt, 4)
    floor_now = _rel_l2(a1.normed, a4.normed)
    a, _ = _path_a(prompt, 0)
    b = _runner()
    b.prefill(L - 1, prompt[:, : L - 1].reshape(-1))
    assert _same_pools(_pools(b), shared_a)
    b.extend(1, prompt[:, L - 1])
    torch.cuda.synchronize()
    assert b.lengths.tolist() == [L] * B and a.lengths.tolist() == [L] * B
    for pa, pb in zip(_pools(a)[0], _pools(b)[0]):      # layer 0: the appended token's bytes do not depend on the attention
        assert torch.equal(pa, pb)
    dist = _rel_l2(b.normed, a.normed)
    msg = "final-norm hidden states, rel L2: extend(1) vs decode step %.3g; floor (1 vs 4 splits) now %.3g, pinned %.3g, bar %.3g" % (
        dist, floor_now, NOISE_FLOOR, FACTOR * NOISE_FLOOR)
    print(msg)
    assert dist <= FACTOR * NOISE_FLOOR, msg


def test_extend_appends_at_per_sequence_lengths():
    """A further turn behind conversations of different lengths (70, 33 and 128 tokens in the pages): extend(20) rotates and
    stores sequence b's tokens at positions lengths[b] + i.  Layer 0's keys and values are a function of (token, position)
    alone, so its pools must equal those of a whole-prompt pass over prompts that carry the new tokens at those positions."""
    n_new, pasts = 20, [70, 33, 128]
    r = _runner()
    prompt = _prompt(r, 148)
    new = _prompt(r, 148)[:, :n_new].flip(0).contiguous()
    r.prefill(148, prompt.reshape(-1))
    r.lengths.copy_(torch.tensor(pasts, dtype=torch.int32, device=r.device))      # the conversations so far
    r.extend(n_new, new.reshape(-1))
    torch.cuda.synchronize()
    assert r.lengths.tolist() == [p + n_new for p in pasts]
    assert torch.isfinite(r.normed.float()).all()
    ref_tokens = prompt.clone()
    for i, p in enumerate(pasts):
        ref_tokens[i, p:p + n_new] = new[i]
    rr = _runner()
    rr.prefill(148, ref_tokens.reshape(-1))
    torch.cuda.synchronize()
    for a, b in zip(r.pools[0], rr.pools[0]):
        assert torch.equal(a, b)


def test_extend_beyond_the_pools_raises():
    r = _runner()
    r.prefill(L, _prompt(r).reshape(-1))
    room = r.max_context - L - 1
    with pytest.raises(ValueError):
        r.extend(room + 1)
    r.extend(room)
    torch.cuda.synchronize()
    assert r.lengths.tolist() == [L + room] * B
    with pytest.raises(ValueError):
        r.extend(1)


def _first_rows(r, count):
    """The bytes of positions [0, count) of every layer's K and V pages (count <= one page): codes, scales and zero points."""
    hk, tpb = r.kl, r.tpb
    data = hk * tpb * 64
    out = []
    for table, layer in zip(r.block_tables, r.pools):
        for kv, pool in enumerate(layer):
            pages = pool[(table[:, kv, 0] - pool.data_ptr()) // r.page_bytes]
            out.append(pages[:, :data].view(B, hk, tpb, 64)[:, :, :count].clone())
            out.append(pages[:, data:].view(B, 2, hk, tpb, 2)[:, :, :, :count].clone())
    return out


def test_prefill_into_larger_buffers_is_a_fresh_runners_prefill():
    """The context stage's buffers only grow: prefill(40) behind prefill(150) runs in the head of the 150-token buffers.  x, normed,
    tokens, lengths and the page bytes of positions [0, 40) equal a fresh runner's prefill(40), whose buffers hold exactly its own
    rows, bit for bit."""
    r = _runner()
    r.prefill(L, _prompt(r).reshape(-1))
    prompt40 = _prompt(r, 40)
    r.prefill(40, prompt40.reshape(-1))
    assert r._prefill_bufs["T"] == B * L
    f = _runner()
    f.prefill(40, prompt40.reshape(-1))
    torch.cuda.synchronize()
    assert f._prefill_bufs["T"] == B * 40
    assert torch.equal(r.x.view(torch.int16), f.x.view(torch.int16))
    assert torch.equal(r.normed.view(torch.int16), f.normed.view(torch.int16))
    assert torch.equal(r.tokens, f.tokens)
    assert r.lengths.tolist() == [40] * B and f.lengths.tolist() == [40] * B
    for a, b in zip(_first_rows(r, 40), _first_rows(f, 40)):
        assert torch.equal(a, b)
