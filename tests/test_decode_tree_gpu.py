"""Tree form of the multi-token decode attention (omni_decode_attention_tree_kv4: 0 - 32 new tokens per sequence, each seeing the
past and the fresh keys its mask word names) on the GPU.  Bar: the project's assert_attention_close, 1e-3 per head against the f64
masked softmax over dequantised past + visible fresh keys (tests/tree_verify_cases.py); every raw call writes to a caller-owned
`out` with a sentinel band behind it and gets a workspace of exactly the advertised size."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import paged_prefill_cases as pc
from tests import tree_verify_cases as tc
from tests.util import GpuPagedKV, assert_attention_close, to_dev

pytestmark = pytest.mark.gpu

D = pc.D
SENTINEL = 0x7BCD      # fp16 bits of the band behind `out`


@contextlib.contextmanager
def _forced_splits(n):
    from omniserve_amd import _lib
    _lib.lib().omni_decode_attention_multi_kv4_set_split_override(n)      # (applies to both forms)
    try:
        yield
    finally:
        _lib.lib().omni_decode_attention_multi_kv4_set_split_override(0)


def _run_raw(case, gk, qkv_rot, mask, nsplit=0, strided=True, max_q=tc.MAX_Q, chain_entry=False):
    """The C entry (chain_entry: omni_decode_attention_multi_kv4 on the same inputs, without the mask) -> fp16 [T, Hq, D] (numpy)."""
    from omniserve_amd import _lib
    Hq, Hk, T = case.Hq, case.Hk, case.T
    qkv_d = to_dev(qkv_rot)
    q = qkv_d[:, : Hq * D].view(T, Hq, D)
    k = qkv_d[:, Hq * D:(Hq + Hk) * D].view(T, Hk, D)
    v = qkv_d[:, (Hq + Hk) * D:].view(T, Hk, D)
    if not strided:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    band = 4 * Hq * D
    out = torch.full((T * Hq * D + band,), SENTINEL, dtype=torch.int16, device=qkv_d.device)
    max_past = int(case.pasts.max())
    h = _lib.lib()
    size = h.omni_decode_attention_multi_kv4_workspace_bytes if chain_entry else h.omni_decode_attention_tree_kv4_workspace_bytes
    ws = torch.empty(size(case.B, Hq, max_q, max_past), dtype=torch.uint8, device=qkv_d.device)
    cu_d, past_d = to_dev(case.cu), to_dev(case.pasts)      # (named: they must outlive the launch)
    mask_d = to_dev(np.ascontiguousarray(mask, np.uint32).view(np.int32))
    assert mask_d.shape == (T,)
    head = (out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0), cu_d.data_ptr(),
            past_d.data_ptr())
    tail = (gk.table.data_ptr(), case.B, gk.table.shape[-1], case.tpb, max_q, Hq, Hk, D, max_past, ws.data_ptr(), ws.numel(),
            _lib.current_stream())
    with _forced_splits(nsplit):
        if chain_entry:
            rc = h.omni_decode_attention_multi_kv4(*head, *tail)
        else:
            rc = h.omni_decode_attention_tree_kv4(*head, mask_d.data_ptr(), *tail)
        torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy()
    assert (host[T * Hq * D:] == SENTINEL).all(), "the band behind out was written"
    return host[: T * Hq * D].view(np.float16).reshape(T, Hq, D)


@functools.lru_cache(maxsize=None)
def _family(name):
    case = tc.family(name)
    return case, tc.case_expected(case)      # (computed once, never modified)


@pytest.mark.parametrize("name", sorted(tc.FAMILIES))
@pytest.mark.parametrize("nsplit", tc.SPLITS)
@pytest.mark.parametrize("strided", [True, False])
def test_tree_attention_grid(name, nsplit, strided):
    """12 sequences per family -- pasts {0, 1, 63, 64, 65, 200} and n {1, 2, 8, 9, 17, 32} twice each, a different tree per
    sequence (chain, star, binary, two chains, random) -- over tokens_per_block 16 / 64 and GQA ratios 1 / 4 / 7 / 8 (n = 32 at
    ratios 8 and 7: 256 and 224 rows per kv head, two row groups, the second ragged); the planner's split count and 1, 2, 3, 7
    forced splits; q / k / v as views of the qkv buffer and as contiguous tensors."""
    case, want = _family(name)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=nsplit, strided=strided)
    assert_attention_close(got, want, "tree attention %s, %d splits (%s)" % (name, nsplit, "views" if strided else "contiguous"))


@functools.lru_cache(maxsize=None)
def _mixed():
    case = tc.mixed()
    return case, tc.case_expected(case)


@pytest.mark.parametrize("nsplit", [0, 3])
def test_tree_attention_mixed_batch_with_empty_sequences(nsplit):
    """(past, n) = (0, 32), (200, 0), (65, 3), (0, 0), (130, 1), (17, 9), (0, 1) in one batch, shuffled non-contiguous tables."""
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=nsplit)
    assert_attention_close(got, want, "tree attention, mixed batch, %d splits" % nsplit)


def test_a_row_that_sees_nothing_is_zeros():
    """Mask words 0 at past 0: exact zeros, with and without the split partials; the other sequences are untouched by it."""
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    mask = case.mask.copy()
    a, e = int(case.cu[0]), int(case.cu[1])      # (0, 32): no past
    mask[a:e] = 0
    for nsplit in (0, 3):
        got = _run_raw(case, gk, case.qkv_rot, mask, nsplit=nsplit)
        assert not got[a:e].view(np.uint16).any()
        assert_attention_close(got[e:], want[e:], "tree attention behind the blind rows, %d splits" % nsplit)


@pytest.mark.parametrize("nsplit", [0, 2, 3, 7])
def test_chain_masks_give_the_chain_entry_its_bits(nsplit):
    """Chain trees, n <= 8: bit-identical to omni_decode_attention_multi_kv4 on the same inputs (the same kernel body: only the
    fresh tile's mask test differs, and it passes the same keys)."""
    case = tc.chain_case()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    want = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=nsplit, max_q=8, chain_entry=True)
    got = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=nsplit, max_q=8)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert np.abs(got.astype(np.float32)).max() > 0


@pytest.mark.parametrize("nsplit", [0, 3])
def test_mask_bits_at_or_above_len_q_change_nothing(nsplit):
    """The fresh tile's rows >= len_q repeat the last key: a set bit there must not count it again."""
    case, _ = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    high = case.mask.copy()
    for b in range(case.B):
        n = int(case.lens[b])
        high[case.cu[b]:case.cu[b + 1]] |= np.uint32((0xFFFFFFFF << n) & 0xFFFFFFFF)
    assert (high != case.mask).sum() >= case.T - 32
    a = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=nsplit)
    b = _run_raw(case, gk, case.qkv_rot, high, nsplit=nsplit)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


@functools.lru_cache(maxsize=None)
def _needles():
    nb = tc.SiblingNeedles()
    return nb, nb.expected()[0]


@pytest.mark.parametrize("nsplit", [3, 7])
def test_sibling_needles(nsplit):
    """154 sequences over one shared table, star tree of 4 nodes, sequence b aimed at key b (150 page keys, 4 fresh ones): node
    i's rows of sequence 150 + j, j != i, j >= 1, aim at a fresh key they must NOT see -- a leak moves the row by about its whole
    value; the rows of sequence 150 aim at the root, which every node must see."""
    nb, want = _needles()
    gk = GpuPagedKV(nb.kc, nb.vc, nb.kidx, nb.vidx)
    got = _run_raw(nb, gk, nb.qkv_rot, nb.mask, nsplit=nsplit, max_q=nb.n)
    assert_attention_close(got, want, "sibling needles, %d splits" % nsplit)
    g, w = got.reshape(nb.B, nb.n, nb.Hq, D), want.reshape(nb.B, nb.n, nb.Hq, D)
    assert_attention_close(g[nb.past + 2, 1], w[nb.past + 2, 1], "node 1 aimed at its sibling 2")
    assert_attention_close(g[nb.past + 1, 3], w[nb.past + 1, 3], "node 3 aimed at its sibling 1")
    assert_attention_close(g[nb.past, 3], w[nb.past, 3], "node 3 aimed at the root")


@pytest.mark.parametrize("nsplit", [0, 3])
def test_tree_attention_never_reads_slots_at_or_behind_past(nsplit):
    """Every page slot at a position >= past holds data 0xFF with scale = zero = NaN: the output is finite and within the bar."""
    case, want = _mixed()
    kc_p, vc_p = pc.poison_from_past(case, case.kc, case.kidx), pc.poison_from_past(case, case.vc, case.vidx)
    got = _run_raw(case, GpuPagedKV(kc_p, vc_p, case.kidx, case.vidx), case.qkv_rot, case.mask, nsplit=nsplit)
    assert np.isfinite(got.astype(np.float32)).all()
    assert_attention_close(got, want, "tree attention, poisoned slots >= past")
    clean = _run_raw(case, GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx), case.qkv_rot, case.mask, nsplit=nsplit)
    assert np.array_equal(got.view(np.uint16), clean.view(np.uint16))


def test_two_runs_give_the_same_bits():
    case, _ = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    a = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=3)
    b = _run_raw(case, gk, case.qkv_rot, case.mask, nsplit=3)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def test_mirror_and_refused_configurations():
    from omniserve_amd.backend import fused_ext
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    q, k, v = case.split(to_dev(case.qkv_rot))
    cu, past = to_dev(case.cu), to_dev(case.pasts)
    mask = to_dev(case.mask.view(np.int32))
    max_past = int(case.pasts.max())
    got = fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask, gk.table, case.tpb, 32, max_past)
    torch.cuda.synchronize()
    assert_attention_close(got.cpu().numpy(), want, "tree attention (mirror) vs oracle")
    m, d = fused_ext.tree_masks(to_dev(case.parents[0]))      # on the device
    assert np.array_equal(m.cpu().numpy().view(np.uint32), case.mask[:32]) and np.array_equal(d.cpu().numpy(), case.depth[:32])
    with pytest.raises(fused_ext.DecodeTreeTooManyTokens):
        fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask, gk.table, case.tpb, 33, max_past)
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask[:-1], gk.table, case.tpb, 32, max_past)      # mask length
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask.long(), gk.table, case.tpb, 32, max_past)    # mask dtype
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask.cpu(), gk.table, case.tpb, 32, max_past)     # mask on the host
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask, gk.table, 24, 32, max_past)                 # tokens_per_block
