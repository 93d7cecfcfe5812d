"""The prefill pair that continues from the KV4 page cache, on the GPU: the writer at an offset (omni_kv4_prefill_write_at:
byte-exact pages, tails and in-place RoPE against the oracle) and the attention over quantised past + fresh chunk
(omni_prefill_attention_paged_kv4: per head relative L2 and max error <= 1e-3 against the f64 oracle, the bar of
tests/test_prefill_attn_edges_gpu.py).  Expected values: tests/paged_prefill_cases.py."""
import functools

import numpy as np
import pytest
import torch

from tests import paged_prefill_cases as pc
from tests.util import GpuPagedKV, assert_attention_close, assert_f16_equal, to_dev

pytestmark = pytest.mark.gpu

D = pc.D
SENTINEL = 0x7BCD      # fp16 bits of the band behind `out`


# ---- writer ---------------------------------------------------------------------------------------------------------------
def _write_at(qkv_d, lens, pasts, table, Hq, Hk, tpb):
    import omniserve_backend.fused_attention_fine_grained_dense as fa
    from omniserve_amd.backend import fused_ext
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    max_len = max(int(np.max(lens)), 1)
    pad = fa.compute_padding_offsets(to_dev(cu), max_len, int(cu[-1]))
    fused_ext.kv4_prefill_write_at(qkv_d, to_dev(np.asarray(lens, np.int32)), to_dev(np.asarray(pasts, np.int32)), pad, table,
                                   Hq, Hk, max_len, tpb, int(np.max(np.asarray(pasts) + np.asarray(lens))), pc.ROPE_BASE)


PASTS = [0, 1, 15, 16, 63, 64, 65, 130]
LENS = [1, 17, 64, 70]


@pytest.mark.parametrize("tpb", [16, 64])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_writer_at_offset_is_byte_exact(tpb, shift):
    """Every past in {0, 1, 15, 16, 63, 64, 65, 130} with every len in {1, 17, 64, 70} (one mixed batch per shift), 8 / 2 heads,
    shuffled tables: pages, scale / zero tails and the rotated q / k in qkv are byte-identical to rope_neox(past + i) +
    PagedKV4.write_token; nothing else in the pools moves (positions below past, the sentinel page behind each table row and the
    pages no table names keep their fill bytes -- the expectation starts from the same fill)."""
    pairs = [(p, LENS[(i + shift) % 4]) for i, p in enumerate(PASTS)]
    case = pc.Case(pairs, 8, 2, tpb, seed=100 + shift, write_past=False)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)          # pools before the call: fill bytes everywhere
    want = pc.write_at(case.qkv_raw, case.lens, case.pasts, case)
    qkv_d = to_dev(case.qkv_raw)
    _write_at(qkv_d, case.lens, case.pasts, gk.table, 8, 2, tpb)
    torch.cuda.synchronize()
    assert_f16_equal(qkv_d, want, "qkv after the in-place RoPE at past + i")
    kp, vp = gk.pools()
    assert np.array_equal(kp, case.kc.pool), "K pages differ"
    assert np.array_equal(vp, case.vc.pool), "V pages differ"
    for b in range(case.B):      # (spelled out: the region below past and the sentinel page are still the fill byte)
        below = int(case.pasts[b])
        for pg in range(case.pages):
            page = kp[int(case.kidx[b][pg])][: 2 * tpb * D // 2].reshape(2, tpb, D // 2)
            lo, hi = pg * tpb, (pg + 1) * tpb
            keep = np.arange(lo, hi) < below if pg < case.pages - 1 else np.ones(tpb, bool)
            assert (page[:, keep] == pc.FILL).all()


def test_writer_in_chunks_equals_writer_in_one_call():
    """150 tokens through omni_kv4_prefill_write in one call, and as chunks of 64, 1 and 85 through the writer at an offset:
    byte-identical pools and byte-identical rotated q / k."""
    import omniserve_backend.fused_attention_fine_grained_dense as fa
    Hq, Hk, tpb, L, B = 8, 2, 64, 150, 2
    case = pc.Case([(0, L)] * B, Hq, Hk, tpb, seed=7, write_past=False)
    one, chunks = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx), GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    qkv_one = to_dev(case.qkv_raw)
    pad = fa.compute_padding_offsets(to_dev(case.cu), L, B * L)
    flags, rank = to_dev(np.ones(Hk, np.int32)), to_dev(np.arange(Hk, dtype=np.int32))
    fa.apply_bias_rope_update_kv_cache(qkv_one, to_dev(case.lens), None, pad, one.table, None, flags, rank, Hq, Hk, L, tpb,
                                       Hk * D // 2, 0, 0, 0, 0, 0, Hk, 0, D, pc.ROPE_BASE, 1.0, 1 << 20, True, True, True)
    raw = case.qkv_raw.reshape(B, L, -1)
    got = np.empty_like(raw)
    s = 0
    for n in (64, 1, 85):
        part = to_dev(raw[:, s:s + n].reshape(B * n, -1))
        _write_at(part, [n] * B, [s] * B, chunks.table, Hq, Hk, tpb)
        got[:, s:s + n] = part.cpu().numpy().reshape(B, n, -1)
        s += n
    torch.cuda.synchronize()
    assert_f16_equal(got.reshape(B * L, -1), qkv_one.cpu().numpy(), "rotated rows, chunks vs one call")
    for a, b in zip(one.pools(), chunks.pools()):
        assert np.array_equal(a, b)


# ---- attention -------------------------------------------------------------------------------------------------------------
def _run_raw(case, gk, qkv_rot, strided=True, max_q=None):
    """The C entry on a caller-owned `out` with a sentinel band behind it; -> fp16 [T, Hq, D] (numpy)."""
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
    max_q = int(max_q if max_q is not None else max(int(case.lens.max()), 1) + 77)     # larger than the longest sequence
    cu_d, past_d = to_dev(case.cu), to_dev(case.pasts)      # (named: they must outlive the launch)
    rc = _lib.lib().omni_prefill_attention_paged_kv4(
        out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
        cu_d.data_ptr(), past_d.data_ptr(), gk.table.data_ptr(), case.B, gk.table.shape[-1], case.tpb,
        max_q, Hq, Hk, D, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy()
    assert (host[T * Hq * D:] == SENTINEL).all(), "the band behind out was written"
    return host[: T * Hq * D].view(np.float16).reshape(T, Hq, D)


@functools.lru_cache(maxsize=None)
def _family(name):
    Hq, Hk, tpb, pairs = pc.ATTENTION_FAMILIES[name]
    case = pc.Case(pairs, Hq, Hk, tpb, seed=sum(map(ord, name)))
    return case, pc.case_expected_attention(case)      # (computed once, never modified)


@pytest.mark.parametrize("name", sorted(pc.ATTENTION_FAMILIES))
@pytest.mark.parametrize("strided", [True, False])
def test_attention_grid(name, strided):
    """32 (past, len_q) pairs over tokens_per_block 16 / 64 and GQA ratios 1 / 4 / 7 / 8; q / k / v as views of the qkv buffer and
    as contiguous tensors; max_seqlen_q larger than the longest sequence; a sentinel band behind out."""
    case, want = _family(name)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot, strided=strided)
    assert_attention_close(got, want, "paged prefill attention %s (%s)" % (name, "views" if strided else "contiguous"))


@functools.lru_cache(maxsize=None)
def _mixed():
    case = pc.Case(pc.MIXED_BATCH, 8, 2, 64, seed=31)
    return case, pc.case_expected_attention(case)


def test_attention_mixed_batch_with_empty_sequences():
    """(past, len_q) = (0, 40), (200, 0), (65, 129), (0, 0), (130, 1) in one batch, shuffled non-contiguous tables."""
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot)
    assert_attention_close(got, want, "paged prefill attention, mixed batch")


def test_attention_never_reads_slots_at_or_behind_past():
    """Every page slot at a position >= past -- the rest of the last partial page, the slots where the chunk's own quantised copy
    sits, the pages behind -- holds data 0xFF with scale = zero = NaN: the output is finite and within the bar.  With the chunk's
    real quantised copy in those slots (the writer ran first) the output is bit-identical."""
    case, want = _mixed()
    kc_p, vc_p = pc.poison_from_past(case, case.kc, case.kidx), pc.poison_from_past(case, case.vc, case.vidx)
    got_poison = _run_raw(case, GpuPagedKV(kc_p, vc_p, case.kidx, case.vidx), case.qkv_rot)
    assert np.isfinite(got_poison.astype(np.float32)).all()
    assert_attention_close(got_poison, want, "paged prefill attention, poisoned slots >= past")
    import copy
    written = copy.copy(case)
    written.kc, written.vc = copy.copy(case.kc), copy.copy(case.vc)
    written.kc.pool, written.vc.pool = case.kc.pool.copy(), case.vc.pool.copy()
    pc.write_at(case.qkv_raw, case.lens, case.pasts, written)
    assert not np.array_equal(written.kc.pool, case.kc.pool)
    got_written = _run_raw(case, GpuPagedKV(written.kc, written.vc, case.kidx, case.vidx), case.qkv_rot)
    assert np.array_equal(got_written.view(np.uint16), got_poison.view(np.uint16))


def test_attention_with_no_past_agrees_with_the_fresh_prefill_kernel():
    from omniserve_amd.backend import fused_ext
    from omniserve_amd.backend.prefill_attn import flash_attn_varlen_func
    case = pc.Case([(0, 200), (0, 1), (0, 129), (0, 64)], 8, 2, 64, seed=41)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    qkv_d = to_dev(case.qkv_rot)
    q, k, v = (t for t in case.split(qkv_d))
    cu = to_dev(case.cu)
    fresh = flash_attn_varlen_func(q, k, v, cu, cu, 200, 200, causal=True)
    got = fused_ext.prefill_attention_paged_kv4(q, k, v, cu, to_dev(case.pasts), gk.table, 64, 200)
    torch.cuda.synchronize()
    assert_attention_close(got.cpu().numpy(), fresh.cpu().numpy(), "paged (past 0) vs omni_prefill_attention")
    assert_attention_close(got.cpu().numpy(), pc.case_expected_attention(case), "paged (past 0) vs oracle")


def test_attention_of_one_query_agrees_with_the_decode_kernel():
    """len_q = 1: the decode kernel (un-rotated q / k, it rotates and appends itself) and the paged prefill kernel (rows rotated
    by the writer at an offset) see the same keys and values: two kernels, each within 1e-3 of the same mathematics -> 2e-3."""
    import omniserve_backend.fused_attention_pure_dense as fa
    from omniserve_amd.backend import fused_ext
    Hq, Hk = 8, 2
    case = pc.Case([(1, 1), (63, 1), (64, 1), (65, 1), (130, 1), (200, 1)], Hq, Hk, 64, seed=51)
    g_dec, g_new = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx), GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    raw_d = to_dev(case.qkv_raw)
    q, k, v = case.split(raw_d)
    lens = to_dev(case.pasts + 1)
    dec = fa.single_query_attention(q, k, v, g_dec.table, lens, None, 65536, 64, Hk * D // 2, int(case.pasts.max()) + 1, D,
                                    pc.ROPE_BASE, True, True, True)
    rot_d = to_dev(case.qkv_raw)
    _write_at(rot_d, case.lens, case.pasts, g_new.table, Hq, Hk, 64)
    qr, kr, vr = case.split(rot_d)
    got = fused_ext.prefill_attention_paged_kv4(qr, kr, vr, to_dev(case.cu), to_dev(case.pasts), g_new.table, 64, 1)
    torch.cuda.synchronize()
    for a, b in zip(g_dec.pools(), g_new.pools()):       # both appended the same quantised token
        assert np.array_equal(a, b)
    assert_attention_close(got.cpu().numpy(), dec.cpu().numpy(), "paged prefill (len_q 1) vs decode kernel", bar=2e-3)
    assert_attention_close(got.cpu().numpy(), pc.case_expected_attention(case), "paged prefill (len_q 1) vs oracle")


def test_refused_configurations_raise():
    from omniserve_amd.backend import fused_ext
    case = pc.Case([(16, 4)], 8, 2, 64, seed=61)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    qkv_d = to_dev(case.qkv_rot)
    q, k, v = case.split(qkv_d)
    cu, past = to_dev(case.cu), to_dev(case.pasts)
    ok = fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past, gk.table, 64, 4)
    assert ok.shape == (4, 8, D)
    with pytest.raises(NotImplementedError):
        fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past, gk.table, 64, 4, causal=False)
    with pytest.raises(NotImplementedError):
        fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past, gk.table, 64, 4, head_mask_type=to_dev(np.zeros(8, np.int32)),
                                              streaming_info=to_dev(np.zeros(16, np.int32)))
    with pytest.raises(RuntimeError):
        fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past, gk.table, 24, 4)                 # tokens_per_block
    with pytest.raises(RuntimeError):
        fused_ext.prefill_attention_paged_kv4(q[:, :7], k, v, cu, past, gk.table, 64, 4)          # 7 q heads over 2 kv heads
    with pytest.raises(RuntimeError):
        fused_ext.prefill_attention_paged_kv4(q.float(), k, v, cu, past, gk.table, 64, 4)         # dtype
    with pytest.raises(RuntimeError):
        fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past[:0], gk.table, 64, 4)             # past_lens shape
    with pytest.raises(RuntimeError):
        fused_ext.prefill_attention_paged_kv4(q, k, v, cu.long(), past, gk.table, 64, 4)          # cu_seqlens dtype
    with pytest.raises(RuntimeError):      # the RoPE table / block table cannot cover past + len
        _write_at(to_dev(case.qkv_raw), [4], [4096], gk.table, 8, 2, 64)
    torch.cuda.synchronize()
