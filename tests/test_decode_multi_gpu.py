"""Multi-token decode attention (omni_decode_attention_multi_kv4: 0 - 8 new tokens per sequence over the KV4 pages, split-KV) on the
GPU.  Bar: the project's assert_attention_close, 1e-3 per head against the f64 oracle over dequantised past + fresh keys
(tests/paged_prefill_cases.py); every raw call writes to a caller-owned `out` with a sentinel band behind it.  Cases:
tests/verify_attn_cases.py."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

from tests import paged_prefill_cases as pc
from tests import verify_attn_cases as vc
from tests.util import GpuPagedKV, assert_attention_close, to_dev

pytestmark = pytest.mark.gpu

D = pc.D
SENTINEL = 0x7BCD      # fp16 bits of the band behind `out`


@contextlib.contextmanager
def _forced_splits(n):
    from omniserve_amd import _lib
    _lib.lib().omni_decode_attention_multi_kv4_set_split_override(n)
    try:
        yield
    finally:
        _lib.lib().omni_decode_attention_multi_kv4_set_split_override(0)


def _run_raw(case, gk, qkv_rot, nsplit=0, strided=True, max_q=vc.MAX_Q):
    """The C entry on a caller-owned `out` with a sentinel band behind it and a workspace of exactly the advertised size;
    -> fp16 [T, Hq, D] (numpy)."""
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
    ws = torch.empty(h.omni_decode_attention_multi_kv4_workspace_bytes(case.B, Hq, max_q, max_past), dtype=torch.uint8,
                     device=qkv_d.device)
    cu_d, past_d = to_dev(case.cu), to_dev(case.pasts)      # (named: they must outlive the launch)
    with _forced_splits(nsplit):
        rc = h.omni_decode_attention_multi_kv4(
            out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
            cu_d.data_ptr(), past_d.data_ptr(), gk.table.data_ptr(), case.B, gk.table.shape[-1], case.tpb,
            max_q, Hq, Hk, D, max_past, ws.data_ptr(), ws.numel(), _lib.current_stream())
        torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy()
    assert (host[T * Hq * D:] == SENTINEL).all(), "the band behind out was written"
    return host[: T * Hq * D].view(np.float16).reshape(T, Hq, D)


@functools.lru_cache(maxsize=None)
def _family(name):
    case = vc.family(name)
    return case, pc.case_expected_attention(case)      # (computed once, never modified)


@pytest.mark.parametrize("name", sorted(vc.FAMILIES))
@pytest.mark.parametrize("nsplit", vc.SPLITS)
@pytest.mark.parametrize("strided", [True, False])
def test_attention_grid(name, nsplit, strided):
    """33 (past, len_q) pairs per family (every past and every len_q at least three times in each) over tokens_per_block 16 / 64
    and GQA ratios 1 / 4 / 7 / 8 (up to 64 rows per kv head: four 16-row tiles on one dequantised K / V tile); the planner's
    split count and 1, 2, 3, 7 forced splits (7 splits of past 0 ... 17: splits without a token); q / k / v as views of the qkv
    buffer and as contiguous tensors."""
    case, want = _family(name)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot, nsplit=nsplit, strided=strided)
    assert_attention_close(got, want, "multi-token decode attention %s, %d splits (%s)" % (
        name, nsplit, "views" if strided else "contiguous"))


@functools.lru_cache(maxsize=None)
def _mixed():
    case = vc.mixed()
    return case, pc.case_expected_attention(case)


@pytest.mark.parametrize("nsplit", [0, 3])
def test_attention_mixed_batch_with_empty_sequences(nsplit):
    """(past, len_q) = (0, 8), (200, 0), (65, 3), (0, 0), (130, 1), (17, 8) in one batch, shuffled non-contiguous tables."""
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    got = _run_raw(case, gk, case.qkv_rot, nsplit=nsplit)
    assert_attention_close(got, want, "multi-token decode attention, mixed batch, %d splits" % nsplit)


@pytest.mark.parametrize("nsplit", [0, 3])
def test_attention_never_reads_slots_at_or_behind_past(nsplit):
    """Every page slot at a position >= past holds data 0xFF with scale = zero = NaN: the output is finite and within the bar, and
    bit-identical to a run with the chunk's real quantised copy in those slots (the writer ran first)."""
    case, want = _mixed()
    kc_p, vc_p = pc.poison_from_past(case, case.kc, case.kidx), pc.poison_from_past(case, case.vc, case.vidx)
    got_poison = _run_raw(case, GpuPagedKV(kc_p, vc_p, case.kidx, case.vidx), case.qkv_rot, nsplit=nsplit)
    assert np.isfinite(got_poison.astype(np.float32)).all()
    assert_attention_close(got_poison, want, "multi-token decode attention, poisoned slots >= past")
    written = copy.copy(case)
    written.kc, written.vc = copy.copy(case.kc), copy.copy(case.vc)
    written.kc.pool, written.vc.pool = case.kc.pool.copy(), case.vc.pool.copy()
    pc.write_at(case.qkv_raw, case.lens, case.pasts, written)
    assert not np.array_equal(written.kc.pool, case.kc.pool)
    got_written = _run_raw(case, GpuPagedKV(written.kc, written.vc, case.kidx, case.vidx), case.qkv_rot, nsplit=nsplit)
    assert np.array_equal(got_written.view(np.uint16), got_poison.view(np.uint16))


@functools.lru_cache(maxsize=None)
def _needles():
    nb = vc.NeedleBatch()
    return nb, pc.expected_attention(nb.q, nb.k_new, nb.v_new, nb.cu, nb.pasts, nb.kc, nb.vc, nb.kidx, nb.vidx)


@pytest.mark.parametrize("nsplit", [3, 7])
def test_needles_in_one_launch(nsplit):
    """153 sequences over one shared table, sequence b aimed at key b (150 page keys, 3 fresh ones), forced splits: a key that is
    dropped, counted twice (by two splits, or as page slot AND fresh key) or leaked to a row in front of it moves that row by
    about its whole value; in particular row i of sequence 150 + j, j > i, must not see the fresh key it aims at."""
    nb, want = _needles()
    gk = GpuPagedKV(nb.kc, nb.vc, nb.kidx, nb.vidx)
    got = _run_raw(nb, gk, nb.qkv_rot, nsplit=nsplit, max_q=nb.n)
    assert_attention_close(got, want, "needles, %d splits" % nsplit)
    blind = got.reshape(nb.B, nb.n, nb.Hq, D)[nb.past + 2, 0]      # aims at fresh key 2, sees only fresh key 0 of the three
    assert_attention_close(blind, want.reshape(nb.B, nb.n, nb.Hq, D)[nb.past + 2, 0], "row 0 aimed at fresh key 2")


def test_two_runs_give_the_same_bits():
    case, _ = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    a = _run_raw(case, gk, case.qkv_rot, nsplit=3)
    b = _run_raw(case, gk, case.qkv_rot, nsplit=3)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def test_agrees_with_the_paged_prefill_kernel():
    """Two kernels, same mathematics, each within 1e-3 of it -> 2e-3 (the project's two-kernel bar); through the mirror, which
    allocates the workspace."""
    from omniserve_amd.backend import fused_ext
    case, want = _mixed()
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    q, k, v = case.split(to_dev(case.qkv_rot))
    cu, past = to_dev(case.cu), to_dev(case.pasts)
    paged = fused_ext.prefill_attention_paged_kv4(q, k, v, cu, past, gk.table, case.tpb, 8)
    got = fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, case.tpb, 8, int(case.pasts.max()))
    torch.cuda.synchronize()
    assert_attention_close(got.cpu().numpy(), paged.cpu().numpy(), "multi-token decode vs paged prefill kernel", bar=2e-3)
    assert_attention_close(got.cpu().numpy(), want, "multi-token decode (mirror) vs oracle")


def test_refused_configurations_raise():
    from omniserve_amd import _lib
    from omniserve_amd.backend import fused_ext
    case = pc.Case([(16, 4)], 8, 2, 64, seed=61)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    q, k, v = case.split(to_dev(case.qkv_rot))
    cu, past = to_dev(case.cu), to_dev(case.pasts)
    ok = fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, 64, 4, 16)
    assert ok.shape == (4, 8, D)
    with pytest.raises(fused_ext.DecodeMultiTooManyTokens):
        fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, 64, 9, 16)
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, 24, 4, 16)                 # tokens_per_block
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q[:, :7], k, v, cu, past, gk.table, 64, 4, 16)          # 7 q heads over 2 kv heads
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q.float(), k, v, cu, past, gk.table, 64, 4, 16)         # dtype
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q, k, v, cu, past[:0], gk.table, 64, 4, 16)             # past_lens shape
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q, k, v, cu.long(), past, gk.table, 64, 4, 16)          # cu_seqlens dtype
    with pytest.raises(RuntimeError):
        fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, 64, 4, 1 << 20)            # max_past beyond the table
    with pytest.raises(RuntimeError):      # a workspace shorter than the planner's one split
        fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, gk.table, 64, 4, 16,
                                             workspace=torch.empty(1024, dtype=torch.uint8, device=q.device))
    out = torch.empty((4, 8, D), dtype=torch.float16, device=q.device)
    rc = _lib.lib().omni_decode_attention_multi_kv4(
        out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0), cu.data_ptr(),
        past.data_ptr(), gk.table.data_ptr(), 1, gk.table.shape[-1], 64, 9, 8, 2, D, 16, None, 0, _lib.current_stream())
    assert rc == -22
    torch.cuda.synchronize()
