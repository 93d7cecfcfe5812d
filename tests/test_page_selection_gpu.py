"""The LServe page choice on the GPU against the oracle, on the cases of tests/page_selection_cases.py (each proved to be what it
claims in tests/test_page_selection_cpu.py):

a. select_topk_pages is oracle.kv4.topk_pages entry for entry -- which pages, not only which scores: tie groups over, inside
   and outside the k-th place, all-equal rows, +-0, +-inf, 1..16 sub-chunks per page, the vector and the scalar load path on the
   same data, k = 0 .. 1024, 0 .. 14336 candidate pages (the declared limits), every refusal of the host entry;
b. pooling and selector on NaN-poisoned pages around the selector's workgroup boundary: pages bit-identical, scores within the
   project's 2 fp16 ulp, nothing read or written that should not be;
c. prefill -> pool -> selector -> top-k -> sparse attention on planted pages, KV4 and KV8: the oracle's pages, then its output.
"""
import numpy as np
import pytest
import torch

from oracle import kv4
from tests import page_selection_cases as pc
from tests.util import dev, f16_ulp_diff, to_dev

pytestmark = pytest.mark.gpu
D = pc.D
UNSET = -7


def _dev(a):
    return to_dev(np.array(a))       # the cases' arrays are read-only: upload a copy


# ---- a. top-k ------------------------------------------------------------------------------------------------------------
def _topk(scores_d, c):
    from omniserve_amd.backend import fused_ext
    B, H, _ = scores_d.shape
    out = torch.full((B, H, c.k + 1), UNSET, dtype=torch.int32, device=dev())
    fused_ext.select_topk_pages(out, scores_d, c.subs, c.total_pages, c.k)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in pc.topk_cases()])
def test_select_topk_pages_is_index_exact(name):
    c = pc.topk_case(name)
    want = c.want()
    sd = _dev(c.scores)
    assert sd.data_ptr() % 8 == 0
    got = _topk(sd, c)
    assert (got != UNSET).all(), "%d of the k + 1 slots were not written" % (got == UNSET).sum()
    assert (got[..., : c.k] != c.n).all(), "the newest page is among the k best"
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d entries differ, first at %s: page %d, want %d" % (
        len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    if c.tail is not None:
        first, pages = c.tail
        assert (got[..., first: first + len(pages)] == np.asarray(pages, np.int32)).all()
    if c.subs == 4:      # the same scores 2 bytes into a buffer: the 8-byte loads give way to the scalar loop
        buf = torch.empty((sd.numel() + 1,), dtype=torch.float16, device=dev())
        off = buf[1:].view(sd.shape)
        off.copy_(sd)
        assert off.is_contiguous() and off.data_ptr() % 8 == 2
        assert np.array_equal(_topk(off, c), got), "aligned and unaligned scores give different pages"


REFUSALS = {
    # name: (scores shape, slice, subs, total_pages, k, out shape)
    "k_above_the_candidates": ((1, 2, 5 * 2), None, 2, 5, 5, (1, 2, 6)),
    "k_1025": ((1, 2, 2000), None, 1, 2000, 1025, (1, 2, 1026)),
    "total_pages_14338": ((1, 2, 14338), None, 1, 14338, 10, (1, 2, 11)),
    "scores_narrower_than_the_candidates": ((1, 2, 99 * 4 - 1), None, 4, 100, 10, (1, 2, 11)),
    "scores_not_contiguous": ((1, 2, 2 * 100 * 4), 2, 4, 100, 10, (1, 2, 11)),
    "out_of_the_wrong_shape": ((1, 2, 100 * 4), None, 4, 100, 10, (1, 2, 10)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_select_topk_pages_refusals_leave_out_untouched(name):
    from omniserve_amd.backend import fused_ext
    shape, step, subs, total_pages, k, out_shape = REFUSALS[name]
    scores = torch.randn(shape, generator=torch.Generator().manual_seed(1)).half().to(dev())
    if step:
        scores = scores[:, :, ::step]
        assert not scores.is_contiguous() and scores.shape[-1] == total_pages * subs
    out = torch.full(out_shape, UNSET, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError):
        fused_ext.select_topk_pages(out, scores, subs, total_pages, k)
    torch.cuda.synchronize()
    assert (out == UNSET).all()
    # the neighbouring accepted call: the same tensors at the limit's own side
    if name == "k_above_the_candidates":
        ok = torch.full((1, 2, 5), UNSET, dtype=torch.int32, device=dev())
        fused_ext.select_topk_pages(ok, scores, subs, total_pages, 4)
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy(), kv4.topk_pages(scores.cpu().numpy(), subs, total_pages, 4))


# ---- b. pool and selector ------------------------------------------------------------------------------------------------
def _selector(c, q_d, ptr_d):
    import omniserve_backend.fused_attention_selector as sel
    s = c.spec
    dummy = torch.empty((c.B, c.Hk, D), dtype=torch.float16, device=dev())
    got = sel.single_query_page_selector(q_d, dummy, dummy, ptr_d, None, _dev(c.flags), _dev(c.rank), None, _dev(c.lengths),
                                         None, 65536, s.tpb, c.H * D // 2, 0, 0, 0, 0, 0, c.H, c.Hk - c.H, int(max(s.hist)), D,
                                         pc.ROPE_BASE, s.rope_scale, True, True, True, s.sub, c.H * D, 1000000)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("name", [s.name for s in pc.SELECTOR_SPECS])
def test_pool_and_selector_on_poisoned_pages(name):
    import omniserve_backend.fused_attention_ctx_pool as cp
    c = pc.selector_case(name)
    s = c.spec
    pool_d = _dev(c.pool0)
    ptr = np.zeros((c.B, 2, c.pages), np.int64)
    ptr[:, 0, :] = pool_d.data_ptr() + c.table.astype(np.int64) * c.page_bytes
    ptr[:, 1, :] = ptr[:, 0, :]
    ptr_d = to_dev(ptr)
    cp.paged_min_max_pool(_dev(c.k), ptr_d, _dev(c.cu), to_dev(np.asarray(c.pooled, np.int32)), int(max(s.hist)), s.sub,
                          s.tpb, c.H * D // 2, True)
    torch.cuda.synchronize()
    assert np.array_equal(pool_d.cpu().numpy(), c.pool), "pooled pages differ from the oracle's (poison included)"

    got = _selector(c, _dev(c.q), ptr_d)
    assert got.shape == c.want.shape
    assert not np.isnan(got).any(), "a poisoned statistic was read"
    for b in range(c.B):
        assert (got.view(np.uint16)[b, :, c.n_sub(b):] == 0).all(), "sequence %d: a slot past its sub-chunks was written" % b
    assert (got.view(np.uint16)[:, s.group: 2 * s.group] == 0).all(), "streaming heads must stay zero"
    ulp = f16_ulp_diff(got, c.want)
    print("%s: max distance %d ulp" % (name, ulp))
    assert ulp <= 2
    # q as the decode step passes it: a view into the qkv projection's output (k, v columns poisoned)
    qkv = torch.full((c.B, (c.Hq + 2 * c.Hk) * D), float("nan"), dtype=torch.float16, device=dev())
    q_view = qkv[:, : c.Hq * D].view(c.B, c.Hq, D)
    q_view.copy_(_dev(c.q))
    assert not q_view.is_contiguous() or c.B == 1
    assert np.array_equal(_selector(c, q_view, ptr_d).view(np.uint16), got.view(np.uint16)), "strided q: other bits"


# ---- c. the chain --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv8", [False, True], ids=["kv4", "kv8"])
def test_selector_topk_sparse_attention_chain(kv8):
    import omniserve_backend.fused_attention_selector as sel
    from omniserve_amd.backend import fused_ext
    from tests.test_fine_grained_gpu import Case
    from tests.test_per_tensor_kv8_gpu import SCALES, _pool_prompt_stats
    cc = pc.chain_case()
    tpb, sub, T = pc.CHAIN_TPB, pc.CHAIN_SUB, pc.CHAIN_HIST
    c = Case(cc.seq_lens, cc.Hq, list(pc.CHAIN_FLAGS), tpb, pc.CHAIN_SINK, pc.CHAIN_LOCAL, seed=1, sub_chunk=sub,
             kv8_scales=SCALES if kv8 else None)
    c.prefill(np.array(cc.qkv_prefill))            # asserts the rotated qkv and all four pools bit-identical
    _pool_prompt_stats(c, tpb, sub)                # pooling through the mirror; pools bit-identical again
    want_scores, want_pages = cc.oracle()
    qkv_d = _dev(cc.qkv_decode)
    Hq, Hk, B = c.Hq, c.Hk, c.B
    qd = qkv_d[:, : Hq * D].view(B, Hq, D)
    kd = qkv_d[:, Hq * D:(Hq + Hk) * D].view(B, Hk, D)
    vd = qkv_d[:, (Hq + Hk) * D:].view(B, Hk, D)

    def dyn_fn(hist):
        assert (np.asarray(hist) == T).all()
        lens = (np.asarray(hist) + 1).astype(np.int32)
        scores = kv4.page_selector(cc.q(), lens, c.flags, c.rank, c.rk.pool, c.rk_idx, Hk, c.nr, tpb, sub, pc.ROPE_BASE,
                                   row_bytes=c.row)
        assert np.array_equal(scores.view(np.uint16), want_scores.view(np.uint16)), "the statistics do not depend on the format"
        stats = sel.single_query_page_selector(
            qd, kd, vd, c.g_retr.table, c.g_strm.table, c.flags_d, c.rank_d, None, to_dev(lens), None, 65536, tpb,
            c.nr * c.row, c.ns * c.row, c.sink, c.local, c.sink_blocks, c.local_blocks, c.nr, c.ns, T, D, pc.ROPE_BASE, 1.0,
            True, not kv8, True, sub, c.nr * D, 1000000)
        out = torch.full((B, Hq, cc.k_best + 1), UNSET, dtype=torch.int32, device=dev())
        fused_ext.select_topk_pages(out, stats, tpb // sub, cc.total_pages, cc.k_best)      # on the DEVICE scores
        torch.cuda.synchronize()
        assert tuple(stats.shape) == want_scores.shape and f16_ulp_diff(stats, want_scores) <= 2
        pages = out.cpu().numpy()
        assert np.array_equal(pages, want_pages), "selected pages differ from the oracle chain's:\n%s\n%s" % (pages, want_pages)
        return pages

    # sparse attention with those pages against the oracle given the same; K / V / statistics after the append bit-identical
    c.decode(1, dyn_fn, qkv_fn=lambda step: np.array(cc.qkv_decode))
