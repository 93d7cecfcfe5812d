"""Decode attention and page selector at GQA ratios that are no whole number of head tiles (3, 5, 6, 7, 10; 7 = Yi-34B's
56 q heads over 8 kv heads).  A workgroup of the decode kernel serves a tile of 4 or 8 q heads of one kv head; the last
tile of such a group is ragged: its padded head slots carry a zero q, run through the sweep and store nothing.

a. parity with the f32 oracle at the project's attention bar (tests/util.py: per-head relative L2 and max error <= 1e-3, no
   absolute term), contexts 1 / 63 / 64 / 65 / several KV splits mixed in a batch, the split count read back from the
   partials entry; appended cache rows byte-identical to the oracle's and to what a ratio-4 call writes for the same k, v;
b. head independence, bit for bit: the heads a ratio-7 (3) call shares with a ratio-8 (4) call on the same pools come out
   identical -- a wrong head <-> slot mapping or anything leaking out of a padded slot cannot hide behind a tolerance;
c. nothing is stored past the output tensor (sentinel guards on both sides);
d. ratio 7 through the fine-grained (dense and sparse, mixed retrieval / streaming kv heads) and per-tensor KV8 entries;
e. the page selector at ratios 3 and 7 with a head that spans several selector workgroups, and the page choice on its scores;
f. a 2-layer Yi-34B runner: graph = eager, fusion level 0 = level 2, also on a TP = 2 shard (28 / 4 heads)."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import kv4
from tests.util import GpuPagedKV, assert_attention_close, dev, f16_ulp_diff, to_dev

pytestmark = pytest.mark.gpu

D, TPB, HK, B = 128, 64, 2, 2
ROPE_BASE = 500000.0
LONG = 300          # ceil(300 / 64) = 5 candidate splits of <= 64 tokens: the planner takes several (asserted below)
# lengths INCLUDE the current token; per case one batch of two sequences
LENS = {"1+64": (1, 64), "63+65": (63, 65), "long+1": (LONG, 1), "65+long": (65, LONG)}
PAGES = (LONG + TPB - 1) // TPB


@functools.lru_cache(maxsize=None)
def _pools(case):
    """Random KV4 pages with sane scale / zero tails (as tests/test_edge_cases_gpu.py does for the BASELINE shapes), the
    page tables, and k / v of the current token: shared by every ratio, never modified (users copy)."""
    rng = np.random.default_rng(sorted(LENS).index(case) + 100)
    n = B * PAGES
    kc, vc = kv4.PagedKV4(n, HK, D), kv4.PagedKV4(n, HK, D)
    for c in (kc, vc):
        c.pool[:] = rng.integers(0, 256, c.pool.shape, dtype=np.uint8)
        for p in range(n):
            c.scales(p)[:] = (0.05 + 0.15 * rng.random((HK, TPB))).astype(np.float16)
            c.zeros(p)[:] = (6.0 + 3.0 * rng.random((HK, TPB))).astype(np.float16)
    kidx, vidx = rng.permutation(n).reshape(B, PAGES), rng.permutation(n).reshape(B, PAGES)
    k = rng.standard_normal((B, HK, D)).astype(np.float16)
    v = rng.standard_normal((B, HK, D)).astype(np.float16)
    for a in (kc.pool, vc.pool, kidx, vidx, k, v):
        a.setflags(write=False)
    return kc, vc, kidx, vidx, k, v


def _fresh(case):
    kc0, vc0, kidx, vidx, k, v = _pools(case)
    kc, vc = kv4.PagedKV4(1, HK, D), kv4.PagedKV4(1, HK, D)
    kc.pool, vc.pool = kc0.pool.copy(), vc0.pool.copy()
    return kc, vc, kidx, vidx, k, v


def _q(case, hq, seed=0):
    rng = np.random.default_rng(1000 * hq + 10 * seed + sorted(LENS).index(case))
    return (0.5 * rng.standard_normal((B, hq, D))).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _oracle(case, hq):
    """(f32-oracle output, K pool, V pool after the append) -- the oracle loops over the kv heads' groups for any ratio."""
    kc, vc, kidx, vidx, k, v = _fresh(case)
    lens = np.asarray(LENS[case], np.int32)
    want = kv4.decode_attention(_q(case, hq), k, v, lens, kc, vc, kidx, vidx, ROPE_BASE)
    for a in (want, kc.pool, vc.pool):
        a.setflags(write=False)
    return want, kc.pool, vc.pool


def _run(case, hq, q=None):
    """single_query_attention through the mirror on fresh pools -> (out fp16 [B, hq, D] numpy, K pool, V pool)."""
    import omniserve_backend.fused_attention_pure_dense as fa
    kc, vc, kidx, vidx, k, v = _fresh(case)
    gk = GpuPagedKV(kc, vc, kidx, vidx)
    lens = np.asarray(LENS[case], np.int32)
    q = _q(case, hq) if q is None else q
    out = fa.single_query_attention(to_dev(q), to_dev(k), to_dev(v), gk.table, to_dev(lens), None, 65536, TPB,
                                    HK * D // 2, int(lens.max()), D, ROPE_BASE, True, True, True)
    torch.cuda.synchronize()
    kp, vp = gk.pools()
    return out.cpu().numpy(), kp, vp


def _partials(case, hq, q=None):
    """omni_kv4_decode_attention_partial on fresh pools -> (nsplit, part_ml [B, hq, S, 2], part_o [B, hq, S, D])."""
    from omniserve_amd import _lib
    from omniserve_amd.rope import rope_table
    kc, vc, kidx, vidx, k, v = _fresh(case)
    gk = GpuPagedKV(kc, vc, kidx, vidx)
    lens = np.asarray(LENS[case], np.int32)
    max_ctx = int(lens.max())
    qd, kd, vd, ld = to_dev(_q(case, hq) if q is None else q), to_dev(k), to_dev(v), to_dev(lens)
    table = rope_table(max_ctx + 1, D, ROPE_BASE, 1.0, dev())
    need = int(_lib.lib().omni_kv4_decode_workspace_bytes(B, hq, D, max_ctx))
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev())
    ns = ctypes.c_int(0)
    rc = _lib.lib().omni_kv4_decode_attention_partial(
        qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), qd.stride(0), kd.stride(0), gk.table.data_ptr(), ld.data_ptr(), B,
        gk.table.shape[-1], hq, HK, D, TPB, max_ctx, table.data_ptr(), table.shape[0], ws.data_ptr(), ws.numel(),
        ctypes.byref(ns), _lib.current_stream())
    _lib.check(rc, "omni_kv4_decode_attention_partial")
    torch.cuda.synchronize()
    s = ns.value
    f = ws.cpu().numpy().view(np.float32)
    ml = f[: B * hq * s * 2].reshape(B, hq, s, 2)
    po = f[B * hq * s * 2: B * hq * s * (2 + D)].reshape(B, hq, s, D)
    return s, ml, po


@functools.lru_cache(maxsize=None)
def _ratio_4_pools(case):
    return _run(case, 4 * HK)[1:]


# ---------------------------------------------------------------------------------------------------------------
# a. parity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(LENS))
@pytest.mark.parametrize("hq", [6, 10, 12, 14, 20])      # ratios 3, 5, 6, 7, 10 (tiles 4 + 4 + 2)
def test_ragged_ratio_matches_the_oracle(hq, case):
    want, kref, vref = _oracle(case, hq)
    got, kp, vp = _run(case, hq)
    assert_attention_close(got, want, "ratio %d, lengths %s" % (hq // HK, LENS[case]))
    assert np.array_equal(kp, kref) and np.array_equal(vp, vref), "K / V pages after the append differ from the oracle's"
    # the writer does not depend on the ratio: same bytes as a ratio-4 call with the same k, v
    kp4, vp4 = _ratio_4_pools(case)
    assert np.array_equal(kp, kp4) and np.array_equal(vp, vp4), "appended rows differ from the ratio-4 call's"


@pytest.mark.parametrize("case", ["long+1", "65+long"])
@pytest.mark.parametrize("hq", [6, 10, 12, 14, 20])
def test_ragged_partials_merge_to_the_oracle(hq, case):
    """The two-launch form over several KV splits: the partial rows are indexed by real head, so merging them on the host
    (the merge kernels' formula) must give the oracle's output for every head -- and the plan really has >= 2 splits."""
    want = _oracle(case, hq)[0]
    ns, ml, po = _partials(case, hq)
    assert ns >= 2, "the plan has %d split(s): the merge over ragged partials is not exercised" % ns
    m = ml[..., 0].astype(np.float64)
    w = np.exp(m - m.max(axis=-1, keepdims=True))
    lsum = (w * ml[..., 1]).sum(axis=-1)
    out = (w[..., None] * po).sum(axis=2) / (lsum[..., None] + 1e-6)
    assert_attention_close(out.astype(np.float16), want, "merged partials, ratio %d, %d splits" % (hq // HK, ns))


# ---------------------------------------------------------------------------------------------------------------
# b. head independence, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["1+64", "65+long"])
@pytest.mark.parametrize("ragged,whole", [(7, 8), (3, 4)])
def test_shared_heads_are_bit_identical_to_the_next_whole_ratio(ragged, whole, case):
    qr = _q(case, ragged * HK, seed=5)
    qw = _q(case, whole * HK, seed=6).reshape(B, HK, whole, D).copy()
    qw[:, :, :ragged] = qr.reshape(B, HK, ragged, D)
    qw = qw.reshape(B, whole * HK, D)
    ns_r, ns_w = _partials(case, ragged * HK, qr)[0], _partials(case, whole * HK, qw)[0]
    # both ratios are one tile of the same width per kv head (7, 8 -> 8; 3, 4 -> 4): same workgroups per split, same plan
    assert ns_r == ns_w, "plans differ (%d vs %d splits): pick other lengths" % (ns_r, ns_w)
    out_r = _run(case, ragged * HK, qr)[0].reshape(B, HK, ragged, D)
    out_w = _run(case, whole * HK, qw)[0].reshape(B, HK, whole, D)
    assert np.isfinite(out_r.astype(np.float32)).all()
    assert np.array_equal(out_r.view(np.uint16), out_w[:, :, :ragged].view(np.uint16)), \
        "ratio %d vs %d (%d splits): shared heads differ" % (ragged, whole, ns_r)


# ---------------------------------------------------------------------------------------------------------------
# c. overrun guard
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["1+64", "65+long"])      # one split (the kernel stores the output itself) and the merge kernel
@pytest.mark.parametrize("hq", [6, 14, 20])
def test_padded_slots_store_nothing_outside_the_output(hq, case):
    from omniserve_amd import _lib
    from omniserve_amd.rope import rope_table
    kc, vc, kidx, vidx, k, v = _fresh(case)
    gk = GpuPagedKV(kc, vc, kidx, vidx)
    lens = np.asarray(LENS[case], np.int32)
    max_ctx = int(lens.max())
    n, guard = B * hq * D, 16 * D
    sentinel = 0x7BAD
    big = torch.full((guard + n + guard,), sentinel, dtype=torch.int16, device=dev())
    out = big[guard: guard + n].view(torch.float16)
    qbig = torch.full((guard + n + guard,), float("nan"), dtype=torch.float16, device=dev())
    qd = qbig[guard: guard + n].view(B, hq, D)
    qd.copy_(to_dev(_q(case, hq)))
    kd, vd, ld = to_dev(k), to_dev(v), to_dev(lens)
    table = rope_table(max_ctx + 1, D, ROPE_BASE, 1.0, dev())
    need = int(_lib.lib().omni_kv4_decode_workspace_bytes(B, hq, D, max_ctx))
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev())
    rc = _lib.lib().omni_kv4_decode_attention(
        out.data_ptr(), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), qd.stride(0), kd.stride(0), gk.table.data_ptr(),
        ld.data_ptr(), B, gk.table.shape[-1], hq, HK, D, TPB, max_ctx, table.data_ptr(), table.shape[0], ws.data_ptr(),
        ws.numel(), _lib.current_stream())
    _lib.check(rc, "omni_kv4_decode_attention")
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert (host[:guard] == sentinel).all() and (host[guard + n:] == sentinel).all(), "stores outside the output tensor"
    got = host[guard: guard + n].view(np.float16).reshape(B, hq, D)
    assert_attention_close(got, _oracle(case, hq)[0], "guarded call, ratio %d" % (hq // HK))


# ---------------------------------------------------------------------------------------------------------------
# d. the fine-grained and per-tensor KV8 families at ratio 7 (smallest configurations of their own suites, same bars)
# ---------------------------------------------------------------------------------------------------------------
def _dyn_fn(c, P, tpb):
    def dyn_fn(hist):
        dyn = np.zeros((c.B, c.Hq, P), np.int32)
        for b in range(c.B):
            last = (int(hist[b]) - 1) // tpb
            for h in range(c.Hq):
                pick = c.rng.choice(last, size=P - 1, replace=False) if last >= P - 1 else np.arange(P - 1) % max(last, 1)
                dyn[b, h, : P - 1] = np.sort(pick)
                dyn[b, h, P - 1] = last
        return dyn
    return dyn_fn


@pytest.mark.parametrize("kv8", [False, True])
def test_ratio_7_fine_grained_and_kv8_dense(kv8):
    from tests.test_fine_grained_gpu import FLAGS_MIXED, Case
    from tests.test_per_tensor_kv8_gpu import SCALES
    c = Case([5, 40, 130, 200], 28, FLAGS_MIXED, 16, 16, 48, seed=77, kv8_scales=SCALES if kv8 else None)
    c.prefill()
    c.decode(2)


@pytest.mark.parametrize("kv8", [False, True])
def test_ratio_7_fine_grained_and_kv8_sparse(kv8):
    from tests.test_fine_grained_gpu import FLAGS_MIXED, Case
    from tests.test_per_tensor_kv8_gpu import SCALES
    tpb, P, sub = 16, 4, 8
    c = Case([130, 200, 97], 28, FLAGS_MIXED, tpb, 16, 48, seed=78, sub_chunk=sub, kv8_scales=SCALES if kv8 else None)
    c.prefill()
    cu = np.concatenate([[0], np.cumsum(c.seq_lens)]).astype(np.int32)
    k_post = c.qkv_post[:, c.Hq * D:(c.Hq + c.Hk) * D].reshape(-1, c.Hk, D)
    heads = [h for h in range(c.Hk) if c.flags[h]]
    kv4.paged_min_max_pool(k_post, cu, heads, c.rk.pool, c.rk_idx, tpb, sub, row_bytes=c.row)
    c.g_retr.kpool.copy_(to_dev(c.rk.pool))
    c.decode(2, _dyn_fn(c, P, tpb))


# ---------------------------------------------------------------------------------------------------------------
# e. page selector
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [3, 7])
def test_page_selector_ragged_ratio(g):
    """Sequence 0 has 40 pages (two selector workgroups per head tile), sequence 1 two.  Scores within 2 fp16 ulp of the
    oracle (fp16 products, f32 vs f64 sums: the bar of tests/test_sparse_utils_gpu.py); the page choice on these scores is
    what torch.topk takes."""
    import omniserve_backend.fused_attention_selector as sel
    from omniserve_amd.backend import fused_ext
    from tests.test_sparse_utils_gpu import SUB, _setup
    seq_lens, Hin, pooled = [2500, 70], 2, [0, 1]
    k, cu, pool, table, pb = _setup(seq_lens, Hin, pooled, seed=g)
    H = len(pooled)
    kv4.paged_min_max_pool(k, cu, pooled, pool, table, TPB, SUB)
    pool_d = to_dev(pool)
    nb, M = table.shape
    ptr = np.zeros((nb, 2, M), np.int64)
    ptr[:, 0, :] = pool_d.data_ptr() + table.astype(np.int64) * pb
    ptr[:, 1, :] = ptr[:, 0, :]
    ptr_d = to_dev(ptr)
    Hq = Hin * g
    flags, rank = np.ones(Hin, np.int32), np.arange(Hin, dtype=np.int32)
    lengths = (np.asarray(seq_lens) + 1).astype(np.int32)
    q = np.random.default_rng(g).standard_normal((nb, Hq, D)).astype(np.float16)
    want = kv4.page_selector(q, lengths, flags, rank, pool, table, Hin, H, TPB, SUB, ROPE_BASE)
    dummy = torch.empty((nb, Hin, D), dtype=torch.float16, device=dev())
    got = sel.single_query_page_selector(to_dev(q), dummy, dummy, ptr_d, None, to_dev(flags), to_dev(rank), None,
                                         to_dev(lengths), None, 65536, TPB, H * D // 2, 0, 0, 0, 0, 0, H, 0,
                                         int(max(seq_lens)), D, ROPE_BASE, 1.0, True, True, True, SUB, H * D, 1000000)
    torch.cuda.synchronize()
    assert tuple(got.shape) == want.shape
    assert f16_ulp_diff(got, want) <= 2
    # page choice of sequence 0 (40 pages) on the device scores: k best of all pages but the newest, newest last
    subs = TPB // SUB
    pages, kk = (seq_lens[0] + TPB - 1) // TPB, 9
    sc = got[:1, :, : pages * subs].contiguous()
    out = torch.empty((1, Hq, kk + 1), dtype=torch.int32, device=dev())
    fused_ext.select_topk_pages(out, sc, subs, pages, kk)
    torch.cuda.synchronize()
    page_scores = sc.cpu().view(1, Hq, pages, subs).max(dim=-1).values.float()
    want_vals, _ = page_scores[:, :, : pages - 1].topk(k=kk, dim=-1)
    idx = out.cpu().long()
    assert (idx[:, :, kk] == pages - 1).all()
    assert torch.equal(torch.gather(page_scores, 2, idx[:, :, :kk]), want_vals)
    assert np.array_equal(out.cpu().numpy(), kv4.topk_pages(sc.cpu().numpy(), subs, pages, kk))      # the same pages, in order


# ---------------------------------------------------------------------------------------------------------------
# f. runner
# ---------------------------------------------------------------------------------------------------------------
def _yi(layers=2):
    from omniserve_amd.runtime import LlamaConfig
    return dataclasses.replace(LlamaConfig.yi_34b(), layers=layers)


def _steps(fused, graph, steps=3, **kw):
    from omniserve_amd.runtime import DecodeRunner
    r = DecodeRunner(_yi(), batch=2, context=70, max_new=8, device=dev(), seed=3, use_graph=graph, fused=fused, **kw)
    toks = []
    for _ in range(steps):
        r.step()
        toks.append(r.tokens.clone())
    torch.cuda.synchronize()
    res = (r.fused, torch.stack(toks).cpu(), r.x.clone().cpu(), [p.clone().cpu() for p in r.pools[0]])
    del r
    torch.cuda.empty_cache()
    return res


def test_yi_34b_runner_levels_and_graph_agree_bitwise():
    """hidden 7168 is outside omni_gemm_rowfree_ok, so a request for level 3 (the default) settles on 2 through the runner's
    own gate.  Every level gives the bits of level 0 -- level 2 also with q / k / v read from the qkv projection's slabs
    (column arithmetic by real head) -- and a captured step the tokens of an eager one."""
    _, t0, x0, p0 = _steps(0, False)
    assert torch.isfinite(x0.float()).all()
    for fused, graph, kw, level in [(1, False, {}, 1), (2, False, dict(qkv_slabs=True), 2), (3, False, {}, 2),
                                    (True, True, {}, 2)]:
        got_level, t, x, p = _steps(fused, graph, **kw)
        assert got_level == level, (fused, got_level)
        assert torch.equal(t, t0), (fused, graph)
        assert torch.equal(x.view(torch.int16), x0.view(torch.int16)), (fused, graph)
        for a, b in zip(p, p0):
            assert torch.equal(a, b), (fused, graph)


def test_yi_34b_runner_tp2_shard_steps():
    """A TP = 2 rank holds 28 q heads over 4 kv heads -- still ratio 7.  One process (the peers' buffers alias this rank's own:
    the collective's values are not a model's, the attention's shapes are)."""
    from omniserve_amd.runtime import DecodeRunner
    r = DecodeRunner(_yi(), batch=2, context=70, max_new=8, device=dev(), seed=3, use_graph=False, fused=True, tp_rank=0,
                     tp_size=2, tp_comm="loopback")
    assert (r.hl, r.kl) == (28, 4)
    for _ in range(2):
        r.step()
    torch.cuda.synchronize()
    assert int(r.lengths[0]) == 72
    assert ((r.tokens >= 0) & (r.tokens < r.cfg.vocab)).all()
