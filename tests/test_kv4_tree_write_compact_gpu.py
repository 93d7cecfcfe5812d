"""The two cache kernels of the tree verify step on the GPU: omni_kv4_prefill_write_at_pos (slot past + i, RoPE row past + depth)
and omni_kv4_compact_rows (the accepted path's rows to the front).  Both are compared byte for byte: pages and rotated rows
against oracle.kv4 (tests/tree_verify_cases.py), the compaction against a numpy move that snapshots first."""
import numpy as np
import pytest
import torch

from oracle import kv4
from tests import paged_prefill_cases as pc
from tests import tree_verify_cases as tc
from tests.util import GpuPagedKV, to_dev

pytestmark = pytest.mark.gpu

D = pc.D


def _write(case, gk, qkv_raw, rope_offsets):
    """-> the rotated rows (numpy); gk's pools hold the pages.  rope_offsets None: the plain writer at an offset."""
    from omniserve_amd.backend import fused_ext
    from omniserve_amd.backend.fused_attention_fine_grained_dense import compute_padding_offsets
    qkv = to_dev(qkv_raw)
    lens, pasts, cu = to_dev(case.lens), to_dev(case.pasts), to_dev(case.cu)
    n_max = int(case.lens.max())
    pad = compute_padding_offsets(cu, n_max, case.T)
    total = int((case.pasts + case.lens).max())
    if rope_offsets is None:
        fused_ext.kv4_prefill_write_at(qkv, lens, pasts, pad, gk.table, case.Hq, case.Hk, n_max, case.tpb, total, pc.ROPE_BASE)
    else:
        fused_ext.kv4_prefill_write_at_pos(qkv, lens, pasts, to_dev(rope_offsets), pad, gk.table, case.Hq, case.Hk, n_max,
                                           case.tpb, total, pc.ROPE_BASE)
    torch.cuda.synchronize()
    return qkv.cpu().numpy()


@pytest.mark.parametrize("tpb", [16, 64])
def test_write_at_pos_pages_and_rows(tpb):
    """pasts {0, 10, 63} (and a sequence without tokens), trees of 9, 32, 17 and 5 nodes of different kinds: the pages byte-exact
    and the rotated q / k rows bit-exact against rope_neox at past + depth and write_token at slot past + i; a tree's depths
    differ from its slots, so does the expectation from the plain writer's."""
    triples = [(0, 9, "binary"), (10, 32, "random"), (63, 17, "star"), (10, 0, "chain"), (63, 5, "two_chains")]
    case = tc.TreeCase(triples, 8, 2, tpb, seed=301 + tpb)
    gk = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)          # the pools before the call
    rot = _write(case, gk, case.qkv_raw, case.depth)
    want_rot = tc.write_at_pos(case.qkv_raw, case.lens, case.pasts, case.rope_positions(), case)      # (updates case.kc / vc)
    assert np.array_equal(want_rot.view(np.uint16), case.qkv_rot.view(np.uint16))
    assert np.array_equal(rot.view(np.uint16), want_rot.view(np.uint16)), "rotated rows"
    kp, vp = gk.pools()
    assert np.array_equal(kp, case.kc.pool), "K pages"
    assert np.array_equal(vp, case.vc.pool), "V pages"
    plain = pc.rotate(case.qkv_raw, case.lens, case.pasts, case.Hq, case.Hk)
    assert not np.array_equal(plain.view(np.uint16), want_rot.view(np.uint16))


@pytest.mark.parametrize("tpb", [16, 64])
def test_write_at_pos_with_arange_is_the_writer_at_an_offset(tpb):
    case = pc.Case([(0, 9), (10, 32), (63, 17), (10, 0), (63, 5)], 8, 2, tpb, seed=311 + tpb)
    a, b = GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx), GpuPagedKV(case.kc, case.vc, case.kidx, case.vidx)
    arange = np.concatenate([np.arange(n) for n in case.lens]).astype(np.int32)
    rot_a = _write(case, a, case.qkv_raw, None)
    rot_b = _write(case, b, case.qkv_raw, arange)
    assert np.array_equal(rot_a.view(np.uint16), rot_b.view(np.uint16))
    assert np.array_equal(rot_a.view(np.uint16), case.qkv_rot.view(np.uint16))
    for x, y in zip(a.pools(), b.pools()):
        assert np.array_equal(x, y)
    assert not np.array_equal(a.pools()[0], case.kc.pool)            # (something was written)


def _pattern_pools(B, pages, Hk, tpb, seed):
    """K and V pools filled with a seeded byte pattern (every byte of every page, tails included: any stray store shows), shuffled
    non-contiguous tables."""
    rng = np.random.default_rng(seed)
    n_pages = B * pages + 3
    kc, vc = kv4.PagedKV4(n_pages, Hk, D, tpb), kv4.PagedKV4(n_pages, Hk, D, tpb)
    kc.pool[:] = rng.integers(0, 256, kc.pool.shape, dtype=np.uint8)
    vc.pool[:] = rng.integers(0, 256, vc.pool.shape, dtype=np.uint8)
    kidx = rng.permutation(n_pages)[: B * pages].reshape(B, pages)
    vidx = rng.permutation(n_pages)[: B * pages].reshape(B, pages)
    return kc, vc, kidx, vidx


PATHS = [[0, 2, 3], [0, 1, 2], [0, 31], [0], [0, 5, 6, 7, 20, 31], [0, 7, 8, 9, 10, 11, 12, 13]]


@pytest.mark.parametrize("Hk", [1, 2, 8])
@pytest.mark.parametrize("tpb,base", [(16, 10), (64, 40)])
def test_compact_rows(Hk, tpb, base):
    """Paths [0, 2, 3] (slot 2 is read for j = 1 and written for j = 2), [0, 1, 2] (identity), [0, 31], a count of 1 and two longer
    ones in one batch, counts varying; base 10 at tokens_per_block 16 (the sources reach positions 10 ... 41: three pages; source
    and destination in different pages) and base 40 at 64 (one page edge); base differing per sequence.  The whole K and V
    pools, every page and tail, byte for byte."""
    from omniserve_amd.backend import fused_ext
    B, rows = len(PATHS), 32
    bases = np.asarray([base + (b % 2) for b in range(B)], np.int32)
    pages = (int(bases.max()) + rows) // tpb + 2
    kc, vc, kidx, vidx = _pattern_pools(B, pages, Hk, tpb, seed=17 * Hk + tpb)
    gk = GpuPagedKV(kc, vc, kidx, vidx)
    src = np.full((B, rows), -1, np.int32)
    counts = np.asarray([len(p) for p in PATHS], np.int32)
    for b, p in enumerate(PATHS):
        src[b, : len(p)] = p
    fused_ext.kv4_compact_rows(gk.table, to_dev(bases), to_dev(src), to_dev(counts), tpb, Hk)
    torch.cuda.synchronize()
    want_k = tc.compact_expected(kc.pool, kidx, tpb, Hk, kc.page_bytes, bases, src, counts)
    want_v = tc.compact_expected(vc.pool, vidx, tpb, Hk, vc.page_bytes, bases, src, counts)
    assert not np.array_equal(want_k, kc.pool)
    got_k, got_v = gk.pools()
    assert np.array_equal(got_k, want_k), "K pool: %d bytes differ" % (got_k != want_k).sum()
    assert np.array_equal(got_v, want_v), "V pool: %d bytes differ" % (got_v != want_v).sum()


def test_compact_rows_narrow_source_table_and_refusals():
    """max_rows = 3 (src [B, 3]); counts of 0 leave a sequence alone; the mirror refuses what the entry refuses."""
    from omniserve_amd.backend import fused_ext
    B, Hk, tpb = 3, 2, 16
    kc, vc, kidx, vidx = _pattern_pools(B, 4, Hk, tpb, seed=5)
    gk = GpuPagedKV(kc, vc, kidx, vidx)
    bases = np.asarray([14, 0, 30], np.int32)
    src = np.asarray([[0, 2, 3], [1, 2, 3], [0, 1, 3]], np.int32)
    counts = np.asarray([3, 0, 3], np.int32)
    fused_ext.kv4_compact_rows(gk.table, to_dev(bases), to_dev(src), to_dev(counts), tpb, Hk)
    torch.cuda.synchronize()
    got_k, got_v = gk.pools()
    assert np.array_equal(got_k, tc.compact_expected(kc.pool, kidx, tpb, Hk, kc.page_bytes, bases, src, counts))
    assert np.array_equal(got_v, tc.compact_expected(vc.pool, vidx, tpb, Hk, vc.page_bytes, bases, src, counts))
    with pytest.raises(ValueError):
        fused_ext.kv4_compact_rows(gk.table, to_dev(bases), to_dev(np.zeros((B, 33), np.int32)), to_dev(counts), tpb, Hk)
    with pytest.raises(RuntimeError):
        fused_ext.kv4_compact_rows(gk.table, to_dev(bases), to_dev(src.astype(np.int64)), to_dev(counts), tpb, Hk)
    with pytest.raises(RuntimeError):
        fused_ext.kv4_compact_rows(gk.table, to_dev(bases[:2]), to_dev(src), to_dev(counts), tpb, Hk)
    with pytest.raises(RuntimeError):
        fused_ext.kv4_compact_rows(gk.table, to_dev(bases), to_dev(src), to_dev(counts), 24, Hk)
