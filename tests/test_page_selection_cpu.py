"""CPU-side checks of tests/page_selection_cases.py: every case is what its table entry claims, proved on the oracle alone
(oracle.kv4.topk_pages / paged_min_max_pool / page_selector).  No GPU."""
import numpy as np
import pytest

from oracle import kv4
from tests import page_selection_cases as pc

TOPK = pc.topk_cases()


def test_topk_pages_is_the_step_inside_select_topk_pages():
    """select_topk_pages = the budget arithmetic around topk_pages; topk_pages against a direct statement of the rule."""
    rng = np.random.default_rng(0)
    stats = rng.integers(-3, 4, (2, 3, 41 * 4)).astype(np.float16)          # few values: many ties
    got = kv4.select_topk_pages(stats, 64, 16, 6 * 64, 40 * 64 + 5)
    assert got.shape == (2, 3, 6) and got.dtype == np.int32
    assert np.array_equal(got, kv4.topk_pages(stats, 4, 41, 5))
    page = stats.reshape(2, 3, 41, 4).max(axis=-1).astype(np.float64)
    for b in range(2):
        for h in range(3):
            order = sorted(range(40), key=lambda p: (-page[b, h, p], p))
            assert got[b, h].tolist() == order[:5] + [40]
    # wider stats than the candidates need, k = 0, one page
    assert np.array_equal(kv4.topk_pages(stats, 4, 30, 5)[..., :5], kv4.topk_pages(stats[:, :, : 29 * 4], 4, 30, 5)[..., :5])
    assert kv4.topk_pages(stats, 4, 41, 0).tolist() == [[[40]] * 3] * 2
    assert kv4.topk_pages(stats[:, :, :4], 4, 1, 0).tolist() == [[[0]] * 3] * 2


def test_no_case_holds_a_nan_and_names_are_unique():
    names = [c.name for c in TOPK]
    assert len(set(names)) == len(names)
    for c in TOPK:
        assert c.scores.dtype == np.float16 and c.scores.shape[-1] == c.total_pages * c.subs, c.name
        assert not np.isnan(c.scores).any(), c.name
        assert 0 <= c.k <= c.n, c.name
        w = c.want()
        assert w.shape == c.scores.shape[:2] + (c.k + 1,) and (w[..., c.k] == c.n).all(), c.name
        assert ((w[..., : c.k] >= 0) & (w[..., : c.k] < c.n)).all(), c.name


@pytest.mark.parametrize("subs", [1, 4])
def test_tie_group_cases(subs):
    """800 pages tie at 1.0 with 50 above: more than 256 members (the radix select's page-bit passes decide) over at least 3
    values of page >> 8 (the third pass decides, and a thread's second and later loop trips hold members)."""
    row = pc.topk_case("ties_straddled_subs%d" % subs).page_scores()
    tied = np.flatnonzero(row[0, 0] == 1.0)
    assert np.array_equal(tied, np.arange(pc.TIE_LO, pc.TIE_HI)) and tied.size > 256
    assert len(set((tied >> 8).tolist())) >= 3
    for what, k in pc.TIE_K.items():
        c = pc.topk_case("ties_%s_subs%d" % (what, subs))
        ps = c.page_scores().astype(np.float32)
        assert ((ps > 1.0).sum(axis=-1) == pc.TIE_ABOVE).all() and ((ps == 1.0).sum(axis=-1) == 800).all()
        w = c.want()
        first, pages = c.tail
        assert first == pc.TIE_ABOVE
        assert (w[..., first: first + len(pages)] == np.asarray(pages)).all(), what
        assert (np.take_along_axis(ps, w[..., :first].astype(np.int64), -1) > 1.0).all()
        inside = {"straddled": 300, "whole": 800, "untouched": 0}[what]
        assert len(pages) == inside
        if what == "straddled":
            assert pages == tuple(range(100, 400)) and first + len(pages) == c.k
        if what == "whole":      # the k-th place is the group's last member: every key of its score is taken
            assert first + len(pages) == c.k
        if what == "untouched":
            assert c.k == first


@pytest.mark.parametrize("subs", [2, 4])
def test_all_equal_rows(subs):
    c = pc.topk_case("all_equal_subs%d" % subs)
    bits = c.scores.view(np.uint16)
    assert (bits[0, 0] == 0).all() and (bits[0, 1] == 0x8000).all()
    assert set(np.unique(bits[0, 2]).tolist()) == {0, 0x8000}
    mixed_pages = bits[0, 2, : c.n * subs].reshape(c.n, subs)
    assert (mixed_pages.min(axis=1) != mixed_pages.max(axis=1)).any()        # +0 and -0 inside one page
    assert c.k < c.n and c.n > 2 * 256
    assert (c.want()[..., : c.k] == np.arange(c.k)).all()


def test_few_valued_rows_cross_tie_groups():
    assert np.unique(pc.FEW_VALUES).size == 37 and not np.isnan(pc.FEW_VALUES).any()
    v = pc.FEW_VALUES.astype(np.float32)
    assert np.isinf(v).sum() == 2 and (v < 0).any() and (v == 65504.0).any()
    sub = np.abs(v[(v != 0) & np.isfinite(v)]) < 6.104e-5
    assert sub.sum() >= 4                                                    # subnormals of both signs
    crossed = set()
    for subs in (1, 4):
        for k in pc.FEW_KS:
            c = pc.topk_case("few_values_k%d_subs%d" % (k, subs))
            ps = c.page_scores().astype(np.float32)
            assert set(np.unique(ps).tolist()) <= set(v.tolist())
            w = c.want().astype(np.int64)
            for h in range(ps.shape[1]):
                kth = ps[0, h, w[0, h, k - 1]]
                taken = (ps[0, h, w[0, h, :k]] == kth).sum()
                if taken < (ps[0, h] == kth).sum():      # some pages of the k-th score are left out
                    crossed.add((subs, k, h))
    assert len(crossed) >= 5, crossed


def test_full_range_rows():
    c = pc.topk_case("full_range")
    assert np.isfinite(c.scores.astype(np.float32)).all()
    B, H, _ = c.scores.shape
    assert B * H >= 3
    rows = c.scores.reshape(B * H, -1)
    assert all(not np.array_equal(rows[i], rows[j]) for i in range(B * H) for j in range(i))
    bits = c.scores.view(np.uint16)
    assert len(np.unique(bits >> 10)) >= 60            # both signs, subnormals to the top exponent


def test_sizes_sub_chunk_counts_and_newest_page():
    have = {(c.n, c.k, c.subs) for c in TOPK if c.name.startswith("size_")}
    assert have == {(n, k, s) for n, k in pc.SIZES for s in (1, 4)}
    assert (14336, 1024) in pc.SIZES and (0, 0) in pc.SIZES
    for subs in pc.SUBS:
        c = pc.topk_case("subs%d" % subs)
        assert c.subs == subs
        B, H, _ = c.scores.shape
        per_page = c.scores[:, :, : c.n * subs].reshape(B, H, c.n, subs).astype(np.float32)
        top = per_page.max(axis=-1, keepdims=True)
        assert ((per_page == top).sum(axis=-1) == 1).all()                  # the maximum sits alone ...
        assert set(per_page.argmax(axis=-1).ravel().tolist()) == set(range(subs))     # ... in every position
        if subs > 1:
            assert (per_page.argmax(axis=-1)[0, 0] != per_page.argmax(axis=-1)[0, 1]).all()
    for subs in (2, 4):
        c = pc.topk_case("newest_inf_subs%d" % subs)
        assert np.isposinf(c.scores[:, :, c.n * subs:].astype(np.float32)).all()
        assert np.isfinite(c.scores[:, :, : c.n * subs].astype(np.float32)).any()
        assert (c.want()[..., : c.k] != c.n).all()


# ---- selector cases ------------------------------------------------------------------------------------------------------
def test_selector_specs_cover_the_issue_s_shapes():
    for tpb, sub in pc.SEL_SHAPES:
        for m in (1, 2):
            s = next(x for x in pc.SELECTOR_SPECS if x.name == "tpb%d_sub%d_m%d" % (tpb, sub, m))
            edge = pc.SEL_PAGES * tpb * m
            assert {edge - 1, edge, edge + 1, sub - 1, 0} == set(s.hist)
    assert {s.group for s in pc.SELECTOR_SPECS} == {2, 3}
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= {h for s in pc.SELECTOR_SPECS if s.tpb == 64 for h in s.hist}
    # sub-chunks of one selector workgroup: 256 and 512 are a second and a fourth trip of its 128-wide loop
    assert sorted({pc.SEL_PAGES * (t // s) for t, s in pc.SEL_SHAPES}) == [32, 64, 256, 512]
    assert any(s.rope_scale == 4.0 for s in pc.SELECTOR_SPECS)


@pytest.mark.parametrize("name", ["tpb64_sub8_m1", "tpb16_sub8_m2", "tpb64_sub8_rope_scale4"])
def test_selector_case_poison_and_zero_slots(name):
    """The pool writes the sub-chunks whose first token exists and nothing else; the oracle's selector reads only those (no NaN
    comes out), leaves streaming heads and the slots past a sequence's own sub-chunks at +0."""
    c = pc.selector_case(name)
    s = c.spec
    stats0 = c.pool0[:, c.stats_off:].view(np.uint16)
    assert (stats0 == pc.NAN_BITS).all() and np.isnan(stats0.view(np.float16)).all()
    assert np.array_equal(c.pool[:, : c.stats_off], c.pool0[:, : c.stats_off])
    subs = s.tpb // s.sub
    written = 0
    for b in range(c.B):
        for blk in range(c.pages):
            kmax, kmin = kv4.pool_views(c.pool[c.table[b, blk]], c.H, pc.D, s.tpb, s.sub)
            for sc in range(subs):
                exists = blk * s.tpb + sc * s.sub < s.hist[b]
                for view in (kmax, kmin):
                    assert np.isnan(view[sc]).all() != exists and np.isnan(view[sc]).any() != exists
                written += exists
    assert written == sum(c.n_sub(b) for b in range(c.B))
    assert not np.isnan(c.want).any()
    g = s.group
    assert (c.want.view(np.uint16)[:, g: 2 * g] == 0).all()                  # the streaming kv head's q heads
    for b in range(c.B):
        assert (c.want.view(np.uint16)[b, :, c.n_sub(b):] == 0).all()
        if c.n_sub(b):
            assert (c.want[b, :g, : c.n_sub(b)] != 0).all()
    assert 0 in s.hist and c.lengths.min() == 1


def test_rope_scale_case_differs_from_the_unscaled_scores():
    c = pc.selector_case("tpb64_sub8_rope_scale4")
    plain = kv4.page_selector(c.q, c.lengths, c.flags, c.rank, c.pool, c.table, c.Hk, c.H, c.spec.tpb, c.spec.sub,
                              pc.ROPE_BASE)
    scored = c.want != 0
    far = np.abs(pc.f16_key(plain) - pc.f16_key(c.want)) > 2         # beyond the selector's tolerance
    assert scored.sum() > 1000 and far[scored].mean() > 0.8


# ---- chain case ----------------------------------------------------------------------------------------------------------
def test_chain_case_needles_are_selected_with_margin():
    c = pc.chain_case()
    scores, pages = c.oracle()
    n, k, subs = c.total_pages - 1, c.k_best, pc.CHAIN_TPB // pc.CHAIN_SUB
    assert (n, k) == (40, 5) and pages.shape == (2, 8, 6)
    assert np.array_equal(pages, kv4.topk_pages(scores, subs, c.total_pages, k))
    page_scores = scores[:, :, : n * subs].reshape(2, 8, n, subs).max(axis=-1)
    key = pc.f16_key(page_scores)
    assert len(c.retrieval_q_heads) == 4
    for b in range(2):
        for h in range(8):
            if h not in c.retrieval_q_heads:
                assert (scores[b, h] == 0).all()
                continue
            chosen = pages[b, h, :k].tolist()
            assert len(c.needles[(b, h)]) == 2 and set(c.needles[(b, h)]) <= set(chosen), (b, h, c.needles[(b, h)], chosen)
            order = np.argsort(-key[b, h], kind="stable")
            assert order[:k].tolist() == chosen
            gaps = -np.diff(key[b, h, order[: k + 1]])           # k - 1 gaps inside the selection, then k-th against (k+1)-th
            print("sequence %d head %d: pages %s, gaps (ulp) %s" % (b, h, chosen, gaps.tolist()))
            assert (gaps >= pc.MARGIN_ULP).all(), (b, h, gaps)
    # the choice matters: the heads of one kv head choose different pages, and so do the sequences
    assert set(pages[0, 0, :k].tolist()) != set(pages[1, 0, :k].tolist())
    assert pages[0, 0, :k].tolist() != pages[0, 1, :k].tolist()
