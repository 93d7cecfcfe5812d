"""Decode attention (kv4_decode_flash_kernel and its merges) under PEAKED and SHIFTED score profiles with FORCED KV splits:
tests/decode_score_profiles.py plants one dominant token at a chosen position (first / last token of a split, of a page, of a
32-token tile, the last history token, the current token), lets the scores climb or fall by ~60 over the history, or shifts all
of them by +-200, and omni_kv4_decode_set_split_override pins the split geometry, so a token that is dropped, masked, read from
the wrong slot or weighted through a wrong rescale fails loudly.  Every output is held to tests.util.assert_attention_close at
the project's 1e-3 bar against the f64 expected values; appended rows are byte-identical to the oracle's.  The same profiles run
through the in-launch merge (fused_ext.decode_attention_f16_amax / decode_attention_quant_fuse_sum), the fine-grained (dense and
sparse) and the per-tensor KV8 instantiations."""
import numpy as np
import pytest
import torch

from oracle import elementwise as oe
from oracle import kv4
from tests import decode_score_profiles as dp
from tests.test_fine_grained_gpu import Case as FgCase
from tests.util import GpuPagedKV, assert_attention_close, dev, to_dev

pytestmark = pytest.mark.gpu

D, ROPE_BASE = dp.D, dp.ROPE_BASE


class forced_splits:
    """omni_kv4_decode_set_split_override(n) for the block, reset to 0 (the planner decides) behind it."""

    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        from omniserve_amd import _lib
        self.lib = _lib.lib()
        self.lib.omni_kv4_decode_set_split_override(self.n)

    def __exit__(self, *exc):
        self.lib.omni_kv4_decode_set_split_override(0)
        return False


def _check_output(c, got, what):
    """Per sequence (the message names the profile), then the planted tokens: the gain-1 head's output IS the needle's V row."""
    for b in range(c.B):
        assert_attention_close(got[b], c.want[b].astype(np.float32), "%s %s: sequence %d %r" % (what, c.name, b, c.seqs[b]))
    for b, nt in c.needles:
        for hk in range(c.Hk):
            hq = hk * c.g
            nv = c.needle_v[(b, hq)].astype(np.float64)
            d = np.linalg.norm(got[b, hq].astype(np.float64) - nv) / np.linalg.norm(nv)
            where = "the current token" if nt == c.seqs[b].T else "token %d (slot %d of page %d, token %d of split %d)" % (
                nt, nt % c.tpb, nt // c.tpb, nt % dp.split_tokens(c.context, max(c.nsplit, 1)),
                nt // dp.split_tokens(c.context, max(c.nsplit, 1)))
            assert d <= 1e-2, "%s %s: sequence %d, head %d lost %s: output is %.3g (relative) away from its V row" % (
                what, c.name, b, hq, where, d)


def _check_pools(c, gk, what):
    kp, vp = gk.pools()
    assert np.array_equal(kp, c.kc.pool), "%s %s: K pages differ after the append" % (what, c.name)
    assert np.array_equal(vp, c.vc.pool), "%s %s: V pages differ after the append" % (what, c.name)


# ---- dense KV4 through fused_attention_pure_dense.single_query_attention ----------------------------------------------------------
@pytest.mark.parametrize("name", list(dp.DENSE))
def test_dense_profiles(name):
    import omniserve_backend.fused_attention_pure_dense as fa
    c = dp.case(name)
    gk = GpuPagedKV(c.kc0, c.vc0, c.kidx, c.vidx)
    with forced_splits(c.nsplit):
        out = fa.single_query_attention(to_dev(c.q), to_dev(c.k), to_dev(c.v), gk.table, to_dev(c.lens), None, 65536, c.tpb,
                                        c.Hk * D // 2, c.context, D, ROPE_BASE, True, True, True)
        torch.cuda.synchronize()
    _check_output(c, out.cpu().numpy().astype(np.float32), "dense")
    _check_pools(c, gk, "dense")


# ---- the in-launch merge (LASTM) and the merge fused into the quantiser ------------------------------------------------------
@pytest.mark.parametrize("name", list(dp.MERGE))
def test_in_launch_merge_f16_amax(name):
    from omniserve_amd.backend import fused_ext
    c = dp.case(name)
    B = c.B
    gk = GpuPagedKV(c.kc0, c.vc0, c.kidx, c.vidx)
    out = torch.full((B, c.Hq * D), 7.0, dtype=torch.float16, device=dev())
    amax = fused_ext.new_amax_slots(B, dev())
    with forced_splits(c.nsplit):
        fused_ext.decode_attention_f16_amax(out, amax, to_dev(c.q), to_dev(c.k), to_dev(c.v), gk.table, to_dev(c.lens), c.tpb,
                                            c.context, ROPE_BASE, single_launch=True)
        torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float32).reshape(B, c.Hq, D)
    _check_output(c, got, "in-launch merge")
    _check_pools(c, gk, "in-launch merge")
    rows = fused_ext.amax_rows(amax, B).cpu().numpy()
    assert np.array_equal(rows, np.abs(got).reshape(B, -1).max(axis=1)), "row maxima are not those of the stored output"
    ref_max = np.abs(c.want.astype(np.float32)).reshape(B, -1).max(axis=1)
    assert (np.abs(rows - ref_max) <= 1e-3 * ref_max).all(), "row maxima %s vs expected %s" % (rows, ref_max)
    assert not fused_ext._tickets(dev()).any(), "tickets must be zero after the call"


@pytest.mark.parametrize("name", list(dp.MERGE))
def test_merge_quant_fuse_sum(name):
    """The quantised output against oracle.elementwise's codes of the EXPECTED output: the 1e-3 bar on the values and on the row
    maximum moves a code by at most 0.127 + 0.127 < 1, so codes agree within 1; the scale is h(amax / 127) of a maximum within
    1e-3 (plus one fp16 rounding, 2^-11)."""
    from omniserve_amd.backend import fused_ext
    c = dp.case(name)
    B = c.B
    gk = GpuPagedKV(c.kc0, c.vc0, c.kidx, c.vidx)
    out = torch.zeros((B, c.Hq * D), dtype=torch.int8, device=dev())
    sm = torch.zeros((B,), dtype=torch.float16, device=dev())
    sc = torch.zeros((B,), dtype=torch.float16, device=dev())
    with forced_splits(c.nsplit):
        fused_ext.decode_attention_quant_fuse_sum(out, to_dev(c.q), to_dev(c.k), to_dev(c.v), gk.table, to_dev(c.lens), c.tpb,
                                                  c.context, ROPE_BASE, sm, sc)
        torch.cuda.synchronize()
    q_ref, s_ref, _ = oe.quant_per_token(c.want.reshape(B, -1), fuse_sum=True)
    diff = np.abs(out.cpu().numpy().astype(np.int32) - q_ref.astype(np.int32))
    print("merge + quant %s: largest code difference %d, codes that differ %d of %d" % (name, diff.max(), (diff > 0).sum(), diff.size))
    assert diff.max() <= 1, "codes differ by %d" % diff.max()
    s_got, s_want = sc.cpu().numpy().astype(np.float64), s_ref.astype(np.float64)
    assert (np.abs(s_got - s_want) <= 1.5e-3 * s_want).all(), "scales %s vs %s" % (s_got, s_want)
    _check_pools(c, gk, "merge + quant")


# ---- fine-grained (FG instantiation) and per-tensor KV8: the pool builders of tests/test_fine_grained_gpu.py ----------------------
def _fg_fill(c, retr_profiles, strm_profiles, seed):
    """History of every (sequence, kv head) written through FineGrainedKV.write with a controlled score profile (a retrieval head
    stores every token, a streaming head only pos < sink or pos >= len - local, as the prefill writer does), mirrored to the GPU.
    -> q, k, v, needles {(b, hk): token index}."""
    rng = np.random.default_rng(seed)
    B, Hq, Hk = c.B, c.Hq, c.Hk
    g = Hq // Hk
    q = np.zeros((B, Hq, D), np.float16)
    k = np.zeros((B, Hk, D), np.float16)
    v = rng.standard_normal((B, Hk, D)).astype(np.float16)
    needles = {}
    for b in range(B):
        T = c.seq_lens[b]
        for hk in range(Hk):
            kind, arg = (retr_profiles if c.flags[hk] else strm_profiles)[b]
            a, cur, needle = dp.profile_scores(kind, arg, T, rng)
            q0, u = dp.unit_query(rng, T)
            for j in range(g):
                q[b, hk * g + j] = (np.float32(dp.GAINS[j]) * q0.astype(np.float32)).astype(np.float16)
            K = (a[:, None] * u[None, :] + 0.02 * rng.standard_normal((T, D))).astype(np.float16)
            V = rng.standard_normal((T, D)).astype(np.float16)
            k[b, hk] = (cur * q0.astype(np.float64) + 0.02 * rng.standard_normal(D)).astype(np.float16)
            if needle is not None:
                needles[(b, hk)] = needle
                V[needle] = dp.needle_v_row(hk)
            for t in range(T):
                if c.flags[hk] or t < c.sink or t >= T - c.local:
                    c.fg.write(b, hk, t, K[t], V[t])
    c.g_retr.kpool.copy_(to_dev(c.rk.pool)); c.g_retr.vpool.copy_(to_dev(c.rv.pool))
    c.g_strm.kpool.copy_(to_dev(c.sk.pool)); c.g_strm.vpool.copy_(to_dev(c.sv.pool))
    return q, k, v, needles


def _fg_decode(c, q, k, v, dyn=None):
    """One decode call of the family the case was built for (KV4 fine-grained or per-tensor KV8; dense or sparse), as
    tests/test_fine_grained_gpu.py::Case.decode makes it, with the given q / k / v.  -> (got f32, expected fp16)."""
    lens = np.asarray(c.seq_lens, np.int32) + 1
    want = kv4.decode_attention_fine_grained(q, k, v, lens, c.fg, ROPE_BASE, 1.0, dyn)
    qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
    kv4_mode = c.kv8 is None
    common = (c.tpb, c.nr * c.row, c.ns * c.row, c.sink, c.local, c.sink_blocks, c.local_blocks, c.nr, c.ns,
              int(lens.max()), D, ROPE_BASE, 1.0, True, kv4_mode, kv4_mode)
    tabs = (c.g_retr.table, c.g_strm.table, c.flags_d, c.rank_d)
    if kv4_mode:
        import omniserve_backend.fused_attention_fine_grained_dense as fad
        import omniserve_backend.fused_attention_fine_grained_sparse as fas
        if dyn is None:
            out = fad.single_query_attention(qd, kd, vd, *tabs, to_dev(lens), None, 65536, *common, 2048)
        else:
            out = fas.single_query_attention(qd, kd, vd, *tabs, to_dev(dyn), to_dev(lens), None, 65536, *common,
                                             c.sub_chunk, c.nr * D, 2048)
    else:
        import omniserve_backend.fused_attention_per_tensor_dense as fpd
        import omniserve_backend.fused_attention_per_tensor_sparse as fps
        if dyn is None:
            out = fpd.single_query_attention(qd, kd, vd, c.qo_d, c.oq_d, *tabs, to_dev(lens), None, 65536, *common, 2048)
        else:
            out = fps.single_query_attention(qd, kd, vd, c.qo_d, c.oq_d, *tabs, to_dev(dyn), to_dev(lens), None, 65536,
                                             *common, c.sub_chunk, c.nr * D, 2048)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float32), want


def _needle_distance(c, got, b, hk, nt):
    """Relative distance of the gain-1 head's output from the planted token's V row (as the cache holds it)."""
    nv = c.fg.read(b, hk, [nt])[1][0].astype(np.float64)
    hq = hk * (c.Hq // c.Hk)
    return float(np.linalg.norm(got[b, hq].astype(np.float64) - nv) / np.linalg.norm(nv))


def _check_fg(c, got, want, needles, absent, what):
    for b in range(c.B):
        assert_attention_close(got[b], want[b].astype(np.float32), "%s: sequence %d" % (what, b))
    for (b, hk), nt in needles.items():
        d = _needle_distance(c, got, b, hk, nt)
        if (b, hk) in absent:
            assert d >= 0.5, "%s: sequence %d, kv head %d attends token %d, which is outside its attended set (%.3g)" % (
                what, b, hk, nt, d)
        else:
            assert d <= 1e-2, "%s: sequence %d, kv head %d lost token %d (slot %d of page %d): %.3g away from its V row" % (
                what, b, hk, nt, nt % c.tpb, nt // c.tpb, d)
    c.check_pools(what)


FG_T, FG_TPB, FG_SINK, FG_LOCAL = 216, 16, 16, 48      # ring: 1 sink page + 4 local pages; window = tokens 169 .. 215


def test_fine_grained_dense_profiles():
    """Retrieval heads (kv heads 0, 3): needle at a page edge (last slot, first slot), climb, needle at the last history token.
    Streaming heads (1, 2): needle in the sink block; at the last slot of the ring's last page (207) and the first slot of the
    page that wraps to the ring's start (208); just outside the local window (168: stored in the ring, must not be read)."""
    c = FgCase([FG_T] * 5, 8, [1, 0, 0, 1], FG_TPB, FG_SINK, FG_LOCAL, seed=1)
    retr = [("needle", FG_TPB - 1), ("needle", FG_TPB), ("climb", dp.CLIMB), ("needle", "last"), ("descend", dp.CLIMB)]
    strm = [("needle", 3), ("needle", 207), ("needle", 208), ("needle", FG_T - FG_LOCAL), ("needle", FG_T - FG_LOCAL + 1)]
    assert kv4.ring_block(208 // FG_TPB, c.sink_blocks, c.local_blocks) == c.sink_blocks      # the wrap
    assert kv4.ring_block(207 // FG_TPB, c.sink_blocks, c.local_blocks) == c.sink_blocks + c.local_blocks - 1
    q, k, v, needles = _fg_fill(c, retr, strm, seed=2)
    got, want = _fg_decode(c, q, k, v)
    absent = {(3, 1), (3, 2)}
    _check_fg(c, got, want, needles, absent, "fine-grained dense profiles")


@pytest.mark.parametrize("nsplit", [7])
@pytest.mark.parametrize("kv8", [False, True], ids=["kv4", "kv8"])
def test_fine_grained_and_kv8_forced_splits(kv8, nsplit):
    """T = 700, pages of 64, 7 forced splits of 112 tokens through the FG instantiation (KV4) and the per-tensor KV8 one: needles at
    the page edge (63, 64) and the split edge (111, 112), climb, offset.  KV8: static scales 0.15 (K) / 0.035 (V) hold the
    profiles without saturating (|k| <= 60 * 0.3 = 18 < 19); its offset is 50 for the same reason."""
    T, tpb = 700, 64
    st = dp.split_tokens(T + 1, nsplit)
    off = 50.0 if kv8 else dp.OFFSET
    retr = [("needle", tpb - 1), ("needle", tpb), ("needle", st - 1), ("needle", st), ("climb", dp.CLIMB), ("offset", off)]
    strm = [("sink_recency", None)] * 6
    c = FgCase([T] * 6, 8, [1, 0], tpb, 128, 256, seed=3 + kv8, kv8_scales=(0.15, 0.035) if kv8 else None)
    q, k, v, needles = _fg_fill(c, retr, strm, seed=5 + kv8)
    with forced_splits(nsplit):
        got, want = _fg_decode(c, q, k, v)
    _check_fg(c, got, want, needles, set(), "forced %d splits, %s" % (nsplit, "per-tensor KV8" if kv8 else "fine-grained KV4"))


def test_fine_grained_sparse_profiles():
    """Selected pages (one list per q head, in selection order): a needle inside a selected page, at the last slot of a selected
    page, inside a page that is NOT selected (its weight must be absent), and a climb over the selected pages."""
    P, sub = 4, 8
    c = FgCase([FG_T] * 4, 8, [1, 1], FG_TPB, FG_SINK, FG_LOCAL, seed=7, sub_chunk=sub)
    retr = [("needle", 100), ("needle", 111), ("needle", 100), ("climb", dp.CLIMB)]
    q, k, v, needles = _fg_fill(c, retr, retr, seed=8)
    last = (FG_T - 1) // FG_TPB
    pages = [[2, 6, 9, last], [6, 2, 9, last], [2, 5, 9, last], [1, 5, 9, last]]
    dyn = np.zeros((c.B, c.Hq, P), np.int32)
    for b in range(c.B):
        dyn[b, :, :] = pages[b]
    got, want = _fg_decode(c, q, k, v, dyn)
    absent = {(2, 0), (2, 1)}
    _check_fg(c, got, want, needles, absent, "fine-grained sparse profiles")
