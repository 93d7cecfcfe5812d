"""The tree verify step without a GPU: the new C entries in the header and the ctypes table, the mirror's names and arities, the
acceptance rule over a tree (accept_paths), the ancestor masks (tree_masks), the mirror's named error before the library is touched,
the C entries' argument checks (they return before any launch), the coverage of the case grid and the fairness of the sibling
needles that tests/test_decode_tree_gpu.py runs."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import tree_verify_cases as tc
from tests import verify_attn_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["omni_decode_attention_tree_kv4", "omni_decode_attention_tree_kv4_workspace_bytes", "omni_kv4_prefill_write_at_pos",
       "omni_kv4_compact_rows"]


def _header_decl(name):
    src = open(os.path.join(ROOT, "include", "omniserve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    assert m, "%s is not declared in the header" % name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def test_surface():
    from omniserve_amd import _lib, runtime
    from omniserve_amd.backend import fused_ext
    for name in NEW:
        assert name in _lib.PROTOTYPES
        assert len(_header_decl(name)) == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(_lib.lib(), name)
    # the chain entry's argument list with the mask words behind past_lens
    multi, tree = _header_decl("omni_decode_attention_multi_kv4"), _header_decl("omni_decode_attention_tree_kv4")
    at = multi.index("const void* past_lens_i32") + 1
    assert tree == multi[:at] + ["const void* tree_mask_u32"] + multi[at:]
    # the writer at an offset with the RoPE offsets behind past_lens
    w, wp = _header_decl("omni_kv4_prefill_write_at"), _header_decl("omni_kv4_prefill_write_at_pos")
    at = w.index("const void* past_lens_i32") + 1
    assert wp == w[:at] + ["const void* rope_offsets_i32"] + w[at:]
    assert _header_decl("omni_kv4_compact_rows") == [
        "const void* kv_pointers_i64", "const void* base_lens_i32", "const void* src_i32", "const void* counts_i32", "int batch",
        "int max_blocks", "int tokens_per_block", "int num_kv_heads", "int head_dim", "int max_rows", "void* stream"]
    assert _lib.lib().omni_abi_version() == 4
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(fused_ext.decode_attention_tree_kv4) == [
        "q", "k_new", "v_new", "cu_seqlens_q", "past_lens", "tree_mask", "kv_pointers", "tokens_per_block", "max_seqlen_q",
        "max_past", "workspace"]
    at_ = sig(fused_ext.kv4_prefill_write_at)
    assert sig(fused_ext.kv4_prefill_write_at_pos) == at_[:3] + ["rope_offsets"] + at_[3:]
    assert sig(fused_ext.kv4_compact_rows) == ["kv_pointers", "base_lens", "src", "counts", "tokens_per_block", "num_kv_heads"]
    assert sig(fused_ext.decode_attention_tree_kv4_workspace_bytes) == sig(fused_ext.decode_attention_multi_kv4_workspace_bytes)
    assert sig(fused_ext.tree_masks) == ["parents"]
    assert fused_ext.DECODE_TREE_MAX_Q == 32 and fused_ext.DECODE_MULTI_MAX_Q == 8
    assert issubclass(fused_ext.DecodeTreeTooManyTokens, ValueError)
    assert sig(runtime.accept_paths) == ["parents", "tokens", "pred"]
    assert sig(runtime.DecodeRunner.verify_tree) == ["self", "tokens", "parents"]
    # default-off: extend() / verify() make today's calls
    assert inspect.signature(runtime.DecodeRunner._extend_rows).parameters["rope_offsets"].default is None


def test_accept_paths():
    from omniserve_amd.runtime import accept_lengths, accept_paths
    # chain parents: the verify step's rule (tests/test_decode_multi_cpu.py's table)
    draft = torch.tensor([[5, 1, 2, 3], [5, 7, 8, 9], [5, 7, 0, 9], [5, 7, 8, 0]])
    pred = torch.tensor([[9, 2, 3, 4], [7, 8, 9, 4], [7, 8, 9, 4], [7, 8, 9, 4]])
    path, m = accept_paths(torch.tensor(tc.chain(4)), draft, pred)
    assert path.dtype == torch.int64 and m.dtype == torch.int64
    assert torch.equal(m, accept_lengths(draft, pred)) and m.tolist() == [1, 4, 2, 3]      # row 0: full reject, m = 1
    assert path.tolist() == [[0, -1, -1, -1], [0, 1, 2, 3], [0, 1, -1, -1], [0, 1, 2, -1]]  # row 2: a match behind a mismatch
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 5, 8):
        d, p = torch.randint(0, 3, (64, n), generator=g), torch.randint(0, 3, (64, n), generator=g)
        path, m = accept_paths(tc.chain(n).tolist(), d, p)
        assert torch.equal(m, accept_lengths(d, p))
        for b in range(64):
            assert path[b].tolist() == list(range(int(m[b]))) + [-1] * (n - int(m[b]))
    # a tree: root -> {1, 2}, 1 -> {3}, 2 -> {4, 5, 6}
    parents = [-1, 0, 0, 1, 2, 2, 2]
    tokens = torch.tensor([[5, 7, 7, 8, 9, 9, 9],       # both children of the root match: the lowest index wins, then 3 matches
                           [5, 6, 7, 8, 1, 9, 9],       # child 2 matches; of its children 5 and 6 match: 5 wins
                           [5, 6, 6, 8, 9, 9, 9],       # no child of the root matches: matches further down are not reached
                           [5, 6, 7, 8, 1, 2, 3]])      # child 2 matches, none of its children does
    pred = torch.tensor([[7, 8, 9, 0, 0, 0, 0],
                         [7, 8, 9, 0, 0, 0, 0],
                         [7, 8, 9, 0, 0, 0, 0],
                         [7, 8, 9, 0, 0, 0, 0]])
    path, m = accept_paths(parents, tokens, pred)
    assert m.tolist() == [3, 3, 1, 2]
    assert path.tolist() == [[0, 1, 3, -1, -1, -1, -1], [0, 2, 5, -1, -1, -1, -1], [0, -1, -1, -1, -1, -1, -1],
                             [0, 2, -1, -1, -1, -1, -1]]


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("n", [1, 2, 9, 32])
def test_tree_masks(kind, n):
    from omniserve_amd.backend import fused_ext
    parents = tc.tree(kind, n, seed=n)
    want_m, want_d = tc.masks_depths(parents)
    mask, depth = fused_ext.tree_masks(torch.from_numpy(parents))
    assert mask.dtype == torch.int32 and mask.shape == (n,) and depth.shape == (n,)
    got = mask.numpy().view(np.uint32)
    assert np.array_equal(got, want_m) and np.array_equal(depth.numpy(), want_d)
    for i in range(n):
        assert (int(got[i]) >> i) & 1                                        # bit i set
        assert int(got[i]) >> (i + 1) == 0                                   # nothing behind the node
        if parents[i] >= 0:                                                  # ancestor closure
            assert int(got[i]) == int(got[parents[i]]) | 1 << i and depth[i] == depth[parents[i]] + 1
    both, both_d = fused_ext.tree_masks(torch.from_numpy(np.stack([parents, tc.chain(n)])))
    assert np.array_equal(both[0].numpy().view(np.uint32), want_m)
    assert both[1].numpy().view(np.uint32).tolist() == [(1 << (i + 1)) - 1 for i in range(n)]
    assert both_d[1].tolist() == list(range(n))


def test_tree_masks_refuses_bad_parents():
    from omniserve_amd.backend import fused_ext
    for bad in ([-1, 1], [-1, 0, 2], [-1, 0, 3], [0, 0], [-1, -1], [-1, 0, -2]):
        with pytest.raises(ValueError):
            fused_ext.tree_masks(torch.tensor(bad))
    with pytest.raises(fused_ext.DecodeTreeTooManyTokens):
        fused_ext.tree_masks(torch.tensor([-1] + list(range(32))))


def test_mirror_raises_its_named_error_before_touching_the_library(monkeypatch):
    from omniserve_amd import _lib
    from omniserve_amd.backend import fused_ext

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    q = torch.zeros((33, 8, 128), dtype=torch.float16)
    kv = torch.zeros((33, 2, 128), dtype=torch.float16)
    cu = torch.tensor([0, 33], dtype=torch.int32)
    past = torch.zeros(1, dtype=torch.int32)
    mask = torch.zeros(33, dtype=torch.int32)
    tab = torch.zeros((1, 2, 4), dtype=torch.int64)
    with pytest.raises(fused_ext.DecodeTreeTooManyTokens):
        fused_ext.decode_attention_tree_kv4(q, kv, kv, cu, past, mask, tab, 64, 33, 0)


def test_entry_checks_return_before_any_launch():
    from omniserve_amd import _lib
    h = _lib.lib()
    need = h.omni_decode_attention_tree_kv4_workspace_bytes(2, 8, 32, 1000)
    assert need == 16 * 2 * 32 * 8 * 130 * 4                    # 16 forced splits of f32 [128 + 2] per (sequence, token, head)
    assert h.omni_decode_attention_tree_kv4_workspace_bytes(2, 8, 32, 0) == need      # ... whatever the past
    assert h.omni_decode_attention_tree_kv4_workspace_bytes(2, 8, 40, 0) == need      # ... and cut at 32 tokens
    assert h.omni_decode_attention_tree_kv4_workspace_bytes(2, 8, 8, 0) == h.omni_decode_attention_multi_kv4_workspace_bytes(2, 8, 8, 0)
    assert h.omni_decode_attention_tree_kv4_workspace_bytes(0, 8, 4, 1000) == 0

    def call(max_q=32, head_dim=128, hq=8, hk=2, tpb=64, ks=1536, ws=1 << 20, ws_bytes=None, max_past=1000, batch=2, mask=1):
        return h.omni_decode_attention_tree_kv4(1, 1, 1, 1, 1536, ks, 1536, 1, 1, mask, 1, batch, 4, tpb, max_q, hq, hk, head_dim,
                                                max_past, ws, need if ws_bytes is None else ws_bytes, None)
    assert call(max_q=33) == -22
    assert call(mask=None) == -22
    assert call(ws=(1 << 20) + 8) == -22                    # misaligned workspace
    assert call(head_dim=64) == -22
    assert call(hq=7) == -22
    assert call(tpb=24) == -22
    assert call(ks=1 << 31) == -22
    assert call(max_past=-1) == -22
    assert call(ws=None) == -12
    assert call(ws_bytes=need // 16 - 1) == -12             # shorter than one split's partials
    assert call(batch=0) == 0 and call(max_q=0) == 0        # nothing to do: no launch
    # the chain entry keeps its bound
    assert h.omni_decode_attention_multi_kv4(1, 1, 1, 1, 1536, 1536, 1536, 1, 1, 1, 2, 4, 64, 9, 8, 2, 128, 1000, 1 << 20, need,
                                             None) == -22

    def write(offsets=1, past=1, rope_rows=64, max_seq_len=8):
        return h.omni_kv4_prefill_write_at_pos(1, 1, past, offsets, 1, 1, 16, 2, 4, 8, 2, 128, max_seq_len, 64, 1, rope_rows,
                                               1 << 20, None)
    assert write(offsets=None) == -22 and write(past=None) == -22 and write(rope_rows=4) == -22

    def compact(rows=4, tpb=16, hk=2, head_dim=128, src=1, batch=2, blocks=4):
        return h.omni_kv4_compact_rows(1, 1, src, 1, batch, blocks, tpb, hk, head_dim, rows, None)
    assert compact(rows=33) == -22 and compact(rows=0) == -22 and compact(tpb=24) == -22 and compact(head_dim=64) == -22
    assert compact(src=None) == -22 and compact(hk=0) == -22 and compact(blocks=0) == -22
    assert compact(batch=0) == 0


def test_case_grid_coverage():
    """Per family: every past of {0, 1, 63, 64, 65, 200} and every n of {1, 2, 8, 9, 17, 32} at least twice, a different tree on
    neighbouring sequences, every tree kind; the four families are verify_attn_cases' (ratios 1 / 4 / 7 / 8, tokens_per_block 16 /
    64), and together they meet every past with at least four different n."""
    assert sorted(tc.FAMILIES) == sorted(vc.FAMILIES)
    met = {}
    for name, (hq, hk, tpb, triples) in tc.FAMILIES.items():
        assert (hq, hk, tpb) == vc.FAMILIES[name][:3]
        for past in (0, 1, 63, 64, 65, 200):
            assert sum(p == past for p, _, _ in triples) >= 2, (name, past)
        for n in (1, 2, 8, 9, 17, 32):
            assert sum(m == n for _, m, _ in triples) >= 2, (name, n)
        assert max(n for _, n, _ in triples) == tc.MAX_Q
        assert {k for _, _, k in triples} == set(tc.KINDS), name
        assert all(a[2] != b[2] for a, b in zip(triples, triples[1:])), name
        for p, n, _ in triples:
            met.setdefault(p, set()).add(n)
    assert all(len(v) >= 4 for v in met.values()), met
    assert (16 // 2) * 32 == 256 and 7 * 32 == 224            # n = 32 at ratios 8 and 7: two row groups of 128, the second ragged
    case = tc.family("gqa7_tpb16")
    for b, par in enumerate(case.parents):                    # the generators give trees: parents[i] < i
        assert len(par) == case.lens[b] and (len(par) == 0 or par[0] == -1) and all(par[i] < i for i in range(1, len(par)))
    assert {(p, n) for p, n, _ in tc.MIXED_BATCH} >= {(200, 0), (0, 0), (0, 1)}
    a, b = case.depth[: case.lens[0]], tc.masks_depths(case.parents[0])[1]
    assert np.array_equal(a, b) and case.rope_positions()[0] == case.pasts[0]


def test_sibling_needles_are_fair():
    """Every row that may see its needle gives it > 0.99 of the softmax mass (f64); the rows aimed at a sibling's (or, for the root,
    a descendant's) fresh key exist, and the masked expectation with the chain's words is the oracle's causal attention."""
    from tests import paged_prefill_cases as pc
    nb = tc.SiblingNeedles()
    want, mass = nb.expected()
    assert nb.B == 154 and mass.shape == (154, 4, 8)
    blind = np.isnan(mass)
    # fresh key j >= 1 is seen by node j alone: 3 blind nodes each; the root key and the page keys by everyone
    assert blind.sum() == 3 * 3 * 8 and not blind[:151].any()
    for j in (1, 2, 3):
        assert [bool(blind[150 + j, i].all()) for i in range(4)] == [i != j for i in range(4)]
    assert np.nanmin(mass) > 0.99, "weakest needle holds %.4f of its row" % np.nanmin(mass)
    cm = np.tile(tc.masks_depths(tc.chain(4))[0], nb.B)
    chain_want = tc.expected_tree_attention(nb.q, nb.k_new, nb.v_new, nb.cu, nb.pasts, cm, nb.kc, nb.vc, nb.kidx, nb.vidx)
    oracle = pc.expected_attention(nb.q, nb.k_new, nb.v_new, nb.cu, nb.pasts, nb.kc, nb.vc, nb.kidx, nb.vidx)
    d = np.abs(oracle.astype(np.float64) - chain_want.astype(np.float64)).max()
    assert d <= 2e-3 * np.abs(chain_want.astype(np.float64)).max(), d
