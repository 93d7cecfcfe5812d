"""The multi-token decode step without a GPU: the acceptance rule, the three new C entries in the header and the ctypes table, the
mirror's named error, the C entry's argument checks (they return before any launch), and the fairness of the needle batch that
tests/test_decode_multi_gpu.py runs."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import paged_prefill_cases as pc
from tests import verify_attn_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["omni_decode_attention_multi_kv4", "omni_decode_attention_multi_kv4_workspace_bytes",
       "omni_decode_attention_multi_kv4_set_split_override"]


def test_accept_lengths():
    from omniserve_amd.runtime import accept_lengths
    draft = torch.tensor([[5, 1, 2, 3],      # nothing accepted: the first drafted token is not what the model says
                          [5, 7, 8, 9],      # all accepted
                          [5, 7, 0, 9],      # a match (9 behind pred 9) behind a mismatch must not count
                          [5, 7, 8, 0]])     # the last drafted token rejected
    pred = torch.tensor([[9, 2, 3, 4],
                         [7, 8, 9, 4],
                         [7, 8, 9, 4],
                         [7, 8, 9, 4]])
    m = accept_lengths(draft, pred)
    assert m.dtype == torch.int64 and m.tolist() == [1, 4, 2, 3]
    assert accept_lengths(draft[:, :1], pred[:, :1]).tolist() == [1, 1, 1, 1]      # n = 1: the pending token alone


def _header_decl(name):
    src = open(os.path.join(ROOT, "include", "omniserve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    assert m, "%s is not declared in the header" % name
    return [a for a in m.group(1).split(",") if a.strip()]


def test_surface():
    from omniserve_amd import _lib
    from omniserve_amd.backend import fused_ext
    from omniserve_amd.runtime import DecodeRunner
    for name in NEW:
        assert name in _lib.PROTOTYPES
        assert len(_header_decl(name)) == len(_lib.PROTOTYPES[name][1])
        assert hasattr(_lib.lib(), name)
    # the paged prefill entry's argument list + max_past, workspace, workspace_bytes in front of the stream
    paged, multi = _header_decl("omni_prefill_attention_paged_kv4"), _header_decl("omni_decode_attention_multi_kv4")
    norm = lambda a: " ".join(a.split())      # noqa: E731
    assert [norm(a) for a in multi[:len(paged) - 1]] == [norm(a) for a in paged[:-1]]
    assert [norm(a) for a in multi[len(paged) - 1:]] == ["int max_past", "void* workspace", "size_t workspace_bytes", "void* stream"]
    header = open(os.path.join(ROOT, "include", "omniserve_hip.h")).read()
    for name in NEW:      # each says that it is a project extension with no reference counterpart
        before = header[: header.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "Project extension" in comment and "no reference counterpart" in comment, name
    assert _lib.lib().omni_abi_version() == 4
    a = list(inspect.signature(fused_ext.decode_attention_multi_kv4).parameters)
    assert a == ["q", "k_new", "v_new", "cu_seqlens_q", "past_lens", "kv_pointers", "tokens_per_block", "max_seqlen_q", "max_past",
                 "workspace"]
    assert callable(DecodeRunner.verify)


def test_mirror_raises_its_named_error_before_touching_the_library(monkeypatch):
    from omniserve_amd import _lib
    from omniserve_amd.backend import fused_ext

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    q = torch.zeros((9, 8, 128), dtype=torch.float16)
    kv = torch.zeros((9, 2, 128), dtype=torch.float16)
    cu = torch.tensor([0, 9], dtype=torch.int32)
    past = torch.zeros(1, dtype=torch.int32)
    tab = torch.zeros((1, 2, 4), dtype=torch.int64)
    with pytest.raises(fused_ext.DecodeMultiTooManyTokens):
        fused_ext.decode_attention_multi_kv4(q, kv, kv, cu, past, tab, 64, 9, 0)
    assert issubclass(fused_ext.DecodeMultiTooManyTokens, ValueError)


def test_entry_checks_return_before_any_launch():
    from omniserve_amd import _lib
    h = _lib.lib()
    need = h.omni_decode_attention_multi_kv4_workspace_bytes(2, 8, 4, 1000)
    assert need >= 16 * 2 * 4 * 8 * 130 * 4                     # 16 forced splits of f32 [128 + 2] per (sequence, token, head)
    assert h.omni_decode_attention_multi_kv4_workspace_bytes(2, 8, 4, 0) == need      # ... whatever the past
    assert h.omni_decode_attention_multi_kv4_workspace_bytes(0, 8, 4, 1000) == 0

    def call(max_q=4, head_dim=128, hq=8, hk=2, tpb=64, ks=1536, ws=1 << 20, ws_bytes=None, max_past=1000, batch=2):
        return h.omni_decode_attention_multi_kv4(1, 1, 1, 1, 1536, ks, 1536, 1, 1, 1, batch, 4, tpb, max_q, hq, hk, head_dim,
                                                 max_past, ws, need if ws_bytes is None else ws_bytes, None)
    assert call(max_q=9) == -22
    assert call(head_dim=64) == -22
    assert call(hq=7) == -22
    assert call(tpb=24) == -22
    assert call(tpb=8) == -22
    assert call(ks=1 << 31) == -22
    assert call(ks=1532) == -22
    assert call(max_past=-1) == -22
    assert call(ws=None) == -12
    assert call(ws_bytes=need // 16 - 1) == -12             # shorter than one split's partials
    assert call(batch=0) == 0 and call(max_q=0) == 0        # nothing to do: no launch


def test_every_family_covers_every_value_three_times():
    """The grid is thinned per GQA family: about 32 pairs in each, every past and every len_q at least three times in each."""
    union = set()
    for name, (hq, hk, tpb, pairs) in vc.FAMILIES.items():
        assert 30 <= len(pairs) <= 34 and len(set(pairs)) == len(pairs), name
        for past in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 200):
            assert sum(p == past for p, _ in pairs) >= 3, (name, past)
        for n in (1, 2, 3, 5, 8):
            assert sum(m == n for _, m in pairs) >= 3, (name, n)
        assert max(n for _, n in pairs) <= vc.MAX_Q
        union |= set(pairs)
    assert len(union) == 55                                      # together: the whole past x len_q product
    assert sorted(hq // hk for hq, hk, _, _ in vc.FAMILIES.values()) == [1, 4, 7, 8]
    assert sorted(tpb for _, _, tpb, _ in vc.FAMILIES.values()) == [16, 16, 64, 64]
    full = {name: sorted(p for p, n in pairs if n == 8) for name, (_, _, _, pairs) in vc.FAMILIES.items()}
    for name in ("gqa8_tpb64", "gqa7_tpb16"):                   # several row tiles against no past, a tile edge, 128 and 200
        assert {0, 128, 200} <= set(full[name]) and {63, 64} & set(full[name]), (name, full[name])


def test_needle_batch_is_fair():
    """Every row that may see its needle gives it > 0.99 of the softmax mass (f64), the rows aimed at a fresh key behind them
    exist (and see something else), and the hand-written expectation agrees with the oracle's varlen attention."""
    nb = vc.NeedleBatch()
    want, mass = nb.expected()
    assert nb.B == 153 and mass.shape == (153, 3, 8)
    blind = np.isnan(mass)
    assert blind.sum() == (2 + 1) * 8                          # fresh key j, rows i < j: (j, i) = (1, 0), (2, 0), (2, 1)
    assert blind[151, 0].all() and blind[152, 0].all() and blind[152, 1].all()
    assert np.nanmin(mass) > 0.99, "weakest needle holds %.4f of its row" % np.nanmin(mass)
    oracle = pc.expected_attention(nb.q, nb.k_new, nb.v_new, nb.cu, nb.pasts, nb.kc, nb.vc, nb.kidx, nb.vidx)
    d = np.abs(oracle.astype(np.float64) - want.astype(np.float64)).max()
    assert d <= 2e-3 * np.abs(want.astype(np.float64)).max(), d
