"""CPU-side checks of the prefill pair that continues from the KV4 pages: the expected-value builder of
tests/paged_prefill_cases.py against the two oracles it must reduce to, the declared symbols, the Python surface and the host-side
refusals of the C entries (which return before any launch: no GPU needed)."""
import copy
import inspect
import os
import re

import numpy as np
import pytest

from oracle import attention as oa
from oracle import kv4
from tests import paged_prefill_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expected_builder_with_no_past_is_the_fresh_causal_attention():
    case = pc.Case([(0, 40), (0, 1), (0, 0), (0, 70)], 8, 2, 16, seed=1)
    q, k, v = case.split(case.qkv_rot)
    want = oa.varlen_attention(q, k, v, case.cu, case.cu, causal=True)
    got = pc.case_expected_attention(case)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def test_expected_builder_with_one_query_is_the_decode_oracle():
    """len_q = 1: the same keys, values and mask as oracle.kv4.decode_attention(emulate_fp16=False) on the same pools.  The two
    differ in the decode oracle's normaliser 1 / (sum + 1e-6) (the reference kernel's) against the plain 1 / sum, and in f32
    against f64 softmax arithmetic.  sum >= 1 (the row maximum contributes exp(0)), so the first term changes every output by a
    relative 1e-6 / (sum + 1e-6) <= 1e-6; the f32 roundings of at most ~200 products and sums add a few 1e-7 relative to the head's
    largest element: 1e-5 covers both with room.  The bound is on the values BEFORE each oracle's final rounding to fp16; after it,
    a pair within 1e-5 is either the same fp16 number or sits astride a rounding boundary and comes out one fp16 step apart.
    So: every element agrees to 1e-5 of the head's largest element or is the neighbouring fp16 value, and the neighbours are
    rare (a boundary within 1e-5 relative of a value whose fp16 spacing is >= 2^-11 relative: under 5 % of the elements)."""
    pairs = [(1, 1), (15, 1), (16, 1), (63, 1), (64, 1), (65, 1), (130, 1), (200, 1)]
    case = pc.Case(pairs, 8, 2, 64, seed=2)
    got = pc.case_expected_attention(case).astype(np.float64)
    q, k, v = case.split(case.qkv_raw)              # the decode oracle rotates q and k itself (position = past)
    kc, vc = copy.copy(case.kc), copy.copy(case.vc)
    kc.pool, vc.pool = case.kc.pool.copy(), case.vc.pool.copy()      # (it appends the token to the pools it is given)
    want16 = kv4.decode_attention(q, k, v, case.pasts + 1, kc, vc, case.kidx, case.vidx, pc.ROPE_BASE, emulate_fp16=False)
    want = want16.astype(np.float64)
    head_max = np.abs(want).max(axis=-1, keepdims=True)
    close = np.abs(got - want) <= 1e-5 * head_max
    step = np.spacing(np.abs(want16)).astype(np.float64)                # fp16 spacing at the expected value
    neighbour = np.abs(got - want) <= step * 1.0000001
    print("elements beyond 1e-5: %d of %d (all neighbouring fp16 values: %s)" % ((~close).sum(), close.size,
                                                                                bool((close | neighbour).all())))
    assert (close | neighbour).all(), "max |d| / head max = %.3g" % float((np.abs(got - want) / head_max).max())
    assert (~close).mean() < 0.05


def _header_decl(name):
    src = open(os.path.join(ROOT, "include", "omniserve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, "include/omniserve_hip.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_both_entries_and_fused_ext_exposes_them():
    args = _header_decl("omni_kv4_prefill_write_at")
    plain = _header_decl("omni_kv4_prefill_write")
    assert len(args) == len(plain) + 1 and any("past_lens_i32" in a for a in args)
    assert [a for a in args if "past_lens_i32" not in a] == plain       # the same arguments plus past_lens
    assert len(_header_decl("omni_prefill_attention_paged_kv4")) == 18
    from omniserve_amd import _lib
    assert len(_lib.PROTOTYPES["omni_kv4_prefill_write_at"][1]) == len(args)
    assert len(_lib.PROTOTYPES["omni_prefill_attention_paged_kv4"][1]) == 18
    from omniserve_amd.backend import fused_ext
    w = inspect.signature(fused_ext.kv4_prefill_write_at).parameters
    assert list(w)[:10] == ["qkv", "seq_lens", "past_lens", "padding_offset", "kv_pointers", "head_num", "kv_head_num",
                            "max_seq_len", "tokens_per_block", "max_total_len"]
    a = inspect.signature(fused_ext.prefill_attention_paged_kv4).parameters
    assert list(a)[:8] == ["q", "k_new", "v_new", "cu_seqlens_q", "past_lens", "kv_pointers", "tokens_per_block",
                           "max_seqlen_q"]


def test_entries_refuse_bad_arguments_before_any_launch():
    from omniserve_amd import _lib
    h = _lib.lib()
    assert h.omni_abi_version() == 4

    def attn(head_dim=128, tpb=64, hq=8, hk=2, ks=1536, vs=1536, batch=2, max_q=16, out=1):
        return h.omni_prefill_attention_paged_kv4(out, 1, 1, 1, 1536, ks, vs, 1, 1, 1, batch, 4, tpb, max_q, hq, hk, head_dim,
                                                  None)
    assert attn(head_dim=64) == -22
    assert attn(tpb=8) == -22 and attn(tpb=24) == -22 and attn(tpb=0) == -22
    assert attn(hq=7, hk=2) == -22
    assert attn(ks=1 << 31) == -22 and attn(vs=1 << 31) == -22          # byte stride >= 2^32
    assert attn(out=None) == -22
    assert attn(batch=0) == 0 and attn(max_q=0) == 0                     # no query token: success, nothing launched

    def write(past=1, head_dim=128, tpb=64, hq=8, hk=2, rope_rows=4096, max_len=16):
        return h.omni_kv4_prefill_write_at(1, 1, past, 1, 1, 32, 2, 4, hq, hk, head_dim, max_len, tpb, 1, rope_rows, 1 << 20, None)
    assert write(past=None) == -22
    assert write(head_dim=64) == -22 and write(tpb=24) == -22 and write(hq=7) == -22
    assert write(rope_rows=8, max_len=16) == -22                         # the table does not even cover the call's own tokens


def test_python_surface_refuses_what_the_kernel_does_not_do():
    import torch
    from omniserve_amd.backend import fused_ext
    q = torch.zeros((4, 4, 128), dtype=torch.float16)
    kv = torch.zeros((4, 2, 128), dtype=torch.float16)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    past = torch.zeros((1,), dtype=torch.int32)
    tab = torch.zeros((1, 2, 4), dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        fused_ext.prefill_attention_paged_kv4(q, kv, kv, cu, past, tab, 64, 4, causal=False)
    with pytest.raises(NotImplementedError):
        fused_ext.prefill_attention_paged_kv4(q, kv, kv, cu, past, tab, 64, 4, head_mask_type=torch.zeros(4, dtype=torch.int32),
                                              streaming_info=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError):          # host tensors: there is no CPU path
        fused_ext.prefill_attention_paged_kv4(q, kv, kv, cu, past, tab, 64, 4)
