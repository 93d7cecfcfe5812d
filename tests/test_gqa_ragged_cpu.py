"""Host side of the ragged GQA ratios (no GPU): the decode entries' argument validation lets ratios 3 / 5 / 6 / 7 / 10
through, still refuses a head count that is no multiple of the kv heads and head_dim 64, and LlamaConfig.yi_34b() has
Yi-34B's sizes.  Nothing is launched: with every pointer non-null the calls stop at the workspace check (0 bytes given:
-ENOMEM), which sits BEHIND the shape checks (-EINVAL) in all three hosts."""
import ctypes

import pytest

from omniserve_amd import _lib

EINVAL, ENOMEM = -22, -12
P = 1      # dummy non-null pointer: never dereferenced on these paths


def _dense(h, heads, kv_heads, head_dim=128):
    return h.omni_kv4_decode_attention(P, P, P, P, heads * head_dim, kv_heads * head_dim, P, P, 2, 4, heads, kv_heads,
                                       head_dim, 64, 200, P, 201, P, 0, None)


def _partial(h, heads, kv_heads, head_dim=128):
    ns = ctypes.c_int(0)
    return h.omni_kv4_decode_attention_partial(P, P, P, heads * head_dim, kv_heads * head_dim, P, P, 2, 4, heads, kv_heads,
                                               head_dim, 64, 200, P, 201, P, 0, ctypes.byref(ns), None)


def _fine_grained(h, heads, kv_heads, head_dim=128, kv8=False):
    args = (P, P, P, P, heads * head_dim, kv_heads * head_dim)
    if kv8:
        args += (P, P)
    # retrieval heads only: tables, flags, rank, lengths, no dynamic pages
    args += (P, None, P, P, P, None, 0, 0, 2, 4, 0, heads, kv_heads, kv_heads, 0, head_dim, 64, 0, 0, 0, 0, 200, P, 201, P,
             0, None)
    f = h.omni_kv8_decode_attention_per_tensor if kv8 else h.omni_kv4_decode_attention_fine_grained
    return f(*args)


ENTRIES = [_dense, _partial, _fine_grained, lambda h, *a: _fine_grained(h, *a, kv8=True)]


@pytest.mark.parametrize("entry", range(len(ENTRIES)))
@pytest.mark.parametrize("ratio", [1, 2, 3, 4, 5, 6, 7, 8, 10])
def test_any_ratio_passes_the_shape_checks(entry, ratio):
    h = _lib.lib()
    assert ENTRIES[entry](h, 2 * ratio, 2) == ENOMEM


@pytest.mark.parametrize("entry", range(len(ENTRIES)))
def test_what_is_still_refused(entry):
    h = _lib.lib()
    assert ENTRIES[entry](h, 7, 2) == EINVAL             # heads no multiple of the kv heads
    assert ENTRIES[entry](h, 14, 2, 64) == EINVAL        # head_dim 64
    assert ENTRIES[entry](h, 0, 2) == EINVAL


def test_level_3_entry_keeps_its_four_heads_per_wave_contract():
    """omni_kv4_decode_attention_f16_amax: num_heads % 4 == 0 stays (the wide merge's wave holds four heads); a ragged ratio
    with such a head count (Yi-34B: 56 / 8, its TP = 2 shard: 28 / 4) goes on to its two-launch form."""
    h = _lib.lib()

    def call(heads, kv_heads):
        return h.omni_kv4_decode_attention_f16_amax(P, P, P, P, P, heads * 128, kv_heads * 128, P, P, 2, 4, heads, kv_heads,
                                                    128, 64, 200, P, 201, P, 0, P, 4096, None)
    assert call(14, 2) == EINVAL
    assert call(28, 4) == ENOMEM and call(56, 8) == ENOMEM and call(32, 8) == ENOMEM


def test_yi_34b_preset():
    from omniserve_amd.runtime import LlamaConfig
    c = LlamaConfig.yi_34b()
    assert (c.hidden, c.layers, c.heads, c.kv_heads, c.head_dim, c.inter, c.vocab) == (7168, 60, 56, 8, 128, 20480, 64000)
    assert c.group_size == -1 and LlamaConfig.yi_34b(128).group_size == 128
    assert c.heads // c.kv_heads == 7
    assert (c.heads + 2 * c.kv_heads) * c.head_dim == 9216      # qkv projection's N
    assert 2 * c.inter == 40960                                 # gate_up projection's N
    # level 3's gate: hidden 7168 is past the row-free GEMVs' plans, the runner degrades to level 2 by itself
    assert _lib.lib().omni_gemm_rowfree_ok(2, c.hidden, c.heads * c.head_dim, c.inter, 0) == 0
    assert _lib.lib().omni_gemm_rowfree_ok(16, c.hidden, c.heads * c.head_dim, c.inter, 0) == 0
