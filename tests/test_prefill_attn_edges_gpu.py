"""Prefill attention off the equal-length causal path, vs the f64 oracle at the project's bar (assert_attention_close, 1e-3 per
output vector; rows the mask leaves without a key must be exact zeros).  The cases live in tests/prefill_edge_cases.py:

  a  unequal q / k lengths per sequence: the bottom-right aligned diagonal and the Lambda window follow qpos = qrow + len_k - len_q
  b  non-causal, through flash_attn_varlen_func (whose default it is)
  c  a class from {0, -1, -2} and a window of its own per q head, under every head-to-XCD split
  d  windows that mean "everything" (1 << 24 ... 2**31 - 1 tokens or 128-token blocks): the int32 window arithmetic
  e  near one-hot softmax with the row maximum climbing (or standing still) from key tile to key tile
  f  max_seqlen_q beyond the longest sequence, zero-length sequences, three different token strides
  g  a sentinel band behind `out` through the two C entries
"""
import numpy as np
import pytest
import torch

from tests import prefill_edge_cases as pe
from tests.util import assert_attention_close, to_dev

pytestmark = pytest.mark.gpu

D = 128


@pytest.fixture(autouse=True, params=[0, 1, 2], ids=["rows16", "rows32", "pingpong"])
def kernel_form(request):
    """Every case runs on the three forms of the kernel (see tests/test_prefill_attn_gpu.py)."""
    from omniserve_amd import _lib
    _lib.lib().omni_prefill_set_variant(request.param)
    yield request.param
    _lib.lib().omni_prefill_set_variant(0)


def _ids(cases):
    return [c["name"] for c in cases]


def _device_inputs(q, k, v, layout="views"):
    """views: q is a token-strided view of a wider buffer, k and v are the two halves of one fused buffer (the token counts of
    the two sides differ, so one qkv buffer cannot hold them).  q_of_qkv (len_q == len_k): q a view of the fused qkv buffer,
    k and v separate contiguous tensors: three different token strides."""
    Lq, Hq, _ = q.shape
    Lk, Hk, _ = k.shape
    if layout == "q_of_qkv":
        assert Lq == Lk
        qkv = to_dev(np.concatenate([q.reshape(Lq, Hq * D), k.reshape(Lk, Hk * D), v.reshape(Lk, Hk * D)], axis=1))
        return qkv[:, : Hq * D].view(Lq, Hq, D), to_dev(k), to_dev(v), qkv
    qbuf = to_dev(np.concatenate([q.reshape(Lq, Hq * D), np.full((Lq, D), 7.0, np.float16)], axis=1))
    kv = to_dev(np.concatenate([k.reshape(Lk, Hk * D), v.reshape(Lk, Hk * D)], axis=1))
    return qbuf[:, : Hq * D].view(Lq, Hq, D), kv[:, : Hk * D].view(Lk, Hk, D), kv[:, Hk * D:].view(Lk, Hk, D), (qbuf, kv)


def _launch(case, max_q=None, layout="views"):
    """The case through the shim its head tables call for -> fp32 numpy [Lq, Hq, D]."""
    import block_sparse_attn as bsa
    q, k, v, cu_q, cu_k = pe.inputs(case)
    qd, kd, vd, _keep = _device_inputs(q, k, v, layout)
    cq, ck = to_dev(cu_q), to_dev(cu_k)
    max_q = max(p[0] for p in case["pairs"]) if max_q is None else max_q
    max_k = max(p[1] for p in case["pairs"])
    if case["hm"] is None:
        out = bsa.flash_attn_varlen_func(qd, kd, vd, cq, ck, max_q, max_k, dropout_p=0.0, causal=case["causal"])
    else:
        assert case["causal"]
        fn = bsa.block_streaming_attn_func if case["block"] == 128 else bsa.token_streaming_attn_func
        out = fn(qd, kd, vd, cq, ck, to_dev(case["hm"]), to_dev(case["si"]), max_q, max_k)
    torch.cuda.synchronize()
    assert out.shape == (q.shape[0], case["Hq"], D) and out.dtype == torch.float16
    return out.cpu().numpy().astype(np.float32)


def _check(case, got, what=None, bar=1e-3):
    ref = pe.reference(case).astype(np.float32)
    z = pe.zero_rows(case)
    assert np.isfinite(got).all(), "%s: non-finite output" % case["name"]
    assert not got[z].any(), "%s: %d of %d rows without a visible key are not exact zeros" % (
        case["name"], int(got[z].any(axis=-1).sum()), int(z.sum()))
    return assert_attention_close(got, ref, what or ("prefill attention, case %s" % case["name"]), bar)


# ---- a. unequal lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.family_a(), ids=_ids(pe.family_a()))
def test_unequal_q_and_k_lengths(case):
    """(len_q, len_k) per sequence from (1, 200), (40, 200), (129, 257), (64, 64), (50, 20) -- the first 30 rows see no key --
    and (5, 0) -- none does --, each alone and mixed in one batch, plus a batch on and next to the tile sizes; dense, token- and
    block-streaming heads.  A batch whose key side is empty altogether has no k / v storage to point at: the shim answers it
    with zeros without a launch."""
    _check(case, _launch(case))


# ---- b. non-causal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.family_b(), ids=_ids(pe.family_b()))
def test_non_causal(case):
    _check(case, _launch(case))


def test_shim_default_is_non_causal():
    """flash_attn.flash_attn_varlen_func with `causal` left out."""
    import flash_attn
    case = {c["name"]: c for c in pe.family_b()}["b-q70-k130"]
    q, k, v, cu_q, cu_k = pe.inputs(case)
    qd, kd, vd, _keep = _device_inputs(q, k, v)
    out = flash_attn.flash_attn_varlen_func(qd, kd, vd, to_dev(cu_q), to_dev(cu_k), 70, 130)
    torch.cuda.synchronize()
    _check(case, out.cpu().numpy().astype(np.float32))


# ---- c. per-head windows and classes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 2, 4, 8])
@pytest.mark.parametrize("case", pe.family_c(), ids=_ids(pe.family_c()))
def test_per_head_windows_and_classes(case, split):
    """A head-to-XCD map that handed a streaming head another head's (sink, local), or a dense head any, fails here."""
    from omniserve_amd import _lib
    _lib.lib().omni_prefill_set_xcd_split(split)
    try:
        got = _launch(case)
    finally:
        _lib.lib().omni_prefill_set_xcd_split(0)
    _check(case, got)


# ---- d. "everything" windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.family_d(), ids=_ids(pe.family_d()))
def test_everything_windows_equal_dense_causal(case):
    """sink or local of 1 << 24, (1 << 24) + 3, 1 << 25, 1 << 30, 2**31 - 1: vs the oracle (Python integers: nothing wraps) and vs
    the dense-causal launch on the same inputs.  Before the window arithmetic clamped (sink, local) to the key length the block
    form wrapped in int32 from 1 << 24 on: the window opened behind the query and the rows came back as zeros."""
    got = _launch(case)
    _check(case, got)
    dense = _launch(dict(case, hm=None, si=None, block=1))
    assert_attention_close(got, dense, "case %s vs the dense-causal launch" % case["name"])


def _raw_launch(case, guard_rows=0, sentinel=12345.0):
    """The case through the C entries (omni_prefill_attention, or the block entry for block windows), with `guard_rows` token
    rows of sentinel behind the output -> (rc, out fp32 numpy [Lq + guard_rows, Hq, D])."""
    from omniserve_amd import _lib
    q, k, v, cu_q, cu_k = pe.inputs(case)
    qd, kd, vd, _keep = _device_inputs(q, k, v)
    cq, ck = to_dev(cu_q), to_dev(cu_k)
    Hq, Hk = case["Hq"], case["Hk"]
    out = torch.full((q.shape[0] + guard_rows, Hq, D), sentinel, dtype=torch.float16, device=qd.device)
    hm = to_dev(case["hm"]) if case["hm"] is not None else None
    si = to_dev(case["si"]) if case["si"] is not None else None
    max_q = max(p[0] for p in case["pairs"])
    head = (out.data_ptr(), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), qd.stride(0), kd.stride(0), vd.stride(0),
            cq.data_ptr(), ck.data_ptr(), len(case["pairs"]), max_q, Hq, Hk, D)
    if case["block"] == 128:
        assert case["causal"]
        rc = _lib.lib().omni_prefill_attention_block_streaming(*head, hm.data_ptr(), si.data_ptr(), _lib.current_stream())
    else:
        rc = _lib.lib().omni_prefill_attention(*head, 1 if case["causal"] else 0, hm.data_ptr() if hm is not None else None,
                                               si.data_ptr() if si is not None else None, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().astype(np.float32)


@pytest.mark.parametrize("case", pe.family_d_noncausal(), ids=_ids(pe.family_d_noncausal()))
def test_everything_windows_non_causal_negative_positions(case):
    """Token windows on a non-causal launch (omni_prefill_attention takes both): with len_q 50 > len_k 20 the first queries sit
    at negative positions, where position - local + 1 left int32 for local = 2**31 - 1 before the clamp."""
    rc, got = _raw_launch(case)
    assert rc == 0
    _check(case, got)
    rc, dense = _raw_launch(dict(case, hm=None, si=None))
    assert rc == 0
    assert_attention_close(got, dense, "case %s vs the dense non-causal launch" % case["name"])


# ---- e. online-softmax stress -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.family_e(), ids=_ids(pe.family_e()))
def test_online_softmax_stress(case):
    """Q scaled by 8 (near one-hot softmax), keys with a norm ramp ascending (every key tile's maximum beats the last by more
    than 20: alpha underflows to 0 at every tile) or descending (the first tile holds the maximum: alpha == 1 and the rescale is
    skipped ever after), L = 700; dense heads and streaming heads with window (0, 20), whose first visited tile is fully masked
    for the late rows of a query tile (running maximum still at its start value).  Finite everywhere, at the 1e-3 bar."""
    _check(case, _launch(case))


# ---- f. launch geometry --------------------------------------------------------------------------------------------------------
_F = {c["name"]: c for c in pe.family_f()}
_F_MODES = ["dense", "token", "block"]


@pytest.mark.parametrize("mode", _F_MODES)
def test_max_seqlen_q_beyond_the_longest_sequence(mode):
    """max_seqlen_q = 1000 for lengths [70, 130]: seven empty tail tiles per head and padding workgroups in the 1-D grid."""
    case = _F["f-70-130-" + mode]
    _check(case, _launch(case, max_q=1000))


@pytest.mark.parametrize("mode", _F_MODES)
def test_zero_length_sequences_first_middle_and_last(mode):
    case = _F["f-zero-lengths-" + mode]
    _check(case, _launch(case))
    _check(case, _launch(case, max_q=257))


@pytest.mark.parametrize("mode", _F_MODES)
def test_three_different_token_strides(mode):
    """q a view of the fused qkv buffer, k and v contiguous tensors of their own."""
    case = _F["f-70-130-" + mode]
    _check(case, _launch(case, layout="q_of_qkv"))


# ---- g. guard band ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pe.family_g(), ids=_ids(pe.family_g()))
def test_rows_behind_out_are_left_alone(case):
    """`out` with two more token rows than tokens, filled with a sentinel; the last sequence ends inside a query tile (65 rows,
    1 row).  The launch returns 0, the two rows still hold the sentinel, the rows before them meet the oracle."""
    sentinel = 12345.0
    rc, got = _raw_launch(case, guard_rows=2, sentinel=sentinel)
    assert rc == 0
    T = sum(p[0] for p in case["pairs"])
    assert got.shape[0] == T + 2
    assert (got[T:] == np.float32(np.float16(sentinel))).all(), "rows behind the last token were written"
    _check(case, got[:T])
