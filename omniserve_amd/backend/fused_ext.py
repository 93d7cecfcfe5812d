"""Opt-in fused entry points (NOT in the reference's omniserve_backend).
Each is bit-identical to the pair of reference calls it replaces."""
import collections

import torch

from .. import _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def add_rms_norm_general_fuse_sum(out, residual, delta, weight, input_sum, scaling, epsilon):
    """residual += delta (in place, fp16), then rms_norm_general_fuse_sum(out, residual, ...).
    input_sum=None: no row sum (= rms_norm_general, what the W8A8 / per-group layers call)."""
    _lib.require_cuda(out, residual, delta, weight, input_sum, scaling)
    hidden = residual.shape[-1]
    tokens = residual.numel() // hidden
    if not residual.is_contiguous() or not delta.is_contiguous():
        raise RuntimeError("add_rms_norm_general_fuse_sum: residual and delta must be contiguous")
    rc = _lib.lib().omni_add_rms_norm_general_fuse_sum(
        out.data_ptr(), residual.data_ptr(), delta.data_ptr(), weight.data_ptr(), _ptr(input_sum),
        scaling.data_ptr(), float(epsilon), tokens, hidden, _lib.current_stream())
    _lib.check(rc, "fused_ext.add_rms_norm_general_fuse_sum")


def silu_mul_quant_fuse_sum(out, input, input_sum, scale):
    """silu_and_mul(tmp, input); invoke_quant_fuse_sum(out, tmp, input_sum, scale) without tmp.
    input_sum=None: invoke_quant (no row sum)."""
    _lib.require_cuda(out, input, input_sum, scale)
    d = input.shape[-1] // 2
    tokens = input.numel() // input.shape[-1]
    rc = _lib.lib().omni_silu_mul_quant_fuse_sum(out.data_ptr(), input.data_ptr(), _ptr(input_sum),
                                                 scale.data_ptr(), tokens, d, _lib.current_stream())
    _lib.check(rc, "fused_ext.silu_mul_quant_fuse_sum")


def gemm_partial_per_chn(in_feats, kernel, slab):
    """Decode-shape W4A8 per-channel GEMM without its epilogue: writes int32 partial sums
    slab[sk][M][N] and returns sk.  Pair with splitk_add_rms_norm_general_fuse_sum."""
    import ctypes
    _lib.require_cuda(in_feats, kernel, slab)
    M, K = in_feats.shape
    N = kernel.shape[0]
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w4a8_per_chn_gemm_partial(in_feats.data_ptr(), kernel.data_ptr(), slab.data_ptr(),
                                                   slab.numel() * slab.element_size(), M, N, K,
                                                   ctypes.byref(sk), _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_per_chn")
    return sk.value


def splitk_add_rms_norm_general_fuse_sum(out, residual, slab, sk, wscales, ascales_in, w_szs, a_ssums_in,
                                         weight, input_sum, scaling, epsilon):
    """residual += fp16(per-channel GEMM epilogue(sum of sk slabs)); then norm + quant (+sum) of it."""
    _lib.require_cuda(out, residual, slab, wscales, ascales_in, w_szs, a_ssums_in, weight, input_sum, scaling)
    hidden = residual.shape[-1]
    tokens = residual.numel() // hidden
    rc = _lib.lib().omni_splitk_add_rms_norm_general_fuse_sum(
        out.data_ptr(), residual.data_ptr(), slab.data_ptr(), int(sk), wscales.data_ptr(), ascales_in.data_ptr(),
        w_szs.data_ptr(), a_ssums_in.data_ptr(), weight.data_ptr(), input_sum.data_ptr(), scaling.data_ptr(),
        float(epsilon), tokens, hidden, _lib.current_stream())
    _lib.check(rc, "fused_ext.splitk_add_rms_norm_general_fuse_sum")


def gemm_partial_w8a8(in_feats, weight, slab):
    """Decode-shape W8A8 GEMM without its epilogue (int32 partial sums slab[sk][M][N], returns sk); pair with
    splitk_w8_add_rms_norm_general_fuse_sum."""
    import ctypes
    _lib.require_cuda(in_feats, weight, slab)
    M, K = in_feats.shape
    N = weight.shape[0]
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w8a8_gemm_partial(in_feats.data_ptr(), weight.data_ptr(), slab.data_ptr(),
                                           slab.numel() * slab.element_size(), M, N, K, ctypes.byref(sk),
                                           _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_w8a8")
    return sk.value


def gemm_partial_per_group(in_feats, qweight, s2_zeros, s2_scales, slab):
    """Decode-shape g128 W4A8 GEMM without its epilogue (int32 slabs, returns sk); the epilogue formula is the W8A8 one, so
    the consumer is splitk_w8_add_rms_norm_general_fuse_sum."""
    import ctypes
    _lib.require_cuda(in_feats, qweight, s2_zeros, s2_scales, slab)
    M, K = in_feats.shape
    N = qweight.shape[0]
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w4a8_per_group_gemm_partial(in_feats.data_ptr(), qweight.data_ptr(), s2_zeros.data_ptr(),
                                                     s2_scales.data_ptr(), slab.data_ptr(),
                                                     slab.numel() * slab.element_size(), M, N, K, ctypes.byref(sk),
                                                     _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_per_group")
    return sk.value


def splitk_w8_add_rms_norm_general_fuse_sum(out, residual, slab, sk, wscales, ascales_in, weight, input_sum, scaling,
                                            epsilon):
    """residual += fp16(W8A8 GEMM epilogue(sum of sk slabs)); then norm + quant (+sum) of it."""
    _lib.require_cuda(out, residual, slab, wscales, ascales_in, weight, input_sum, scaling)
    hidden = residual.shape[-1]
    tokens = residual.numel() // hidden
    rc = _lib.lib().omni_splitk_w8_add_rms_norm_general_fuse_sum(
        out.data_ptr(), residual.data_ptr(), slab.data_ptr(), int(sk), wscales.data_ptr(), ascales_in.data_ptr(),
        weight.data_ptr(), _ptr(input_sum), scaling.data_ptr(), float(epsilon), tokens, hidden,
        _lib.current_stream())
    _lib.check(rc, "fused_ext.splitk_w8_add_rms_norm_general_fuse_sum")


def splitk_add_rms_norm(out, residual, slab, sk, wscales, ascales_in, w_szs, a_ssums_in, weight, epsilon):
    """The LAST layer's deferred down projection consumed by the model's final norm: residual += fp16(GEMM epilogue(sum of
    sk slabs)); out fp16 = rms_norm(residual) (layernorm_ops.rms_norm, no quantisation).  w_szs / a_ssums_in both None: the
    W8A8 / per-group epilogue; both given: the per-channel W4A8 one.  Bit-identical to GEMM -> add -> rms_norm."""
    _lib.require_cuda(out, residual, slab, wscales, ascales_in, w_szs, a_ssums_in, weight)
    hidden = residual.shape[-1]
    tokens = residual.numel() // hidden
    rc = _lib.lib().omni_splitk_add_rms_norm(out.data_ptr(), residual.data_ptr(), slab.data_ptr(), int(sk),
                                             wscales.data_ptr(), ascales_in.data_ptr(), _ptr(w_szs), _ptr(a_ssums_in),
                                             weight.data_ptr(), float(epsilon), tokens, hidden, _lib.current_stream())
    _lib.check(rc, "fused_ext.splitk_add_rms_norm")


def decode_arm_qkv_slabs(slab, sk, rows, width, col_q, col_k, col_v, wscales, ascales, w_szs=None, a_ssums=None):
    """The next decode-attention call of this thread reads the current token's q / k / v from the qkv projection's int32
    split-K slabs (gemm_partial_*: slab [sk][rows][width]) and applies the projection's epilogue itself: no slab epilogue
    launch between the projection and the attention, same bits.  col_*: first channel of the q / k / v blocks of a row.
    w_szs / a_ssums: per-channel W4A8 zero term (both) or None (W8A8 / per-group).  slab=None disarms."""
    if slab is None:
        _lib.check(_lib.lib().omni_decode_arm_qkv_slabs(None, 0, 0, 0, 0, 0, 0, None, None, None, None),
                   "fused_ext.decode_arm_qkv_slabs")
        return
    _lib.require_cuda(slab, wscales, ascales, w_szs, a_ssums)
    rc = _lib.lib().omni_decode_arm_qkv_slabs(slab.data_ptr(), int(sk), int(rows), int(width), int(col_q), int(col_k),
                                              int(col_v), wscales.data_ptr(), ascales.data_ptr(), _ptr(w_szs),
                                              _ptr(a_ssums))
    _lib.check(rc, "fused_ext.decode_arm_qkv_slabs")


def decode_step_begin(out, table, idx, lengths=None, zero=None):
    """First launch of a decode step: out = table[idx] (embed_rows), lengths += 1 (int32), zero[...] = 0 (int32 / uint32
    words: the step's row-maximum slots) in one kernel instead of three."""
    _lib.require_cuda(out, table, idx, lengths, zero)
    if table.dtype != torch.float16 or out.dtype != torch.float16 or table.dim() != 2 or not table.is_contiguous() or \
            not out.is_contiguous() or out.shape[-1] != table.shape[1]:
        raise RuntimeError("decode_step_begin: contiguous fp16 table [V, cols] and out [rows, cols] expected")
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.numel() != out.numel() // table.shape[1]:
        raise RuntimeError("decode_step_begin: idx must be a contiguous int64 tensor with one id per output row")
    if lengths is not None and (lengths.dtype != torch.int32 or not lengths.is_contiguous()):
        raise RuntimeError("decode_step_begin: lengths must be a contiguous int32 tensor")
    if zero is not None and (zero.element_size() != 4 or not zero.is_contiguous()):
        raise RuntimeError("decode_step_begin: zero must be a contiguous tensor of 32-bit words")
    rc = _lib.lib().omni_decode_step_begin(out.data_ptr(), table.data_ptr(), idx.data_ptr(), idx.numel(), table.shape[1],
                                           table.shape[0], _ptr(lengths), 0 if lengths is None else lengths.numel(),
                                           _ptr(zero), 0 if zero is None else zero.numel(), _lib.current_stream())
    _lib.check(rc, "fused_ext.decode_step_begin")


def decode_attention_quant_fuse_sum(out_i8, q, k, v, kv_pointers, lengths, tokens_per_block, timestep,
                                    rotary_base, input_sum, scale):
    """single_query_attention (KV4 + zeros, neox RoPE) followed by invoke_quant_fuse_sum of its
    [B, Hq*Dh] output, with the flash-decoding merge fused into the quantisation kernel."""
    import ctypes
    from ..rope import rope_table
    _lib.require_cuda(out_i8, q, k, v, kv_pointers, lengths, input_sum, scale)
    B, Hq, D = q.shape
    Hkv = k.shape[1]
    max_ctx = max(int(timestep), 1)
    table = rope_table(max_ctx + 1, D, float(rotary_base), 1.0, q.device)
    need = _lib.lib().omni_kv4_decode_workspace_bytes(B, Hq, D, max_ctx)
    ws = _lib.workspace(need, q.device, "attn")
    ns = ctypes.c_int(0)
    rc = _lib.lib().omni_kv4_decode_attention_partial(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), kv_pointers.data_ptr(),
        lengths.data_ptr(), B, kv_pointers.shape[-1], Hq, Hkv, D, int(tokens_per_block), max_ctx,
        table.data_ptr(), table.shape[0], ws.data_ptr(), ws.numel(), ctypes.byref(ns), _lib.current_stream())
    _lib.check(rc, "fused_ext.decode_attention_quant_fuse_sum (partials)")
    ml_bytes = B * Hq * ns.value * 2 * 4
    rc = _lib.lib().omni_attn_merge_quant_fuse_sum(out_i8.data_ptr(), ws.data_ptr(), ws.data_ptr() + ml_bytes, ns.value,
                                                   _ptr(input_sum), scale.data_ptr(), B, Hq, _lib.current_stream())
    _lib.check(rc, "fused_ext.decode_attention_quant_fuse_sum (merge+quant)")


# ---- row-kernel-free decode layer (round 3): the quantisers between two projections folded into the projections ----------
AMAX_WORDS = 8 * 16 * 8      # csrc/common.h: [XCD][row][sub-slot] row-maximum candidates of one activation tensor (<= 16 rows)


def new_amax_slots(rows, device):
    """Zeroed buffer of row-maximum candidates (f32 bit patterns, layout [8 XCDs][16 rows][8 sub-slots]) for an
    activation of `rows` <= 16 rows.  A producer (gemm_silu_*, decode_attention_f16_amax) RAISES the words with an integer
    max: zero the buffer before every producer call that should start a fresh maximum."""
    if rows > 16:
        raise RuntimeError("row-maximum hand-off covers at most 16 activation rows")
    return torch.zeros((AMAX_WORDS,), dtype=torch.int32, device=device)


def amax_rows(amax, rows):
    """float32 [rows]: the row maxima a buffer of candidates currently holds (tests / debugging)."""
    return amax.view(torch.float32).view(8, 16, 8).amax(dim=(0, 2))[:rows]


def gemm_silu_per_chn(in_feats, qweight, wscales, ascales, w_szs, a_ssums, act, amax):
    """gate_up projection + silu_and_mul in one kernel: act fp16 [M, N/2] = silu_and_mul(gemm_forward_cuda(...)) bit for
    bit, and the row maxima of |act| raised in `amax` (new_amax_slots).  M <= 16."""
    _lib.require_cuda(in_feats, qweight, wscales, ascales, w_szs, a_ssums, act, amax)
    M, K = in_feats.shape
    N = qweight.shape[0]
    if act.dtype != torch.float16 or tuple(act.shape) != (M, N // 2) or not act.is_contiguous():
        raise RuntimeError("gemm_silu_per_chn: act must be a contiguous fp16 [M, N/2] tensor")
    rc = _lib.lib().omni_w4a8_per_chn_gemm_silu(in_feats.data_ptr(), qweight.data_ptr(), wscales.data_ptr(),
                                                ascales.data_ptr(), w_szs.data_ptr(), a_ssums.data_ptr(),
                                                act.data_ptr(), amax.data_ptr(), M, N, K, _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_silu_per_chn")


def gemm_silu_per_group(in_feats, qweight, s2_zeros, s2_scales, wscales, ascales, act, amax):
    """The g128 form of gemm_silu_per_chn."""
    _lib.require_cuda(in_feats, qweight, s2_zeros, s2_scales, wscales, ascales, act, amax)
    M, K = in_feats.shape
    N = qweight.shape[0]
    if act.dtype != torch.float16 or tuple(act.shape) != (M, N // 2) or not act.is_contiguous():
        raise RuntimeError("gemm_silu_per_group: act must be a contiguous fp16 [M, N/2] tensor")
    rc = _lib.lib().omni_w4a8_per_group_gemm_silu(in_feats.data_ptr(), qweight.data_ptr(), s2_zeros.data_ptr(),
                                                  s2_scales.data_ptr(), wscales.data_ptr(), ascales.data_ptr(),
                                                  act.data_ptr(), amax.data_ptr(), M, N, K, _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_silu_per_group")


def gemm_partial_f16_per_chn(act, amax, qweight, slab, sum_out, scale_out):
    """o / down projection straight from fp16 activations: the int8 codes invoke_quant_fuse_sum(act) would produce are
    computed inside the GEMV from `amax` (row maxima left by the producer of `act`); writes int32 split-K slabs (returns
    sk, as gemm_partial_per_chn) and -- by rider workgroups -- the fp16 row sums / scales of invoke_quant_fuse_sum into
    sum_out / scale_out, for splitk_add_rms_norm_general_fuse_sum.  M <= 16, K <= 16384."""
    import ctypes
    _lib.require_cuda(act, amax, qweight, slab, sum_out, scale_out)
    M, K = act.shape
    N = qweight.shape[0]
    if act.dtype != torch.float16 or not act.is_contiguous():
        raise RuntimeError("gemm_partial_f16_per_chn: act must be a contiguous fp16 [M, K] tensor")
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w4a8_per_chn_gemm_partial_f16(act.data_ptr(), amax.data_ptr(), qweight.data_ptr(),
                                                       slab.data_ptr(), slab.numel() * slab.element_size(),
                                                       _ptr(sum_out), scale_out.data_ptr(), M, N, K, ctypes.byref(sk),
                                                       _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_f16_per_chn")
    return sk.value


def gemm_partial_f16_per_group(act, amax, qweight, s2_zeros, s2_scales, slab, sum_out, scale_out):
    """The g128 form of gemm_partial_f16_per_chn (sum_out may be None: the per-group layers read no row sums)."""
    import ctypes
    _lib.require_cuda(act, amax, qweight, s2_zeros, s2_scales, slab, sum_out, scale_out)
    M, K = act.shape
    N = qweight.shape[0]
    if act.dtype != torch.float16 or not act.is_contiguous():
        raise RuntimeError("gemm_partial_f16_per_group: act must be a contiguous fp16 [M, K] tensor")
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w4a8_per_group_gemm_partial_f16(act.data_ptr(), amax.data_ptr(), qweight.data_ptr(),
                                                         s2_zeros.data_ptr(), s2_scales.data_ptr(), slab.data_ptr(),
                                                         slab.numel() * slab.element_size(), _ptr(sum_out),
                                                         scale_out.data_ptr(), M, N, K, ctypes.byref(sk),
                                                         _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_f16_per_group")
    return sk.value


def gemm_silu_w8a8(in_feats, weight, wscales, ascales, act, amax):
    """The W8A8 form of gemm_silu_per_chn (LServe models: gate_up_proj -> silu*mul, llama_w8a8_unpad.py:94-105): act fp16
    [M, N/2] bit for bit what w8a8_gemm_forward_cuda -> silu_and_mul leave, row maxima of |act| raised in `amax`.  M <= 16."""
    _lib.require_cuda(in_feats, weight, wscales, ascales, act, amax)
    M, K = in_feats.shape
    N = weight.shape[0]
    if act.dtype != torch.float16 or tuple(act.shape) != (M, N // 2) or not act.is_contiguous():
        raise RuntimeError("gemm_silu_w8a8: act must be a contiguous fp16 [M, N/2] tensor")
    rc = _lib.lib().omni_w8a8_gemm_silu(in_feats.data_ptr(), weight.data_ptr(), wscales.data_ptr(), ascales.data_ptr(),
                                        act.data_ptr(), amax.data_ptr(), M, N, K, _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_silu_w8a8")


def gemm_partial_f16_w8a8(act, amax, weight, slab, scale_out):
    """The W8A8 form of gemm_partial_f16_per_chn: slabs of gemm_partial_w8a8 on the codes invoke_quant(act) would produce,
    scale_out = invoke_quant's scales (no row sums: W8A8 has no zero-point term).  M <= 16, any K."""
    import ctypes
    _lib.require_cuda(act, amax, weight, slab, scale_out)
    M, K = act.shape
    N = weight.shape[0]
    if act.dtype != torch.float16 or not act.is_contiguous():
        raise RuntimeError("gemm_partial_f16_w8a8: act must be a contiguous fp16 [M, K] tensor")
    sk = ctypes.c_int(0)
    rc = _lib.lib().omni_w8a8_gemm_partial_f16(act.data_ptr(), amax.data_ptr(), weight.data_ptr(), slab.data_ptr(),
                                               slab.numel() * slab.element_size(), scale_out.data_ptr(), M, N, K,
                                               ctypes.byref(sk), _lib.current_stream())
    _lib.check(rc, "fused_ext.gemm_partial_f16_w8a8")
    return sk.value


_TICKETS = {}


TICKET_WORDS = 4096


def new_tickets(device):
    """Ticket words of the single-launch decode attention: zero between launches (the last arriver resets its word).
    include/omniserve_hip.h asks for one buffer per stream: a runner OWNS one (allocated once, before any capture) and hands it
    to decode_attention_f16_amax -- two runners decoding concurrently on two streams then never share words, and a captured
    graph holds no allocation made during capture (the per-(device, stream) cache below missed on torch's capture
    stream and allocated + zero-filled inside the graph)."""
    return torch.zeros((TICKET_WORDS,), dtype=torch.int32, device=device)


def _tickets(device):
    """Fallback for callers that pass no buffer (tests, one-off calls): one buffer per (device, stream)."""
    key = (torch.device(device), int(_lib.current_stream()))
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = new_tickets(device)
    return t


def decode_attention_f16_amax(out_f16, amax, q, k, v, kv_pointers, lengths, tokens_per_block, timestep, rotary_base,
                              single_launch=True, tickets=None):
    """single_query_attention (KV4 + zeros, neox RoPE) writing the fp16 [B, Hq*Dh] output (the values
    single_query_attention returns) into out_f16 and raising the row maxima of |out| in `amax` -- the input pair of
    gemm_partial_f16_*.  single_launch: the last-arriving split workgroup of every (sequence, head group) merges the splits
    inside the attention launch (omni_kv4_decode_attention_f16_amax); False: split partials + the wide merge kernel (two
    launches).  Same bits either way."""
    import ctypes
    from ..rope import rope_table
    _lib.require_cuda(out_f16, amax, q, k, v, kv_pointers, lengths)
    B, Hq, D = q.shape
    Hkv = k.shape[1]
    max_ctx = max(int(timestep), 1)
    table = rope_table(max_ctx + 1, D, float(rotary_base), 1.0, q.device)
    need = _lib.lib().omni_kv4_decode_workspace_bytes(B, Hq, D, max_ctx)
    ws = _lib.workspace(need, q.device, "attn")
    if single_launch:
        tk = tickets if tickets is not None else _tickets(q.device)
        rc = _lib.lib().omni_kv4_decode_attention_f16_amax(
            out_f16.data_ptr(), amax.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0),
            kv_pointers.data_ptr(), lengths.data_ptr(), B, kv_pointers.shape[-1], Hq, Hkv, D, int(tokens_per_block), max_ctx,
            table.data_ptr(), table.shape[0], ws.data_ptr(), ws.numel(), tk.data_ptr(), tk.numel(), _lib.current_stream())
        _lib.check(rc, "fused_ext.decode_attention_f16_amax (single launch)")
        return
    ns = ctypes.c_int(0)
    rc = _lib.lib().omni_kv4_decode_attention_partial(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), kv_pointers.data_ptr(),
        lengths.data_ptr(), B, kv_pointers.shape[-1], Hq, Hkv, D, int(tokens_per_block), max_ctx,
        table.data_ptr(), table.shape[0], ws.data_ptr(), ws.numel(), ctypes.byref(ns), _lib.current_stream())
    _lib.check(rc, "fused_ext.decode_attention_f16_amax (partials)")
    ml_bytes = B * Hq * ns.value * 2 * 4
    rc = _lib.lib().omni_attn_merge_f16_amax(out_f16.data_ptr(), ws.data_ptr(), ws.data_ptr() + ml_bytes, ns.value,
                                             amax.data_ptr(), B, Hq, _lib.current_stream())
    _lib.check(rc, "fused_ext.decode_attention_f16_amax (merge)")


def prefetch_arm_gemm(weight, M, N, K, mode=0, deferred=False, budget_bytes=24 << 20, blocks=240):
    """Arm the one-shot L2 weight prefetch for the NEXT decode-shape GEMM (include/omniserve_hip.h:
    omni_prefetch_arm_gemm): the next decode-size quant / norm row kernel launched through this library carries
    `blocks` extra workgroups that pull up to `budget_bytes` of `weight` into the L2s.  mode: 0 W4A8 per-channel,
    1 per-group, 2 W8A8; | 0x10: the GEMM will run as gemm_silu_* (gate / up tile rows paired per workgroup); | 0x20: that
    GEMM keeps non-temporal weight loads (default: the GEMM enqueued next on `weight` loads plain -- its lines sit in L2;
    every other decode-shape GEMM streams non-temporally: the policy is per call, there is no process-wide switch).
    budget_bytes <= 0 disarms.  A performance hint only."""
    _lib.require_cuda(weight)
    rc = _lib.lib().omni_prefetch_arm_gemm(weight.data_ptr(), int(M), int(N), int(K), int(mode), int(bool(deferred)),
                                           int(budget_bytes), int(blocks))
    _lib.check(rc, "fused_ext.prefetch_arm_gemm")


def prefetch_disarm():
    """Drop an armed (not yet consumed) prefetch descriptor of this thread."""
    rc = _lib.lib().omni_prefetch_arm_gemm(None, 0, 0, 0, 0, 0, 0, 0)
    _lib.check(rc, "fused_ext.prefetch_disarm")


def sparse_decode_attention_quant(out_i8, input_sum, scale, q, k, v, retrieval_kv_pointers, streaming_kv_pointers,
                                  retrieval_head_flags, head_rank_table, dynamic_sparse_page_idxes, lengths,
                                  tokens_per_block, size_per_retrieval_token, size_per_streaming_token, sink_token_num,
                                  local_token_num, sink_block_num, local_block_num, num_retrieval_kv_heads,
                                  num_streaming_kv_heads, timestep, rotary_base, rotary_embedding_scale,
                                  tokens_per_sub_chunk, kv_scale_quant_orig=None, kv_scale_orig_quant=None):
    """LServe decode attention (fused_attention_fine_grained_sparse / fused_attention_per_tensor_sparse
    .single_query_attention; per-tensor KV8 when the two scale tensors are given) followed by the per-token
    quantisation of its [B, Hq*Dh] output (fused_kernels.invoke_quant[_fuse_sum]), with the flash-decoding merge done by
    the quantiser: one launch less and no fp16 round trip; codes and scales bit-identical to the two-call sequence."""
    from ._attn_common import decode_attention_fine_grained
    per_tensor = kv_scale_quant_orig is not None
    D = q.shape[-1]
    decode_attention_fine_grained(
        q, k, v, retrieval_kv_pointers, streaming_kv_pointers, retrieval_head_flags, head_rank_table,
        dynamic_sparse_page_idxes, lengths, tokens_per_block, size_per_retrieval_token, size_per_streaming_token,
        sink_token_num, local_token_num, sink_block_num, local_block_num, num_retrieval_kv_heads, num_streaming_kv_heads,
        int(timestep), D, rotary_base, 1.0 / float(rotary_embedding_scale), True, not per_tensor, not per_tensor,
        tokens_per_sub_chunk, "fused_ext.sparse_decode_attention_quant", kv_scale_quant_orig=kv_scale_quant_orig,
        kv_scale_orig_quant=kv_scale_orig_quant, per_tensor=per_tensor, merge_quant=(out_i8, input_sum, scale))


def sparse_decode_attention_f16_amax(out_f16, amax, q, k, v, retrieval_kv_pointers, streaming_kv_pointers,
                                     retrieval_head_flags, head_rank_table, dynamic_sparse_page_idxes, lengths,
                                     tokens_per_block, size_per_retrieval_token, size_per_streaming_token, sink_token_num,
                                     local_token_num, sink_block_num, local_block_num, num_retrieval_kv_heads,
                                     num_streaming_kv_heads, timestep, rotary_base, rotary_embedding_scale,
                                     tokens_per_sub_chunk, kv_scale_quant_orig=None, kv_scale_orig_quant=None):
    """LServe decode attention (as sparse_decode_attention_quant) with the merge as the wide kernel of
    decode_attention_f16_amax: out_f16 [B, Hq*Dh] = the values single_query_attention returns, row maxima of |out| raised
    in `amax` -- the input pair of gemm_partial_f16_w8a8 (o_proj quantises on the fly: no quantiser row kernel)."""
    from ._attn_common import decode_attention_fine_grained
    per_tensor = kv_scale_quant_orig is not None
    D = q.shape[-1]
    decode_attention_fine_grained(
        q, k, v, retrieval_kv_pointers, streaming_kv_pointers, retrieval_head_flags, head_rank_table,
        dynamic_sparse_page_idxes, lengths, tokens_per_block, size_per_retrieval_token, size_per_streaming_token,
        sink_token_num, local_token_num, sink_block_num, local_block_num, num_retrieval_kv_heads, num_streaming_kv_heads,
        int(timestep), D, rotary_base, 1.0 / float(rotary_embedding_scale), True, not per_tensor, not per_tensor,
        tokens_per_sub_chunk, "fused_ext.sparse_decode_attention_f16_amax", kv_scale_quant_orig=kv_scale_quant_orig,
        kv_scale_orig_quant=kv_scale_orig_quant, per_tensor=per_tensor, merge_f16=(out_f16, amax))


def embed_rows(out, table, idx):
    """out fp16 [rows, cols] = table[idx] (torch.index_select(table, 0, idx, out=out)): the embedding lookup of the decode
    drivers as one short kernel -- upstream it is torch.nn.Embedding, not one of the reference's kernels."""
    _lib.require_cuda(out, table, idx)
    if table.dtype != torch.float16 or out.dtype != torch.float16 or table.dim() != 2 or not table.is_contiguous() or \
            not out.is_contiguous() or out.shape[-1] != table.shape[1]:
        raise RuntimeError("embed_rows: contiguous fp16 table [V, cols] and out [rows, cols] expected")
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.numel() != out.numel() // table.shape[1]:
        raise RuntimeError("embed_rows: idx must be a contiguous int64 tensor with one id per output row")
    rc = _lib.lib().omni_gather_rows_f16(out.data_ptr(), table.data_ptr(), idx.data_ptr(), idx.numel(), table.shape[1],
                                         table.shape[0], _lib.current_stream())
    _lib.check(rc, "fused_ext.embed_rows")


def argmax(out, logits):
    """out int64 [rows] = torch.argmax(logits fp16 [rows, cols], dim=-1) (first maximum); greedy-sampling helper of the
    decode runner -- the reference's sampler is torch code, this is not one of its kernels."""
    _lib.require_cuda(out, logits)
    if logits.dtype != torch.float16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("argmax: logits must be fp16 [rows, cols] with contiguous rows")
    if out.dtype != torch.int64 or out.numel() != logits.shape[0] or not out.is_contiguous():
        raise RuntimeError("argmax: out must be a contiguous int64 [rows] tensor")
    need = _lib.lib().omni_argmax_workspace_bytes(logits.shape[0])
    ws = _lib.workspace(need, logits.device, "argmax")
    rc = _lib.lib().omni_argmax_f16(out.data_ptr(), logits.data_ptr(), logits.stride(0), logits.shape[0],
                                    logits.shape[1], ws.data_ptr(), ws.numel(), _lib.current_stream())
    _lib.check(rc, "fused_ext.argmax")


def _per_row(value, rows, dtype, device, name):
    """A sampling parameter as a contiguous [rows] device tensor of `dtype` (a Python scalar is broadcast)."""
    if not torch.is_tensor(value):
        return torch.full((rows,), value, dtype=dtype, device=device)
    if value.dtype != dtype or value.numel() != rows or not value.is_contiguous():
        raise RuntimeError("sample: %s must be a contiguous %s tensor with one entry per row" %
                           (name, str(dtype).replace("torch.", "")))
    return value


def sample(out, logits, temperature, top_k, top_p, u, probe=None, exclude=None, probe_prob=None):
    """out int64 [rows] = one sampled token per row of logits fp16 [rows, cols]: temperature, then the top-p filter, then the
    top-k filter, then the draw -- one kernel family in place of the reference sampler's torch code (omniserve/modeling/
    layers/sampler.py:29-50, 96-102: the three HF warpers, softmax, torch.multinomial), full-vocabulary sort included.
    temperature f32 / top_k i32 (<= 0: off) / top_p f32 (>= 1: off): per-row device tensors or Python scalars; u f32 [rows] in
    [0, 1): the draw.  A row with temperature < 1e-5, top_p < 1e-8 or top_k == 1 (the reference's greedy test), with a NaN /
    +inf maximum or nothing but -inf gets fused_ext.argmax's token.  probe / exclude int64 [rows] (-1: none): probe_prob f32
    [rows] = the probed token's probability under the filtered distribution (0 if filtered out); the excluded token is left
    out of the draw (the rejection rule of speculative sampling needs both).  Contract and tie rule: DESIGN.md section 4.6."""
    if logits.dtype != torch.float16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("sample: logits must be fp16 [rows, cols] with contiguous rows")
    rows, cols = logits.shape
    if out.dtype != torch.int64 or out.numel() != rows or not out.is_contiguous():
        raise RuntimeError("sample: out must be a contiguous int64 [rows] tensor")
    dev = logits.device
    temperature = _per_row(temperature, rows, torch.float32, dev, "temperature")
    top_k = _per_row(top_k, rows, torch.int32, dev, "top_k")
    top_p = _per_row(top_p, rows, torch.float32, dev, "top_p")
    if not torch.is_tensor(u):
        raise RuntimeError("sample: u must be a float32 tensor with one draw per row")
    u = _per_row(u, rows, torch.float32, dev, "u")
    if probe_prob is not None and probe is None:
        raise RuntimeError("sample: probe_prob needs probe")
    if probe is not None:
        probe = _per_row(probe, rows, torch.int64, dev, "probe")
    if exclude is not None:
        exclude = _per_row(exclude, rows, torch.int64, dev, "exclude")
    if probe_prob is not None:
        probe_prob = _per_row(probe_prob, rows, torch.float32, dev, "probe_prob")
    _lib.require_cuda(out, logits, temperature, top_k, top_p, u, probe, exclude, probe_prob)
    need = _lib.lib().omni_sample_workspace_bytes(rows, cols)
    ws = _lib.workspace(need, dev, "sample")
    rc = _lib.lib().omni_sample_f16(out.data_ptr(), _ptr(probe_prob), logits.data_ptr(), logits.stride(0), rows, cols,
                                    temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), u.data_ptr(), _ptr(probe),
                                    _ptr(exclude), ws.data_ptr(), ws.numel(), _lib.current_stream())
    _lib.check(rc, "fused_ext.sample")


LOGPROB_MAX_TOP = 20     # csrc/logprob.hip
LOGPROB_CHUNKS = 32      # workgroups per row; a chunk is logprob_chunk_cols(cols) columns
LOGPROB_VEC = 8          # columns per 16-byte load (row stride % 8 == 0 and a 16-byte aligned base)

LogProbs = collections.namedtuple("LogProbs", "lse token_logprob rank top_tokens top_logprobs")


def logprob_chunk_cols(cols):
    """Columns per chunk of the log-probability kernels: a function of cols only (part of the determinism contract)."""
    return ((cols + LOGPROB_CHUNKS - 1) // LOGPROB_CHUNKS + LOGPROB_VEC - 1) // LOGPROB_VEC * LOGPROB_VEC


def logprobs(logits, target=None, n_top=0, lse=None, token_logprob=None, rank=None, top_tokens=None, top_logprobs=None):
    """Log-probabilities under the RAW distribution of each row of logits fp16 [rows, cols] (no temperature, no filter): what the
    reference's SamplingParams.logprobs / prompt_logprobs ask for and its sampler never fills.  lse f32 [rows] = max + ln sum
    exp(x - max); with target int64 [rows]: token_logprob f32 [rows] = x[target] - lse and rank int32 [rows] = the target's
    1-based position in the canonical order (value descending by fused_ext.argmax's key, then index ascending); NaN / 0 for a
    target outside [0, cols); with n_top in 1 .. LOGPROB_MAX_TOP: top_tokens int64 / top_logprobs f32 [rows, n_top], the first
    n_top tokens in that order (-1 / -inf behind the last column).  Outputs that are not passed are allocated (token_logprob /
    rank only with a target, the top lists only with n_top > 0).  -> LogProbs(lse, token_logprob, rank, top_tokens,
    top_logprobs), None where nothing was computed.  Contract: DESIGN.md section 4.6a."""
    if logits.dtype != torch.float16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("logprobs: logits must be fp16 [rows, cols] with contiguous rows")
    rows, cols = logits.shape
    dev = logits.device
    n_top = int(n_top)
    if not 0 <= n_top <= LOGPROB_MAX_TOP:
        raise ValueError("logprobs: n_top must be in 0 .. %d, got %d" % (LOGPROB_MAX_TOP, n_top))
    if target is None and (token_logprob is not None or rank is not None):
        raise RuntimeError("logprobs: token_logprob / rank need target")
    if n_top == 0 and (top_tokens is not None or top_logprobs is not None):
        raise RuntimeError("logprobs: top_tokens / top_logprobs need n_top > 0")
    if target is not None and (target.dtype != torch.int64 or target.numel() != rows or not target.is_contiguous()):
        raise RuntimeError("logprobs: target must be a contiguous int64 tensor with one entry per row")

    def out(t, name, shape, dtype, wanted):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev) if wanted else None
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("logprobs: %s must be a contiguous %s %s tensor" %
                               (name, str(dtype).replace("torch.", ""), list(shape)))
        return t

    lse = out(lse, "lse", (rows,), torch.float32, True)
    token_logprob = out(token_logprob, "token_logprob", (rows,), torch.float32, target is not None)
    rank = out(rank, "rank", (rows,), torch.int32, target is not None)
    top_tokens = out(top_tokens, "top_tokens", (rows, n_top), torch.int64, n_top > 0)
    top_logprobs = out(top_logprobs, "top_logprobs", (rows, n_top), torch.float32, n_top > 0)
    _lib.require_cuda(logits, target, lse, token_logprob, rank, top_tokens, top_logprobs)
    need = _lib.lib().omni_logprob_workspace_bytes(rows, cols, n_top)
    ws = _lib.workspace(need, dev, "logprob")
    rc = _lib.lib().omni_logprob_f16(_ptr(lse), _ptr(token_logprob), _ptr(rank), _ptr(top_tokens), _ptr(top_logprobs),
                                     logits.data_ptr(), logits.stride(0), rows, cols, _ptr(target), n_top, ws.data_ptr(),
                                     ws.numel(), _lib.current_stream())
    _lib.check(rc, "fused_ext.logprobs")
    return LogProbs(lse, token_logprob, rank, top_tokens, top_logprobs)


def select_topk_pages(out, scores, subs_per_page, total_pages, k):
    """out int32 [B, Hq, k+1] <- the k best pages of [0, total_pages-1) by max-over-sub-chunks selector score (descending),
    then the newest page: one kernel for the torch view / max / topk / cat / to(int32) sequence of
    decoding_attention.py:132-142.  scores fp16 [B, Hq, padded_sub_chunks] as single_query_page_selector returns them."""
    _lib.require_cuda(out, scores)
    if scores.dtype != torch.float16 or scores.dim() != 3 or not scores.is_contiguous():
        raise RuntimeError("select_topk_pages: scores must be a contiguous fp16 [B, Hq, sub_chunks] tensor")
    B, H, _ = scores.shape
    if out.dtype != torch.int32 or tuple(out.shape) != (B, H, k + 1) or not out.is_contiguous():
        raise RuntimeError("select_topk_pages: out must be a contiguous int32 [B, Hq, k+1] tensor")
    rc = _lib.lib().omni_select_topk_pages(out.data_ptr(), scores.data_ptr(), scores.stride(1), B * H,
                                           int(subs_per_page), int(total_pages), int(k), _lib.current_stream())
    _lib.check(rc, "fused_ext.select_topk_pages")


# ---- round 6: (norm -> GEMV) pairs as one launch (csrc/norm_gemv_fused.h) -------------------------------------------
NGF_SYNC_WORDS = 32     # per call site: arrival counter + the rows' {scale, sum} pairs; zeroed by the caller before every launch


def norm_gemm_fused_ok(M, N, K, group_size=-1, silu=False):
    """True when omni_w4a8_per_*_norm_gemm_fused takes the shape and its whole grid is resident on this device."""
    return _lib.lib().omni_norm_gemm_fused_ok(int(M), int(N), int(K), 0 if group_size == -1 else 1, 1 if silu else 0) == 1


def norm_gemm_fused(codes, residual, gamma, input_sum, scaling, epsilon, lin, out, sync, err, slab=None, sk=0, delta=None,
                    producer=None, p_ascales=None, p_asums=None, amax=None, clk=None):
    """rows: residual (+= epilogue(sum of `sk` split-K slabs of `producer`) | += delta | as is) -> rms_norm_general[_fuse_sum] ->
    codes / scaling / input_sum; tiles: out = lin(codes) (amax given: out = silu_and_mul(lin(codes)) [M, N/2], row maxima
    raised) -- ONE launch, bit-identical to the two (three) reference calls.  `lin` / `producer`: objects with qweight,
    s1_scales and s1_szeros (per-channel) or s2_zeros / s2_scales (per-group).  `sync`: NGF_SYNC_WORDS zeroed uint32 words."""
    _lib.require_cuda(codes, residual, gamma, input_sum, scaling, out, sync, err, slab, delta, amax, clk)
    M, K = residual.shape
    N = lin.qweight.shape[0]
    per_chn = getattr(lin, "group", -1) == -1
    st = _lib.current_stream()
    if slab is not None:
        p_ws = producer.s1_scales.data_ptr()
        p_wsz = producer.s1_szeros.data_ptr() if per_chn else None
    else:
        p_ws = p_wsz = None
    if per_chn:
        rc = _lib.lib().omni_w4a8_per_chn_norm_gemm_fused(
            codes.data_ptr(), residual.data_ptr(), _ptr(slab), int(sk), _ptr(delta), p_ws, _ptr(p_ascales), p_wsz,
            _ptr(p_asums), gamma.data_ptr(), _ptr(input_sum), scaling.data_ptr(), float(epsilon), lin.qweight.data_ptr(),
            lin.s1_scales.data_ptr(), lin.s1_szeros.data_ptr(), out.data_ptr(), out.stride(0), _ptr(amax), sync.data_ptr(),
            err.data_ptr(), M, N, K, _ptr(clk), st)
    else:
        rc = _lib.lib().omni_w4a8_per_group_norm_gemm_fused(
            codes.data_ptr(), residual.data_ptr(), _ptr(slab), int(sk), _ptr(delta), p_ws, _ptr(p_ascales), gamma.data_ptr(),
            _ptr(input_sum), scaling.data_ptr(), float(epsilon), lin.qweight.data_ptr(), lin.s2_zeros.data_ptr(),
            lin.s2_scales.data_ptr(), lin.s1_scales.data_ptr(), out.data_ptr(), out.stride(0), _ptr(amax), sync.data_ptr(),
            err.data_ptr(), M, N, K, _ptr(clk), st)
    _lib.check(rc, "fused_ext.norm_gemm_fused")


# ---- chunked / multi-turn prefill: the prefill pair that continues from the KV4 pages ----------------
def _check_lens(t, n, what, name):
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous int32 [%d] tensor" % (what, name, n))


def _kv4_prefill_write(what, qkv, seq_lens, past_lens, rope_offsets, padding_offset, kv_pointers, head_num, kv_head_num,
                       max_seq_len, tokens_per_block, max_total_len, rotary_base, rope_scale, cyclic_len):
    """kv4_prefill_write_at (rope_offsets None) and kv4_prefill_write_at_pos: the checks, the RoPE table and the call."""
    from ..rope import rope_table
    _lib.require_cuda(qkv, seq_lens, past_lens, rope_offsets, padding_offset, kv_pointers)
    width = (head_num + 2 * kv_head_num) * 128
    if qkv.dtype != torch.float16 or qkv.dim() != 2 or qkv.shape[1] != width or not qkv.is_contiguous():
        raise RuntimeError("%s: qkv must be contiguous fp16 [tokens, (Hq+2Hkv)*128]" % what)
    B = seq_lens.shape[0]
    _check_lens(seq_lens, B, what, "seq_lens")
    _check_lens(past_lens, B, what, "past_lens")
    if rope_offsets is not None:
        _check_lens(rope_offsets, qkv.shape[0], what, "rope_offsets")
    _check_lens(padding_offset, qkv.shape[0], what, "padding_offset")
    if kv_pointers.dtype != torch.int64 or kv_pointers.dim() != 3 or kv_pointers.shape[0] != B or kv_pointers.shape[1] != 2 \
            or not kv_pointers.is_contiguous():
        raise RuntimeError("%s: kv_pointers must be a contiguous int64 [B,2,blocks] tensor" % what)
    if int(max_total_len) < int(max_seq_len) or int(max_total_len) > kv_pointers.shape[2] * int(tokens_per_block):
        raise RuntimeError("%s: max_total_len must cover the call's tokens and fit the block table" % what)
    table = rope_table(int(max_total_len), 128, float(rotary_base), float(rope_scale), qkv.device)
    head = (qkv.data_ptr(), seq_lens.data_ptr(), past_lens.data_ptr())
    tail = (padding_offset.data_ptr(), kv_pointers.data_ptr(), qkv.shape[0], B, kv_pointers.shape[2], int(head_num),
            int(kv_head_num), 128, int(max_seq_len), int(tokens_per_block), table.data_ptr(), table.shape[0], int(cyclic_len),
            _lib.current_stream())
    if rope_offsets is None:
        rc = _lib.lib().omni_kv4_prefill_write_at(*head, *tail)
    else:
        rc = _lib.lib().omni_kv4_prefill_write_at_pos(*head, rope_offsets.data_ptr(), *tail)
    _lib.check(rc, what)


def kv4_prefill_write_at(qkv, seq_lens, past_lens, padding_offset, kv_pointers, head_num, kv_head_num, max_seq_len,
                         tokens_per_block, max_total_len, rotary_base=10000.0, rope_scale=1.0, cyclic_len=1 << 20):
    """apply_bias_rope_update_kv_cache (dense KV4 + zeros) for tokens that continue a sequence: token i of sequence b is
    position past_lens[b] + i (RoPE row, page, slot).  qkv fp16 [tokens, (Hq+2Hkv)*128] (q and k rotated in place), seq_lens /
    past_lens int32 [B] on the device, padding_offset = compute_padding_offsets(cu_seqlens, max_seq_len, tokens).
    max_total_len: the host's bound on max(past + len) -- the RoPE table is built for it (the lengths themselves stay on the
    device).  Same page bytes as the plain writer would leave for the same positions."""
    _kv4_prefill_write("fused_ext.kv4_prefill_write_at", qkv, seq_lens, past_lens, None, padding_offset, kv_pointers, head_num,
                       kv_head_num, max_seq_len, tokens_per_block, max_total_len, rotary_base, rope_scale, cyclic_len)


def _check_paged_attention_args(what, q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers, tokens_per_block):
    """The tensor checks that the attentions over quantised past + fresh tokens share (prefill_attention_paged_kv4,
    decode_attention_multi_kv4): one copy, so that the two raise the same errors.  -> (B, tokens_per_block)."""
    _lib.require_cuda(q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers)
    if q.dtype != torch.float16 or q.dim() != 3 or q.shape[-1] != 128:
        raise RuntimeError("%s: q must be fp16 [tokens, heads, 128]" % what)
    for t in (k_new, v_new):
        if t.dtype != torch.float16 or t.dim() != 3 or t.shape[-1] != 128 or t.shape[0] != q.shape[0]:
            raise RuntimeError("%s: k_new / v_new must be fp16 [tokens, kv heads, 128] with q's token count" % what)
    for t in (q, k_new, v_new):
        if t.stride(2) != 1 or t.stride(1) != 128:
            raise RuntimeError("%s: heads must be contiguous (token-strided views are fine)" % what)
    if k_new.shape[1] != v_new.shape[1] or k_new.shape[1] < 1 or q.shape[1] % k_new.shape[1] != 0:
        raise RuntimeError("%s: the q heads must be a multiple of the kv heads" % what)
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.shape[0] < 1:
        raise RuntimeError("%s: cu_seqlens_q must be int32 [B+1]" % what)
    B = cu_seqlens_q.shape[0] - 1
    _check_lens(cu_seqlens_q, B + 1, what, "cu_seqlens_q")
    _check_lens(past_lens, B, what, "past_lens")
    if kv_pointers.dtype != torch.int64 or kv_pointers.dim() != 3 or kv_pointers.shape[0] != B or kv_pointers.shape[1] != 2 \
            or not kv_pointers.is_contiguous():
        raise RuntimeError("%s: kv_pointers must be a contiguous int64 [B,2,blocks] tensor" % what)
    tpb = int(tokens_per_block)
    if tpb < 16 or tpb & (tpb - 1):
        raise RuntimeError("%s: tokens_per_block must be a power of two >= 16" % what)
    return B, tpb


def prefill_attention_paged_kv4(q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers, tokens_per_block, max_seqlen_q,
                                causal=True, head_mask_type=None, streaming_info=None):
    """Causal prefill attention whose first past_lens[b] keys / values of sequence b come from the KV4 pages (fp16 dequant, as the
    decode attention reads them) and whose last len_q keys / values are the call's own fp16 k_new / v_new -- the page slots of
    those tokens are not read.  q [Lq, Hq, 128], k_new / v_new [Lq, Hkv, 128] fp16 with contiguous heads (token-strided views of
    the qkv buffer, already rotated by kv4_prefill_write_at); cu_seqlens_q int32 [B+1], past_lens int32 [B], kv_pointers int64
    [B, 2, blocks].  -> out fp16 [Lq, Hq, 128].  Dense heads and the causal mask only."""
    what = "fused_ext.prefill_attention_paged_kv4"
    if not causal:
        raise NotImplementedError("%s: only the causal mask is implemented" % what)
    if head_mask_type is not None or streaming_info is not None:
        raise NotImplementedError("%s: streaming heads are not implemented (all heads are dense)" % what)
    B, tpb = _check_paged_attention_args(what, q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers, tokens_per_block)
    out = torch.empty((q.shape[0], q.shape[1], 128), dtype=torch.float16, device=q.device)
    if q.shape[0] == 0 or B == 0:
        return out
    rc = _lib.lib().omni_prefill_attention_paged_kv4(
        out.data_ptr(), q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), q.stride(0), k_new.stride(0), v_new.stride(0),
        cu_seqlens_q.data_ptr(), past_lens.data_ptr(), kv_pointers.data_ptr(), B, kv_pointers.shape[2], tpb,
        int(max_seqlen_q), q.shape[1], k_new.shape[1], 128, _lib.current_stream())
    _lib.check(rc, what)
    return out


# ---- multi-token decode step: split-KV attention for 1 - 8 new tokens over the KV4 pages -------------
DECODE_MULTI_MAX_Q = 8


class DecodeMultiTooManyTokens(ValueError):
    """decode_attention_multi_kv4 serves at most DECODE_MULTI_MAX_Q new tokens per sequence (longer chunks: the paged prefill)."""


def decode_attention_multi_kv4_set_split_override(nsplit):
    """Tuning / test hook: force the KV split count of decode_attention_multi_kv4 (at most 16); 0: the planner decides."""
    _lib.lib().omni_decode_attention_multi_kv4_set_split_override(int(nsplit))


def _workspace_bytes_of(name):
    def workspace_bytes(batch, num_heads, max_seqlen_q, max_past):
        size = getattr(_lib.lib(), "omni_%s_workspace_bytes" % name)
        return int(size(int(batch), int(num_heads), int(max_seqlen_q), int(max_past)))
    return workspace_bytes


decode_attention_multi_kv4_workspace_bytes = _workspace_bytes_of("decode_attention_multi_kv4")


def _decode_attention_multi(name, limit, too_many, q, k_new, v_new, cu_seqlens_q, past_lens, tree_mask, kv_pointers,
                            tokens_per_block, max_seqlen_q, max_past, workspace):
    """decode_attention_multi_kv4 (tree_mask None: the chain entry) and decode_attention_tree_kv4: the checks, the workspace
    and the call.  name: the public function's, which is also the C entry's behind "omni_"; limit / too_many: its token limit
    and the exception past it."""
    what = "fused_ext." + name
    if int(max_seqlen_q) > limit:
        raise too_many("%s: max_seqlen_q = %d, at most %d new tokens per sequence" % (what, int(max_seqlen_q), limit))
    _lib.require_cuda(workspace, tree_mask)
    B, tpb = _check_paged_attention_args(what, q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers, tokens_per_block)
    if tree_mask is not None:
        _check_lens(tree_mask, q.shape[0], what, "tree_mask")
    if int(max_past) < 0 or int(max_past) > kv_pointers.shape[2] * tpb:
        raise RuntimeError("%s: max_past must be non-negative and fit the block table" % what)
    out = torch.empty((q.shape[0], q.shape[1], 128), dtype=torch.float16, device=q.device)
    if q.shape[0] == 0 or B == 0 or int(max_seqlen_q) < 1:
        return out
    if workspace is None:
        workspace = _lib.workspace(_workspace_bytes_of(name)(B, q.shape[1], max_seqlen_q, max_past), q.device,
                                   "decode_multi")
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise RuntimeError("%s: workspace must be a contiguous uint8 tensor" % what)
    rc = getattr(_lib.lib(), "omni_" + name)(
        out.data_ptr(), q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), q.stride(0), k_new.stride(0), v_new.stride(0),
        cu_seqlens_q.data_ptr(), past_lens.data_ptr(), *(() if tree_mask is None else (tree_mask.data_ptr(),)),
        kv_pointers.data_ptr(), B, kv_pointers.shape[2], tpb, int(max_seqlen_q), q.shape[1], k_new.shape[1], 128, int(max_past),
        workspace.data_ptr(), workspace.numel(), _lib.current_stream())
    _lib.check(rc, what)
    return out


def decode_attention_multi_kv4(q, k_new, v_new, cu_seqlens_q, past_lens, kv_pointers, tokens_per_block, max_seqlen_q, max_past,
                               workspace=None):
    """prefill_attention_paged_kv4 for 0 - 8 new tokens per sequence against a long past: one sweep of a kv head's pages serves
    all of its q heads and all new tokens, and the past is split over workgroups (merged in a fixed order: same inputs, same
    bits).  Same tensors and checks as prefill_attention_paged_kv4; max_seqlen_q <= 8 bounds the new tokens per sequence and
    max_past bounds past_lens (the host's numbers: the lengths stay on the device).  workspace: uint8 device tensor of at
    least decode_attention_multi_kv4_workspace_bytes(...) bytes, allocated (and kept) here when None.
    -> out fp16 [Lq, Hq, 128]."""
    return _decode_attention_multi("decode_attention_multi_kv4", DECODE_MULTI_MAX_Q, DecodeMultiTooManyTokens, q, k_new, v_new,
                                   cu_seqlens_q, past_lens, None, kv_pointers, tokens_per_block, max_seqlen_q, max_past, workspace)


# ---- tree verify: masked multi-token attention, RoPE depths, KV4 compaction --------------------------
DECODE_TREE_MAX_Q = 32


class DecodeTreeTooManyTokens(ValueError):
    """decode_attention_tree_kv4 serves at most DECODE_TREE_MAX_Q new tokens (tree nodes) per sequence."""


def tree_masks(parents):
    """Ancestor masks and depths of a token tree.  parents: int tensor [n] or [B, n] (one tree per row), parents[..., 0] = -1 (the
    root: the pending token) and 0 <= parents[..., i] < i behind it; n <= 32.  -> (mask int32, depth int32), parents' shape:
    mask[i] = mask[parents[i]] | 1 << i (the node and its ancestors: the word decode_attention_tree_kv4 takes, bit 31 in the sign)
    and depth[i] = depth[parents[i]] + 1 (the RoPE offset kv4_prefill_write_at_pos takes).  Pure tensor arithmetic on the
    parents' device; the check of the parents reads their values."""
    p = torch.as_tensor(parents)
    if p.dim() not in (1, 2) or p.dtype not in (torch.int32, torch.int64) or p.shape[-1] < 1:
        raise ValueError("tree_masks: parents must be an int32 / int64 [n] or [B, n] tensor")
    n = p.shape[-1]
    if n > DECODE_TREE_MAX_Q:
        raise DecodeTreeTooManyTokens("tree_masks: %d nodes, at most %d" % (n, DECODE_TREE_MAX_Q))
    p2 = p.reshape(-1, n).to(torch.int64)
    idx = torch.arange(n, device=p2.device)
    if not bool(((p2[:, 0] == -1) & ((p2[:, 1:] >= 0) & (p2[:, 1:] < idx[1:])).all(dim=1)).all()):
        raise ValueError("tree_masks: parents[0] must be -1 and 0 <= parents[i] < i behind it")
    mask = torch.ones_like(p2)
    depth = torch.zeros_like(p2)
    for i in range(1, n):
        par = p2[:, i:i + 1]
        mask[:, i] = mask.gather(1, par).squeeze(1) | (1 << i)
        depth[:, i] = depth.gather(1, par).squeeze(1) + 1
    mask = torch.where(mask >= (1 << 31), mask - (1 << 32), mask)      # bit 31 -> the sign bit of the int32 word
    return mask.to(torch.int32).reshape(p.shape), depth.to(torch.int32).reshape(p.shape)


decode_attention_tree_kv4_workspace_bytes = _workspace_bytes_of("decode_attention_tree_kv4")


def decode_attention_tree_kv4(q, k_new, v_new, cu_seqlens_q, past_lens, tree_mask, kv_pointers, tokens_per_block, max_seqlen_q,
                              max_past, workspace=None):
    """decode_attention_multi_kv4 over a token tree, 0 - 32 new tokens per sequence: the row of token i sees the whole past and
    the fresh key j of its own sequence iff bit j of tree_mask[token i] is set and j < len_q (tree_masks(parents): a node sees its
    ancestors and itself; siblings do not see each other).  tree_mask: contiguous int32 [tokens] device tensor in q's token order
    (never read on the host).  The chain's masks give decode_attention_multi_kv4's bits.  Everything else -- tensors, checks,
    max_past, the workspace (decode_attention_tree_kv4_workspace_bytes) and the split override -- is decode_attention_multi_kv4's.
    -> out fp16 [Lq, Hq, 128]."""
    if tree_mask is None:
        raise RuntimeError("fused_ext.decode_attention_tree_kv4: tree_mask must be a contiguous int32 [tokens] tensor")
    return _decode_attention_multi("decode_attention_tree_kv4", DECODE_TREE_MAX_Q, DecodeTreeTooManyTokens, q, k_new, v_new,
                                   cu_seqlens_q, past_lens, tree_mask, kv_pointers, tokens_per_block, max_seqlen_q, max_past,
                                   workspace)


def kv4_prefill_write_at_pos(qkv, seq_lens, past_lens, rope_offsets, padding_offset, kv_pointers, head_num, kv_head_num,
                             max_seq_len, tokens_per_block, max_total_len, rotary_base=10000.0, rope_scale=1.0,
                             cyclic_len=1 << 20):
    """kv4_prefill_write_at with the RoPE row decoupled from the slot: token i of sequence b is written to page / slot
    past_lens[b] + i and rotated (q and k in place) at RoPE row past_lens[b] + rope_offsets[token].  rope_offsets: contiguous int32
    [tokens] device tensor (a tree node's depth, 0 <= depth <= i: tree_masks).  Same checks as kv4_prefill_write_at; the RoPE
    table is built for max_total_len, the host's bound on max(past + len), which covers past + depth."""
    if rope_offsets is None:
        raise RuntimeError("fused_ext.kv4_prefill_write_at_pos: rope_offsets must be a contiguous int32 [tokens] tensor")
    _kv4_prefill_write("fused_ext.kv4_prefill_write_at_pos", qkv, seq_lens, past_lens, rope_offsets, padding_offset, kv_pointers,
                       head_num, kv_head_num, max_seq_len, tokens_per_block, max_total_len, rotary_base, rope_scale, cyclic_len)


def kv4_compact_rows(kv_pointers, base_lens, src, counts, tokens_per_block, num_kv_heads):
    """Move the KV4 rows of an accepted tree path to the front: for every sequence b, kv head, K and V pool and j < counts[b] the
    row (64 code bytes, fp16 scale, fp16 zero point) at position base_lens[b] + src[b, j] goes to position base_lens[b] + j,
    byte-exact, across pages where need be; nothing else changes.  kv_pointers int64 [B, 2, blocks]; base_lens, counts int32 [B];
    src int32 [B, max_rows], max_rows <= 32 -- device tensors, never read on the host.  Contract (not checked): src[b] strictly
    increasing with src[b, j] >= j (a path through a tree whose nodes were written in index order), base + src inside the block
    table.  A destination may be another move's source (path 0, 2, 3): all rows are read before any is written."""
    what = "fused_ext.kv4_compact_rows"
    _lib.require_cuda(kv_pointers, base_lens, src, counts)
    if kv_pointers.dtype != torch.int64 or kv_pointers.dim() != 3 or kv_pointers.shape[1] != 2 or not kv_pointers.is_contiguous():
        raise RuntimeError("%s: kv_pointers must be a contiguous int64 [B,2,blocks] tensor" % what)
    B = kv_pointers.shape[0]
    _check_lens(base_lens, B, what, "base_lens")
    _check_lens(counts, B, what, "counts")
    if src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != B or not src.is_contiguous():
        raise RuntimeError("%s: src must be a contiguous int32 [B, max_rows] tensor" % what)
    if src.shape[1] < 1 or src.shape[1] > DECODE_TREE_MAX_Q:
        raise DecodeTreeTooManyTokens("%s: %d rows per sequence, at most %d" % (what, src.shape[1], DECODE_TREE_MAX_Q))
    if B == 0:
        return
    rc = _lib.lib().omni_kv4_compact_rows(kv_pointers.data_ptr(), base_lens.data_ptr(), src.data_ptr(), counts.data_ptr(), B,
                                          kv_pointers.shape[2], int(tokens_per_block), int(num_kv_heads), 128, src.shape[1],
                                          _lib.current_stream())
    _lib.check(rc, what)
