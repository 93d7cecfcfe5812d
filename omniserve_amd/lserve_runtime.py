"""Decode-step driver for the LServe configuration of BASELINE.json (configs[3]: Llama-3-8B-1048k, W8A8, long context,
batch 1, half of the kv heads streaming, dynamic page selection) on one MI355X.

Not an engine: like omniserve_amd/runtime.py it wires the kernels in the order of the reference's decoder layer
(omniserve/modeling/models/llama_w8a8_unpad.py:276-345,382-427 and omniserve/modeling/layers/decoding_attention.py:
dynamic_select_topk_pages :88-142, forward_w_dynamic_sparse_per_tensor :239-306 / the fine_grained twin :356-421) on
synthetic weights and synthetic cache pages, so that the a10-a12 rows of SURVEY.md 8 (and f-2, the per-tensor KV8
family the reference's published LServe numbers use) are timed end to end:

    rms_norm_general -> qkv W8A8 GEMM -> [every `interval` steps: page selector -> max over sub-chunks -> top-k pages]
    -> sparse single_query_attention (retrieval heads: selected pages, streaming heads: sink + local ring)
    -> invoke_quant -> o_proj -> residual add -> rms_norm_general -> gate_up -> silu_and_mul -> invoke_quant -> down
    -> residual add ... x layers, then rms_norm -> fp16 lm_head -> argmax.

kv_format: "kv8" = per_tensor int8 pages (scripts/lserve_benchmark/launch.sh:6-7), "kv4" = fine_grained KV4 pages
(BASELINE.json configs[3] as written).  The cache pages are random bytes with sane tails / statistics: the cost of the
step does not depend on their values.  All calls go through the mirrored `omniserve_backend.*` modules.
"""
from __future__ import annotations

import torch

from .backend import (activation_ops, fused_attention_ctx_pool, fused_attention_fine_grained_dense,
                      fused_attention_fine_grained_sparse, fused_attention_per_tensor_dense,
                      fused_attention_per_tensor_sparse, fused_attention_selector, fused_ext, fused_kernels, layernorm_ops,
                      prefill_attn, qgemm_w8a8)
from .rope import rope_table
from .runtime import LlamaConfig, SamplingState
from . import _lib


def head_rank_table(retrieval_head_flags):
    """Index of every kv head inside its class (ctx_attn_init.py:58-81 `transform_sequence`): retrieval heads
    (flag 1) and streaming heads (flag 0) are numbered separately in head order."""
    rank, nr, ns = [], 0, 0
    for f in retrieval_head_flags:
        if f:
            rank.append(nr); nr += 1
        else:
            rank.append(ns); ns += 1
    return rank


class W8A8Linear:
    """Synthetic W8A8 weights in the reference layout (w8a8_linear.py:38-60): int8 [N, K] row-major + fp16 scale [N]."""

    def __init__(self, n, k, gen, device):
        self.n, self.k = n, k
        self.weight = torch.randint(-127, 128, (n, k), dtype=torch.int8, device=device, generator=gen)
        self.dequant_scale = (torch.rand((n,), device=device, generator=gen) * 0.0012 + 0.0002).half()

    def forward(self, x_i8, scales, out):
        qgemm_w8a8.w8a8_gemm_forward_cuda(x_i8, self.weight, self.dequant_scale, scales, out)

    def weight_bytes(self):
        return self.weight.numel()


class LServeDecodeRunner(SamplingState):
    """One sequence per batch entry with `context` cached tokens; step() decodes one token per sequence."""

    def __init__(self, cfg: LlamaConfig, batch: int, context: int, max_new: int, device, seed=0, kv_format="kv8",
                 streaming_ratio=0.5, sink=128, local=256, budget_tokens=4096, selector_interval=4,
                 sub_chunk_per_block=4, use_graph=True, fused=True, prefetch_mb=None, ctx_sink=128, ctx_local=8192,
                 prefetch_blocks=160, arm_o=False, defer=True, qkv_slabs=True, rowfree=True, sampling=False):
        """fused: use the opt-in fused entry points (residual add + norm + quant, silu*mul + quant) -- bit-identical to the
        reference call sequence, three launches fewer per layer.  fused=True (or 3) also takes the
        row-kernel-free forms where they apply (batch <= 16: the attention merge leaves fp16 + row maxima, gate_up runs
        with the SiLU*mul epilogue, o_proj / down_proj quantise on the fly -- runtime.py's fusion level 3 for the W8A8
        layers); fused=2 keeps the quantiser row kernels.  prefetch_mb / prefetch_blocks / arm_o / defer / qkv_slabs / rowfree: the
        A/B switches of the step (this module reads no environment).  sampling=True: tokens are drawn by fused_ext.sample
        instead of arg-max (runtime.DecodeRunner's switch: parameters start greedy, set_sampling() changes them in place)."""
        c = cfg
        self.cfg, self.B, self.device = cfg, batch, device
        self._init_sampling(sampling, batch, device, seed)      # (read by the captured steps; u is refilled outside the graphs)
        if self.sampling:
            _lib.workspace(_lib.lib().omni_sample_workspace_bytes(batch, c.vocab), device, "sample")
        self.fused = bool(fused)
        level = 3 if fused is True else int(fused)
        # L2 weight prefetch riding on the row kernels (see omniserve_amd/runtime.py; a hint, results unaffected)
        prefetch_default = prefetch_mb is None
        if prefetch_mb is None:
            # round 2 (quantiser row kernels as carriers): 4-5 % SLOWER at batch 1 with W8A8 weights, so it was off; with the
            # row-kernel-free layer (norms and the wide merge as the carriers) 24-64 MiB measure 1.5-2 % FASTER per step
            # (3.11-3.13 -> 3.05-3.07 ms, tools/r03_call60/61.sh); 8-16 MiB are neutral
            prefetch_mb = 32.0 if self.fused else 0.0
        self.prefetch_bytes = int(float(prefetch_mb) * (1 << 20)) if self.fused else 0
        self.prefetch_blocks = int(prefetch_blocks)
        # (the wide merge as a carrier for o_proj's 16.8 MB costs it 2.8 us where o_proj gains 1.1: 3.07 -> 3.05 ms without)
        self.arm_o = bool(arm_o)
        if kv_format not in ("kv8", "kv4"):
            raise ValueError("kv_format must be 'kv8' (per_tensor) or 'kv4' (fine_grained)")
        self.kv8 = kv_format == "kv8"
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        d, Hq, Hk = c.head_dim, c.heads, c.kv_heads
        self.tpb = 64
        self.sub = self.tpb // sub_chunk_per_block            # tokens per sub-chunk
        self.interval = int(selector_interval)
        self.budget_tokens = int(budget_tokens)
        self.budget_pages = min(max(3, budget_tokens // self.tpb), context // self.tpb + 1)   # <= pages of the history
        ns = int(round(Hk * streaming_ratio))
        nr = Hk - ns
        # alternate head classes like a DuoAttention pattern file would (attn_patterns/*/full_attention_heads.tsv)
        flags = [1 if (i % 2 == 0 and i // 2 < nr) or (i % 2 == 1 and i // 2 >= ns) else 0 for i in range(Hk)]
        if sum(flags) != nr:
            flags = [1] * nr + [0] * ns
        rank = head_rank_table(flags)
        self.nr, self.ns = nr, ns
        self.flags = torch.tensor(flags, dtype=torch.int32, device=device)
        self.rank = torch.tensor(rank, dtype=torch.int32, device=device)
        self.sink, self.local = sink, local
        # context stage (ctx_attn_init.py:28-50): 0 = dense causal head, -1 = sink + local tokens only
        g = Hq // Hk
        self.head_mask_type = torch.tensor([0 if flags[h // g] else -1 for h in range(Hq)], dtype=torch.int32, device=device)
        self.streaming_info = torch.tensor([ctx_sink, ctx_local] * Hq, dtype=torch.int32, device=device)
        self.pooling_heads_idx = torch.tensor([h for h in range(Hk) if flags[h]], dtype=torch.int32, device=device)
        self.sink_blocks = (sink + self.tpb - 1) // self.tpb
        self.local_blocks = local // self.tpb + 1              # attn_config.py:63-64
        self.row = d if self.kv8 else d // 2                   # bytes of one token row of one head
        qkv_n = (Hq + 2 * Hk) * d
        self.layers = []
        for _ in range(c.layers):
            self.layers.append(dict(
                ln1=(1.0 + 0.05 * torch.randn(c.hidden, device=device, generator=gen)).half(),
                ln2=(1.0 + 0.05 * torch.randn(c.hidden, device=device, generator=gen)).half(),
                qkv=W8A8Linear(qkv_n, c.hidden, gen, device), o=W8A8Linear(c.hidden, Hq * d, gen, device),
                gate_up=W8A8Linear(2 * c.inter, c.hidden, gen, device), down=W8A8Linear(c.hidden, c.inter, gen, device)))
        self.final_norm = torch.ones(c.hidden, device=device).half()
        self.embed = (0.02 * torch.randn(c.vocab, c.hidden, device=device, generator=gen)).half()
        self.lm_head = (0.02 * torch.randn(c.vocab, c.hidden, device=device, generator=gen)).half()

        # ---- page pools (cache_engine.py:231-300): retrieval pool (K pages carry min/max statistics) and the
        # streaming ring, per layer ------------------------------------------------------------------------------
        self.max_context = context + max_new + 1
        rpages = (self.max_context + self.tpb - 1) // self.tpb
        spages = self.sink_blocks + self.local_blocks
        subs = self.tpb // self.sub

        def pool(n_pages, heads, stats):
            data = heads * self.tpb * self.row
            tail = 2 * heads * self.tpb * 2
            extra = 2 * subs * heads * d * 2 if stats else 0
            p = torch.empty((n_pages, data + tail + extra), dtype=torch.uint8, device=device)
            p[:, :data] = torch.randint(0, 256, (n_pages, data), dtype=torch.uint8, device=device, generator=gen)
            t = p[:, data:data + tail].view(torch.float16).view(n_pages, 2, heads * self.tpb)
            t[:, 0] = 0.25 * (0.5 + torch.rand((n_pages, heads * self.tpb), device=device, generator=gen))
            t[:, 1] = 7.5
            if stats:   # kmax > kmin, magnitudes of post-RoPE keys
                st = p[:, data + tail:].view(torch.float16).view(n_pages, 2, subs * heads * d)
                base = torch.randn((n_pages, subs * heads * d), device=device, generator=gen)
                st[:, 0] = (base + 1.0).half()
                st[:, 1] = (base - 1.0).half()
            return p

        def table(kp, vp, n_pages_per_seq):
            tab = torch.empty((batch, 2, n_pages_per_seq), dtype=torch.int64, device=device)
            for i, p in enumerate((kp, vp)):
                perm = torch.randperm(p.shape[0], device=device, generator=gen).view(batch, n_pages_per_seq)
                tab[:, i] = p.data_ptr() + perm * p.shape[1]
            return tab

        self.pools, self.retr_tables, self.strm_tables = [], [], []
        for _ in range(c.layers):
            rk, rv = pool(batch * rpages, max(nr, 1), True), pool(batch * rpages, max(nr, 1), False)
            sk, sv = pool(batch * spages, max(ns, 1), False), pool(batch * spages, max(ns, 1), False)
            self.pools.append((rk, rv, sk, sv))
            self.retr_tables.append(table(rk, rv, rpages))
            self.strm_tables.append(table(sk, sv, spages))
        self.kv_qo = torch.tensor([0.03, 0.035], dtype=torch.float32, device=device)   # kv_scale_quant_orig (K, V)
        self.kv_oq = (1.0 / self.kv_qo).contiguous()

        B, f16, i8 = batch, torch.float16, torch.int8
        self.x = torch.empty((B, c.hidden), dtype=f16, device=device)
        self.q_hidden = torch.empty((B, c.hidden), dtype=i8, device=device)
        self.q_inter = torch.empty((B, c.inter), dtype=i8, device=device)
        self.q_attn = torch.empty((B, Hq * d), dtype=i8, device=device)
        self.act_scale = torch.empty((B,), dtype=f16, device=device)
        self.act_sum = torch.empty((B,), dtype=f16, device=device)    # by-product of the fused entry points, unused
        self.act_scale2 = torch.empty((B,), dtype=f16, device=device)  # scales written by the quant-type kernels
        # fused: o_proj / down_proj leave int32 split-K slabs; the next add+norm kernel applies the GEMM epilogue
        self.defer = self.fused and bool(defer)
        self.slab = torch.empty((16 << 20,), dtype=torch.uint8, device=device) if self.defer else None
        # the qkv projection as slabs consumed by the attention kernel (fused_ext.decode_arm_qkv_slabs) on the steps
        # without a selector refresh: no slab epilogue launch behind the (96, 2)-workgroup qkv GEMV
        self.qkv_slabs = self.defer and bool(qkv_slabs)
        # row-kernel-free decode layer (fused level 3): needs the deferred epilogue (slab consumers) and <= 16 rows
        # (and plans its entry points accept: omni_gemm_rowfree_ok, W8A8 form)
        self.rowfree = (self.defer and level >= 3 and B <= 16 and Hq % 4 == 0 and
                        bool(rowfree) and
                        _lib.lib().omni_gemm_rowfree_ok(B, c.hidden, Hq * d, c.inter, 2) == 1)
        if prefetch_default and not self.rowfree:
            self.prefetch_bytes = 0     # (with the quantiser row kernels as carriers the prefetch measured slower)
        if self.rowfree:
            self.attn_f16 = torch.empty((B, Hq * d), dtype=f16, device=device)
            self.amax = torch.zeros((c.layers, 2, fused_ext.AMAX_WORDS), dtype=torch.int32, device=device)
        self.qkv_buf = torch.empty((B, qkv_n), dtype=f16, device=device)
        self.proj_buf = torch.empty((B, c.hidden), dtype=f16, device=device)
        self.gate_up_buf = torch.empty((B, 2 * c.inter), dtype=f16, device=device)
        self.mlp_act = torch.empty((B, c.inter), dtype=f16, device=device)
        self.normed = torch.empty((B, c.hidden), dtype=f16, device=device)
        self.context0 = context
        self.lengths = torch.full((B,), context, dtype=torch.int32, device=device)
        self.tokens = torch.randint(0, c.vocab, (B,), device=device, generator=gen)
        # cached page selection per layer (decoding_attention.py: cached_dynamic_sparse_page_idx)
        npick = self.budget_pages
        self.page_idx = [torch.zeros((B, Hq, npick), dtype=torch.int32, device=device) for _ in range(c.layers)]
        rope_table(self.max_context + 1, d, c.rope_theta, 1.0, device)
        self.use_graph = use_graph
        self.graphs = {}
        self.steps_done = 0

    def _arm(self, lin, deferred=False):
        if self.prefetch_bytes > 0:
            # (| 0x20: the W8A8 GEMVs keep their non-temporal loads, the arrangement this driver was measured with)
            fused_ext.prefetch_arm_gemm(lin.weight, self.B, lin.n, lin.k, 2 | 0x20, deferred, self.prefetch_bytes,
                                        self.prefetch_blocks)

    # one decode step; `select` = this step refreshes the page selection (every `interval`-th step upstream)
    def _eager_step(self, hist: int, select: bool):
        try:
            self._eager_step_body(hist, select)
        finally:
            if self.qkv_slabs:      # a step that raised between arming and the attention launch must not leave the
                fused_ext.decode_arm_qkv_slabs(None, 0, 0, 0, 0, 0, 0, None, None)   # one-shot descriptor armed

    def _eager_step_body(self, hist: int, select: bool):
        """hist = upper bound of the history length of this step's page bucket (the kernels take the true lengths from
        `self.lengths`; `hist` only sizes RoPE tables, split plans and the selector's padded output)."""
        c, B = self.cfg, self.B
        Hq, Hk, d = c.heads, c.kv_heads, c.head_dim
        if self.fused:     # embedding rows + lengths += 1 + the step's row-maximum slots zeroed: one launch
            fused_ext.decode_step_begin(self.x, self.embed, self.tokens, self.lengths, self.amax if self.rowfree else None)
        else:
            self.lengths.add_(1)
            torch.index_select(self.embed, 0, self.tokens, out=self.x)
        sc = self.act_scale                      # scales written by the norm kernels
        sq = self.act_scale2 if self.fused else sc   # ... by the quantisers (kept apart: a deferred epilogue reads them)
        pending = None                           # (sk, linear) of a down_proj whose epilogue is deferred
        nl = len(self.layers)
        attn = fused_attention_per_tensor_sparse if self.kv8 else fused_attention_fine_grained_sparse
        size_r, size_s = self.nr * self.row, self.ns * self.row
        total_pages = hist // self.tpb + 1
        sm = None          # W8A8: nobody reads a row sum (rms_norm_general / invoke_quant upstream): the fused kernels skip it
        rowfree = self.rowfree
        for li, L in enumerate(self.layers):
            self._arm(L["qkv"])
            if pending is not None:       # residual += down_proj(previous layer) [deferred epilogue], norm + quant
                fused_ext.splitk_w8_add_rms_norm_general_fuse_sum(self.q_hidden, self.x, self.slab, pending[0],
                                                                  pending[1].dequant_scale, sq, L["ln1"], sm, sc, c.eps)
                pending = None
            elif self.fused and li > 0:   # residual += down_proj(previous layer), then norm + quant
                fused_ext.add_rms_norm_general_fuse_sum(self.q_hidden, self.x, self.proj_buf, L["ln1"], sm, sc, c.eps)
            else:
                layernorm_ops.rms_norm_general(self.q_hidden, self.x, L["ln1"], sc, c.eps, True)
            if self.qkv_slabs and not select:   # slabs only: the attention applies the projection's epilogue (the page
                lin = L["qkv"]                  # selector of a refresh step reads fp16 q / k: regular GEMM there)
                sk_q = fused_ext.gemm_partial_w8a8(self.q_hidden, lin.weight, self.slab)
                fused_ext.decode_arm_qkv_slabs(self.slab, sk_q, B, lin.n, 0, Hq * d, (Hq + Hk) * d, lin.dequant_scale, sc)
            else:
                L["qkv"].forward(self.q_hidden, sc, self.qkv_buf)
            q = self.qkv_buf[:, : Hq * d].view(B, Hq, d)
            k = self.qkv_buf[:, Hq * d:(Hq + Hk) * d].view(B, Hk, d)
            v = self.qkv_buf[:, (Hq + Hk) * d:].view(B, Hk, d)
            if select:
                stats = fused_attention_selector.single_query_page_selector(
                    q, k, v, self.retr_tables[li], self.strm_tables[li], self.flags, self.rank, None, self.lengths,
                    None, self.max_context, self.tpb, size_r, size_s, self.sink, self.local, self.sink_blocks,
                    self.local_blocks, self.nr, self.ns, hist, d, c.rope_theta, 1.0, True, not self.kv8, True,
                    self.sub, self.nr * d, 1000000)
                npick = self.budget_pages
                if self.fused:      # one kernel for the torch view / max / topk / cat / to(int32) sequence
                    fused_ext.select_topk_pages(self.page_idx[li], stats, self.tpb // self.sub, total_pages, npick - 1)
                else:
                    stats = stats.view(B, Hq, -1, self.tpb // self.sub).max(dim=-1).values
                    _, idx = stats[:, :, : total_pages - 1].topk(k=npick - 1, dim=-1)
                    self.page_idx[li][:, :, : npick - 1].copy_(idx)
                    self.page_idx[li][:, :, npick - 1].fill_(total_pages - 1)
            # (no refresh: the cached selection is used as it is, decoding_attention.py:259-260 -- also across a page
            #  boundary, where its last entry is then the previous page, full, and the new page is first selected at the
            #  next refresh)
            common = (self.tpb, size_r, size_s, self.sink, self.local, self.sink_blocks, self.local_blocks, self.nr,
                      self.ns, hist + 1, d, c.rope_theta, 1.0, True, not self.kv8, not self.kv8, self.sub, self.nr * d,
                      2048)
            if rowfree:         # merge as a wide kernel (fp16 + row maxima); o_proj quantises on the fly
                if self.arm_o:
                    self._arm(L["o"], True)
                fused_ext.sparse_decode_attention_f16_amax(
                    self.attn_f16, self.amax[li, 0], q, k, v, self.retr_tables[li], self.strm_tables[li], self.flags,
                    self.rank, self.page_idx[li], self.lengths, self.tpb, size_r, size_s, self.sink, self.local,
                    self.sink_blocks, self.local_blocks, self.nr, self.ns, hist + 1, c.rope_theta, 1.0, self.sub,
                    self.kv_qo if self.kv8 else None, self.kv_oq if self.kv8 else None)
            elif self.fused:    # merge of the KV splits fused into the per-token quantiser (one launch less)
                self._arm(L["o"], self.defer)
                fused_ext.sparse_decode_attention_quant(
                    self.q_attn, sm, sq, q, k, v, self.retr_tables[li], self.strm_tables[li], self.flags, self.rank,
                    self.page_idx[li], self.lengths, self.tpb, size_r, size_s, self.sink, self.local, self.sink_blocks,
                    self.local_blocks, self.nr, self.ns, hist + 1, c.rope_theta, 1.0, self.sub,
                    self.kv_qo if self.kv8 else None, self.kv_oq if self.kv8 else None)
            elif self.kv8:
                out = attn.single_query_attention(q, k, v, self.kv_qo, self.kv_oq, self.retr_tables[li],
                                                  self.strm_tables[li], self.flags, self.rank, self.page_idx[li],
                                                  self.lengths, None, self.max_context, *common)
            else:
                out = attn.single_query_attention(q, k, v, self.retr_tables[li], self.strm_tables[li], self.flags,
                                                  self.rank, self.page_idx[li], self.lengths, None, self.max_context,
                                                  *common)
            if not self.fused:
                fused_kernels.invoke_quant(self.q_attn, out.view(B, Hq * d), sq)
            if rowfree:
                sk = fused_ext.gemm_partial_f16_w8a8(self.attn_f16, self.amax[li, 0], L["o"].weight, self.slab, sq)
            elif self.defer:
                sk = fused_ext.gemm_partial_w8a8(self.q_attn, L["o"].weight, self.slab)
            else:
                L["o"].forward(self.q_attn, sq, self.proj_buf)
            if not (rowfree and li < nl - 1):     # (the SiLU-epilogue form pairs gate / up rows: no prefetch descriptor)
                self._arm(L["gate_up"])
            # (letting that norm carry the head of down_proj's 58.7 MB instead measured slower: 3.09 -> 3.21 ms per step)
            if self.defer:
                fused_ext.splitk_w8_add_rms_norm_general_fuse_sum(self.q_hidden, self.x, self.slab, sk,
                                                                  L["o"].dequant_scale, sq, L["ln2"], sm, sc, c.eps)
            elif self.fused:
                fused_ext.add_rms_norm_general_fuse_sum(self.q_hidden, self.x, self.proj_buf, L["ln2"], sm, sc, c.eps)
            else:
                self.x.add_(self.proj_buf)
                layernorm_ops.rms_norm_general(self.q_hidden, self.x, L["ln2"], sc, c.eps, True)
            if rowfree and li < nl - 1:     # gate_up with the SiLU*mul epilogue; down_proj quantises on the fly
                G = L["gate_up"]
                fused_ext.gemm_silu_w8a8(self.q_hidden, G.weight, G.dequant_scale, sc, self.mlp_act, self.amax[li, 1])
                pending = (fused_ext.gemm_partial_f16_w8a8(self.mlp_act, self.amax[li, 1], L["down"].weight, self.slab,
                                                           sq), L["down"])
                continue
            L["gate_up"].forward(self.q_hidden, sc, self.gate_up_buf)
            self._arm(L["down"], self.defer and li < nl - 1)
            if self.fused:
                fused_ext.silu_mul_quant_fuse_sum(self.q_inter, self.gate_up_buf, sm, sq)
            else:
                activation_ops.silu_and_mul(self.mlp_act, self.gate_up_buf)
                fused_kernels.invoke_quant(self.q_inter, self.mlp_act, sq)
            if self.defer and li < nl - 1:
                pending = (fused_ext.gemm_partial_w8a8(self.q_inter, L["down"].weight, self.slab), L["down"])
            else:
                L["down"].forward(self.q_inter, sq, self.proj_buf)
                if not self.fused or li == nl - 1:
                    self.x.add_(self.proj_buf)
        layernorm_ops.rms_norm(self.normed, self.x, self.final_norm, c.eps, False)
        self._pick(torch.matmul(self.normed, self.lm_head.t()))

    # ---- context stage ------------------------------------------------------------------------------------------------
    def prefill(self, tokens=None, hidden=None, seq_len=None, chunk=16384):
        """The reference's context stage (llama_w8a8_unpad.py:253-313,382-427) over `batch` prompts of `seq_len` tokens each
        (default: the `context` the runner was built for; model_runner.py:262-360 builds the same metadata): per layer
        norm + quant -> qkv W8A8 GEMM -> RoPE in place + cache write (every token of a retrieval head, sink + local ring of a
        streaming head) -> min/max statistics of the retrieval heads' keys -> varlen causal attention with the Lambda mask
        on streaming heads -> quant -> o_proj -> residual -> norm + quant -> gate_up / SiLU*mul + quant / down in chunks of
        `chunk` tokens (model_config.chunk_prefill_size) -> residual.  The synthetic page contents are overwritten; the
        decode state (lengths, next tokens from the last position's logits) is set so that step() continues the sequences.
        Input: `tokens` int64 [batch*seq_len] (embedding lookup) or `hidden` fp16 [batch*seq_len, hidden].
        Returns the final hidden states [batch*seq_len, hidden]."""
        c, B, dev = self.cfg, self.B, self.device
        Hq, Hk, d = c.heads, c.kv_heads, c.head_dim
        Lp = int(seq_len) if seq_len is not None else self.context0
        if Lp < 1 or Lp + 1 > self.max_context:
            raise ValueError("seq_len %d does not fit the pools (max_context %d)" % (Lp, self.max_context))
        T = B * Lp
        f16, i8 = torch.float16, torch.int8
        if hidden is not None:
            x = hidden.to(dev, f16).clone()
        else:
            if tokens is None:
                g = torch.Generator(device=dev)
                g.manual_seed(1234)
                tokens = torch.randint(0, c.vocab, (T,), device=dev, generator=g)
            x = torch.index_select(self.embed, 0, tokens.to(dev))
        if tuple(x.shape) != (T, c.hidden):
            raise ValueError("prefill input must cover batch * seq_len = %d tokens" % T)
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * Lp
        lens = torch.full((B,), Lp, dtype=torch.int32, device=dev)
        slens = torch.full((B,), min(Lp, self.sink + self.local), dtype=torch.int32, device=dev)
        pad = fused_attention_fine_grained_dense.compute_padding_offsets(cu, Lp, T)
        q_hidden = torch.empty((T, c.hidden), dtype=i8, device=dev)
        q_attn = torch.empty((T, Hq * d), dtype=i8, device=dev)
        scale = torch.empty((T,), dtype=f16, device=dev)
        qkv = torch.empty((T, (Hq + 2 * Hk) * d), dtype=f16, device=dev)
        proj = torch.empty((T, c.hidden), dtype=f16, device=dev)
        ch = min(int(chunk), T)
        gate_up = torch.empty((ch, 2 * c.inter), dtype=f16, device=dev)
        mlp_act = None if self.fused else torch.empty((ch, c.inter), dtype=f16, device=dev)
        q_inter = torch.empty((ch, c.inter), dtype=i8, device=dev)
        size_r, size_s = self.nr * self.row, self.ns * self.row
        sums = None        # W8A8: no row sums (the fused entry points skip them when given None)
        nl = len(self.layers)
        for li, L in enumerate(self.layers):
            if self.fused and li > 0:      # residual += down_proj(previous layer), norm + quant: one pass over x
                fused_ext.add_rms_norm_general_fuse_sum(q_hidden, x, proj, L["ln1"], sums, scale, c.eps)
            else:
                layernorm_ops.rms_norm_general(q_hidden, x, L["ln1"], scale, c.eps, True)
            L["qkv"].forward(q_hidden, scale, qkv)
            tail = (self.retr_tables[li], self.strm_tables[li], self.flags, self.rank, Hq, Hk, Lp, self.tpb, size_r, size_s,
                    self.sink, self.local, self.sink_blocks, self.local_blocks, self.nr, self.ns, d, c.rope_theta, 1.0,
                    self.max_context + 1, True, not self.kv8, not self.kv8)
            if self.kv8:
                fused_attention_per_tensor_dense.apply_bias_rope_update_kv_cache(qkv, self.kv_oq, lens, slens, pad, *tail)
            else:
                fused_attention_fine_grained_dense.apply_bias_rope_update_kv_cache(qkv, lens, slens, pad, *tail)
            q = qkv[:, : Hq * d].view(T, Hq, d)
            k = qkv[:, Hq * d:(Hq + Hk) * d].view(T, Hk, d)
            v = qkv[:, (Hq + Hk) * d:].view(T, Hk, d)
            if self.nr > 0:       # sparse decode mode: the page selector's statistics (llama_w8a8_unpad.py:290-294)
                fused_attention_ctx_pool.paged_min_max_pool(k.contiguous(), self.retr_tables[li], cu, self.pooling_heads_idx,
                                                            Lp, self.sub, self.tpb, size_r, True)
            if self.ns > 0:
                out = prefill_attn.token_streaming_attn_func(q, k, v, cu, cu, self.head_mask_type, self.streaming_info, Lp, Lp)
            else:
                out = prefill_attn.flash_attn_varlen_func(q, k, v, cu, cu, Lp, Lp, dropout_p=0.0, causal=True)
            fused_kernels.invoke_quant(q_attn, out.view(T, Hq * d), scale)
            L["o"].forward(q_attn, scale, proj)
            if self.fused:
                fused_ext.add_rms_norm_general_fuse_sum(q_hidden, x, proj, L["ln2"], sums, scale, c.eps)
            else:
                x.add_(proj)
                layernorm_ops.rms_norm_general(q_hidden, x, L["ln2"], scale, c.eps, True)
            for s0 in range(0, T, ch):
                n = min(ch, T - s0)
                L["gate_up"].forward(q_hidden[s0:s0 + n], scale[s0:s0 + n], gate_up[:n])
                if self.fused:             # SiLU*mul + quant without the fp16 round trip (bit-identical)
                    fused_ext.silu_mul_quant_fuse_sum(q_inter[:n], gate_up[:n], sums, scale[:n])
                else:
                    activation_ops.silu_and_mul(mlp_act[:n], gate_up[:n])
                    fused_kernels.invoke_quant(q_inter[:n], mlp_act[:n], scale[:n])
                L["down"].forward(q_inter[:n], scale[:n], proj[s0:s0 + n])
            if not self.fused or li == nl - 1:
                x.add_(proj)
        # decode state: the sequences now hold Lp tokens; the next token comes from the last position of each prompt
        self.context0, self.steps_done = Lp, 0
        self.lengths.fill_(Lp)
        self.graphs.clear()
        npick = min(max(3, self.budget_tokens // self.tpb), Lp // self.tpb + 1)
        if npick != self.budget_pages:
            self.budget_pages = npick
            self.page_idx = [torch.zeros((B, Hq, npick), dtype=torch.int32, device=dev) for _ in self.layers]
        last = x[Lp - 1::Lp].contiguous()
        layernorm_ops.rms_norm(self.normed, last, self.final_norm, c.eps, False)
        self._refill_u()
        self._pick(torch.matmul(self.normed, self.lm_head.t()))
        return x

    def step(self):
        """Decode one token.  Two HIP graphs (with / without page selection) per history length bucket: the page
        count only changes every 64 tokens, and the benchmark runs far fewer steps than that."""
        bucket = (self.context0 + self.steps_done) // self.tpb
        hist = (bucket + 1) * self.tpb - 1          # largest history length with the same page count
        # decoding_attention.py:259: refresh when nothing is cached yet (first step after the context stage) or when the
        # length INCLUDING the token being generated (model_runner.py:388-400 -> max_seq_len) is a multiple of the interval
        select = self.steps_done == 0 or (self.context0 + self.steps_done + 1) % self.interval == 0
        self._refill_u()
        if not self.use_graph:
            self._eager_step(hist, select)
            self.steps_done += 1
            return
        if bucket + 1 < self.budget_pages:
            # (cannot happen after __init__ / prefill() sized budget_pages; kept as a guard for hand-made states)
            raise RuntimeError("page budget larger than the history's page count")
        if hist + 1 <= self.budget_tokens and bucket + 1 > self.budget_pages:
            # decoding_attention.py:99-100 attends EVERY page while the history fits the token budget; this driver keeps a
            # fixed number of selected pages per head (the benchmark's regime: history >> budget)
            raise NotImplementedError("history within the dynamic-sparse token budget and growing past the page count the "
                                      "runner was sized for: re-run prefill() or build the runner for the longer context")
        key = (bucket, select)
        g = self.graphs.get(key)
        if g is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                saved = (self.lengths.clone(), self.tokens.clone(), [p.clone() for p in self.page_idx])
                self._eager_step(hist, select)
                self.lengths.copy_(saved[0]); self.tokens.copy_(saved[1])
                for p, q in zip(self.page_idx, saved[2]):
                    p.copy_(q)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._eager_step(hist, select)
            self.graphs[key] = g
            # the capture itself did not execute: replay below does
        g.replay()
        self.steps_done += 1

    def weight_bytes_per_step(self):
        return sum(L[k].weight_bytes() for L in self.layers for k in ("qkv", "o", "gate_up", "down"))
