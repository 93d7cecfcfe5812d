"""Minimal decode-step driver for the QServe W4A8KV4 Llama path on one MI355X.

Not an engine: it only wires the kernels in the order of the reference's decoder layer
(omniserve/modeling/models/llama_w4a8_unpad.py:406-438) on synthetic weights so
that bench.py / smoke() can time the hot path named by BASELINE.json:

    rms_norm_general_fuse_sum -> qkv GEMM -> single_query_attention (RoPE + KV4 append fused)
    -> invoke_quant_fuse_sum -> o_proj GEMM -> residual add -> rms_norm_general_fuse_sum
    -> gate_up GEMM -> silu_and_mul -> invoke_quant_fuse_sum -> down GEMM -> residual add
    ... x num_layers, then rms_norm -> fp16 lm_head -> argmax  (llama_w4a8_unpad.py:485-488,556-563)

All calls go through the mirrored `omniserve_backend.*` modules, i.e. through the C ABI.
The whole step is captured in one HIP graph (the reference launches ~322 kernels per step
eagerly; at MI355X speeds the step is launch-bound otherwise).
"""
from __future__ import annotations

import collections
import dataclasses

import torch

from .backend import (activation_ops, fused_attention_fine_grained_dense, fused_attention_pure_dense, fused_ext, fused_kernels,
                      layernorm_ops, qgemm_w4a8_per_chn, qgemm_w4a8_per_group)
from .rope import rope_table
from . import _lib


@dataclasses.dataclass
class LlamaConfig:
    hidden: int = 4096
    inter: int = 14336
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    layers: int = 32
    vocab: int = 128256
    rope_theta: float = 500000.0
    eps: float = 1e-5
    group_size: int = -1          # -1 = per-channel, 128 = g128

    @staticmethod
    def llama3_8b(group_size=-1):
        return LlamaConfig(group_size=group_size)

    @staticmethod
    def llama2_70b(group_size=-1):
        return LlamaConfig(hidden=8192, inter=28672, heads=64, kv_heads=8, layers=80, vocab=32000, rope_theta=10000.0,
                           group_size=group_size)

    @staticmethod
    def yi_34b(group_size=-1):
        """Yi-34B: 56 q heads over 8 kv heads -- a GQA ratio of 7 (28 / 4 on a TP = 2 shard), which the decode attention serves
        with ragged head tiles (csrc/kv_cache.hip).  hidden 7168 is past the level-3 gate (omni_gemm_rowfree_ok): level 2."""
        return LlamaConfig(hidden=7168, inter=20480, heads=56, kv_heads=8, layers=60, vocab=64000, rope_theta=5000000.0,
                           group_size=group_size)

    @staticmethod
    def tiny():
        return LlamaConfig(hidden=512, inter=1024, heads=4, kv_heads=2, layers=2, vocab=512)


class W4A8Linear:
    """Synthetic packed weights in the reference layout (w4a8_linear.py:43-100).  Any byte pattern
    is a valid packing of uniform random 4-bit codes, so the weights are drawn on the device."""

    def __init__(self, n, k, group_size, gen, device):
        self.n, self.k, self.group = n, k, group_size
        self.qweight = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device=device, generator=gen).view(torch.int8)
        self.s1_scales = (torch.rand((n,), device=device, generator=gen) * 0.018 + 0.002).half()
        if group_size != -1:
            # level-2 weights span +-120 instead of +-15: keep the synthetic model's activations in fp16 range
            self.s1_scales = (self.s1_scales.float() / 8.0).half()
        if group_size == -1:
            zeros = torch.randint(0, 16, (n,), device=device, generator=gen).half()
            self.s1_szeros = (zeros * self.s1_scales).half()
        else:
            ng = k // group_size
            s2 = torch.randint(1, 9, (ng, n), device=device, generator=gen)
            z = torch.randint(0, 16, (ng, n), device=device, generator=gen)
            self.s2_scales = s2.to(torch.int8)
            self.s2_zeros = (-(z * s2)).to(torch.int8)

    def forward(self, x_i8, scales, sums, out):
        if self.group == -1:
            qgemm_w4a8_per_chn.gemm_forward_cuda(x_i8, self.qweight, self.s1_scales, scales, self.s1_szeros, sums, out)
        else:
            qgemm_w4a8_per_group.gemm_forward_cuda(x_i8, self.qweight, self.s2_zeros, self.s2_scales,
                                                   self.s1_scales, scales, out)

    def weight_bytes(self):
        b = self.qweight.numel()
        if self.group != -1:
            b += self.s2_scales.numel() + self.s2_zeros.numel()
        return b

    # ---- tensor-parallel shards of a full layer (omniserve_amd/tp.py has the granularity rules) ------------
    def select_rows(self, ranges):
        """Column-parallel shard: output channels [a,b) for (a,b) in ranges (multiples of 64), concatenated."""
        sh = object.__new__(W4A8Linear)
        cat = lambda t, dim: torch.cat([t.narrow(dim, a, b - a) for a, b in ranges], dim=dim).contiguous()
        sh.n, sh.k, sh.group = sum(b - a for a, b in ranges), self.k, self.group
        sh.qweight = cat(self.qweight, 0)
        sh.s1_scales = cat(self.s1_scales, 0)
        if self.group == -1:
            sh.s1_szeros = cat(self.s1_szeros, 0)
        else:
            sh.s2_scales, sh.s2_zeros = cat(self.s2_scales, 1), cat(self.s2_zeros, 1)
        return sh

    def shard_k(self, rank, world):
        """Row-parallel shard: the rank's slice of the reduction dimension (whole 128-k blocks)."""
        from . import tp
        sh = object.__new__(W4A8Linear)
        sh.n, sh.k, sh.group = self.n, self.k // world, self.group
        sh.qweight = tp.shard_qweight_k(self.qweight, rank, world)
        sh.s1_scales = self.s1_scales
        if self.group == -1:
            sh.s1_szeros = self.s1_szeros
        else:
            sh.s2_scales = tp.shard_group_params_k(self.s2_scales, rank, world, self.group)
            sh.s2_zeros = tp.shard_group_params_k(self.s2_zeros, rank, world, self.group)
        return sh


def accept_lengths(draft, pred):
    """Tokens per sequence that a multi-token step keeps.  draft int64 [B, n]: column 0 the pending token, columns 1 .. the
    drafted continuation; pred int64 [B, n]: the model's token behind draft[b, :j + 1].  m[b] = 1 + the number of LEADING j
    with draft[b, j + 1] == pred[b, j] (a match behind a mismatch does not count): the pending token is always kept, and each
    drafted token as long as it is what the model would have produced.  Pure tensor arithmetic (CPU or device).  -> int64 [B]."""
    match = (draft[:, 1:] == pred[:, :-1]).to(torch.int64)
    return 1 + torch.cumprod(match, dim=1).sum(dim=1)


def accept_sampled(probe_prob, u_acc, drawn):
    """The rejection rule of speculative sampling for a deterministic draft, the sampled counterpart of accept_lengths.
    probe_prob f32 [B, n]: probe_prob[b, j] = the probability of the drafted token draft[b, j + 1] under the target's filtered
    distribution behind draft[b, :j + 1] (column n - 1 is not read: nothing is drafted behind it); u_acc f32 [B, n]: uniforms
    in [0, 1); drawn int64 [B, n]: drawn[b, j] = a draw from that distribution WITHOUT the drafted token (column n - 1: an
    unrestricted draw).  Drafted token j + 1 is accepted while u_acc[b, j] < probe_prob[b, j], LEADING accepts only (an accept
    behind a rejection does not count); m = 1 + accepts; the next pending token is drawn[b, m - 1]: at the rejection point the
    draw without the rejected token -- for a one-hot draft distribution q the residual norm(max(p - q, 0)) is p with the
    drafted token removed, so the output is distributed exactly as p --, behind a fully accepted draft the unrestricted draw.
    Pure tensor arithmetic (CPU or device).  -> (m int64 [B], next int64 [B])."""
    B, n = drawn.shape
    ok = (u_acc[:, : n - 1] < probe_prob[:, : n - 1]).to(torch.int64)
    m = 1 + torch.cumprod(ok, dim=1).sum(dim=1)
    return m, drawn.gather(1, (m - 1).view(B, 1)).squeeze(1)


def accept_paths(parents, tokens, pred):
    """The accepted path per sequence through a verified token tree.  parents int [n]: one topology for the batch, parents[0] =
    -1, parents[i] < i; tokens int64 [B, n]: the nodes' tokens (node 0 = the pending token); pred int64 [B, n]: the model's
    token behind node i's path.  Start at node 0, which is always kept; from node c take the LOWEST-index child j with
    tokens[b, j] == pred[b, c]; stop when there is none (a match below a rejected node is never reached).  -> (path int64
    [B, n]: the kept nodes in order, strictly increasing, padded with -1; m int64 [B]: how many).  For chain parents m ==
    accept_lengths(tokens, pred).  Pure tensor arithmetic (CPU or device, no host read)."""
    B, n = tokens.shape
    dev = tokens.device
    par = torch.as_tensor(parents, device=dev).to(torch.int64).view(1, n)
    idx = torch.arange(n, device=dev).view(1, n)
    cur = torch.zeros((B,), dtype=torch.int64, device=dev)
    alive = torch.ones((B,), dtype=torch.bool, device=dev)
    path = torch.full((B, n), -1, dtype=torch.int64, device=dev)
    path[:, 0] = 0
    m = torch.ones((B,), dtype=torch.int64, device=dev)
    for step in range(1, n):
        want = pred.gather(1, cur.view(B, 1))
        cand = (par == cur.view(B, 1)) & (tokens == want) & alive.view(B, 1)
        nxt = torch.where(cand, idx, n).min(dim=1).values
        alive = nxt < n
        cur = torch.where(alive, nxt, cur)
        path[:, step] = torch.where(alive, nxt, -1)
        m = m + alive.to(torch.int64)
    return path, m


ScoreResult = collections.namedtuple("ScoreResult", "logprob rank top_tokens top_logprobs")


def perplexity(logprob, mask=None):
    """exp(-mean log-probability) per sequence: logprob [B, n] (DecodeRunner.score's), mask bool [B, n] (None: every position
    counts) -> f64 [B].  A -inf log-probability gives inf.  Pure tensor arithmetic (CPU or device)."""
    lp = logprob.to(torch.float64)
    if mask is None:
        return torch.exp(-lp.mean(dim=1))
    keep = mask.to(torch.bool)
    total = torch.where(keep, lp, torch.zeros_like(lp)).sum(dim=1)
    return torch.exp(-total / keep.sum(dim=1).to(torch.float64))


class SamplingState:
    """Sampled decoding's state and its two operations, for DecodeRunner and lserve_runtime.LServeDecodeRunner (a mixin: the
    runners keep the attributes).  The per-row parameters and the draw u live in device tensors that a captured step READS, so
    changing them needs no re-capture; u is refilled outside the graph before each step from a generator of its own (the
    model's generator draws the same weights / prompts whether the runner samples or not).  Needs self.tokens."""

    def _init_sampling(self, sampling, batch, device, seed):
        """The parameters start at temperature 0, i.e. greedy.  (The sampler's workspace is the runner's to pre-size.)"""
        self.sampling = bool(sampling)
        if self.sampling:
            self.s_temperature = torch.zeros((batch,), dtype=torch.float32, device=device)
            self.s_top_k = torch.zeros((batch,), dtype=torch.int32, device=device)
            self.s_top_p = torch.ones((batch,), dtype=torch.float32, device=device)
            self.s_u = torch.zeros((batch,), dtype=torch.float32, device=device)
            self.sample_gen = torch.Generator(device=device)
            self.sample_gen.manual_seed(seed)

    def set_sampling(self, temperature=None, top_k=None, top_p=None, seed=None):
        """Change the sampling parameters (a number for all sequences or one value per sequence) and / or reseed the draws.
        Written into the runner's device tensors in place: a captured step picks them up at its next replay."""
        if not self.sampling:
            raise RuntimeError("set_sampling needs a runner built with sampling=True")
        for dst, val in ((self.s_temperature, temperature), (self.s_top_k, top_k), (self.s_top_p, top_p)):
            if val is not None:
                dst.copy_(torch.as_tensor(val, dtype=dst.dtype).to(dst.device).expand(dst.shape))
        if seed is not None:
            self.sample_gen.manual_seed(int(seed))

    def _uniforms(self, *shape):
        return torch.rand(shape, dtype=torch.float32, device=self.s_u.device, generator=self.sample_gen)

    def _refill_u(self):
        """s_u <- one fresh draw per sequence (nothing on a greedy runner).  Never inside a capture: the replay reads s_u."""
        if self.sampling:
            self.s_u.copy_(self._uniforms(self.s_u.shape[0]))

    def _pick(self, logits, fused_argmax=True):
        """self.tokens <- one token per row of logits fp16 [B, vocab]: drawn with s_u, or on a greedy runner the arg-max
        (fused_ext.argmax, or torch's with fused_argmax=False: same result)."""
        if self.sampling:
            fused_ext.sample(self.tokens, logits, self.s_temperature, self.s_top_k, self.s_top_p, self.s_u)
        elif fused_argmax:
            fused_ext.argmax(self.tokens, logits)
        else:
            self.tokens.copy_(torch.argmax(logits, dim=-1))


class DecodeRunner(SamplingState):
    """bs sequences with `context` cached tokens each; step() decodes one token per sequence."""

    def __init__(self, cfg: LlamaConfig, batch: int, context: int, max_new: int, device, seed=0,
                 use_graph=True, fused=True, tp_rank=0, tp_size=1, tp_group=None, shard_full=False,
                 prefetch_mb=None, prefetch_blocks=160, weight_policy=1, tp_comm=None, max_fused=4, tp_l2_attn=True,
                 l3_prefetch_down=1, qkv_slabs="auto", attn_single=True, arm_qkv=True, arm_o=True, l3_last=True,
                 sampling=False, logprobs=None):
        """tp_size > 1: Megatron-style tensor parallelism (omniserve_amd/tp.py): qkv / gate_up column-parallel,
        o / down row-parallel, attention by kv head, one fp16 sum all-reduce of the [B, hidden] projection after
        o_proj and after down_proj.  shard_full=True builds the full layers from the seed and keeps this
        rank's shards (tests: every rank then holds shards of the SAME model); otherwise only the local shapes
        are drawn (bench: synthetic weights, no point in materialising 70B parameters per rank).
        The A/B switches of the decode step are constructor arguments (this module reads no environment): max_fused caps the
        fusion level the runner may pick; tp_l2_attn / qkv_slabs ("auto", True, False) / attn_single / arm_qkv / arm_o /
        l3_prefetch_down (0, 1, 2) / l3_last select the forms described where they are used below.
        sampling=True: every token is drawn by fused_ext.sample (temperature / top-p / top-k) instead of
        arg-max; the parameters start at temperature 0, i.e. greedy, and set_sampling() changes them.
        logprobs (None: off; 0: the pending token's log-probability and rank; N in 1 .. 20: the top N as well): after every method
        that sets self.tokens the buffers token_logprob f32 [B], token_rank i32 [B], top_tokens i64 [B, N] and top_logprobs f32
        [B, N] describe that token under the RAW distribution of the logits row it was picked from (fused_ext.logprobs, DESIGN.md
        section 4.6a) -- greedy or sampled alike.  Read-only: tokens and state are the same bits with or without it."""
        if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, int) or
                                     not 0 <= logprobs <= fused_ext.LOGPROB_MAX_TOP):
            raise ValueError("logprobs must be None or an integer in 0 .. %d, got %r" % (fused_ext.LOGPROB_MAX_TOP, logprobs))
        self.logprobs = logprobs
        self.cfg, self.B, self.device = cfg, batch, device
        self.tp_rank, self.tp_size, self.tp_group = int(tp_rank), int(tp_size), tp_group
        # tp_comm = "peer": the decode step's collectives run on the library's own peer-mapped all-reduce (tp.PeerComm: one
        # launch per collective, folded into the add + norm kernel where one follows) instead of torch.distributed / RCCL
        self.comm = None
        tp_comm = tp_comm or ""
        # ("peer": one / two shots by payload, csrc/tp_comm.h; "peer1" / "peer2": forced; "loopback[2]": one process, all peers =
        #  this rank -- timing only)
        if self.tp_size > 1 and tp_comm in ("peer", "peer1", "peer2", "loopback", "loopback2"):
            from . import tp
            algo = {"peer1": "one_shot", "peer2": "two_shot", "loopback2": "two_shot"}.get(tp_comm, "auto")
            self.comm = tp.PeerComm(self.tp_rank, self.tp_size, batch * cfg.hidden, device, tp_group,
                                    loopback=tp_comm.startswith("loopback"), algo=algo)
        if cfg.heads % self.tp_size or cfg.kv_heads % self.tp_size or cfg.inter % (128 * self.tp_size):
            raise ValueError("heads / kv_heads / intermediate size not divisible by the TP degree")
        self.hl, self.kl, self.il = cfg.heads // self.tp_size, cfg.kv_heads // self.tp_size, cfg.inter // self.tp_size
        # fused: 0/False = the reference call sequence; 1 = opt-in fused entry points (residual add +
        # norm + quant, silu*mul + quant); 2/True = additionally defer the split-K epilogue of o_proj /
        # down_proj into the following add+norm kernel.  All bit-identical to the reference sequence
        # (SURVEY.md 8f.1).
        # 3 = additionally NO quantiser row kernels: the gate_up GEMV
        # applies silu_and_mul in its epilogue and leaves the row maxima, the attention merge is a wide kernel that
        # leaves fp16 + row maxima, and o_proj / down_proj quantise their input on the fly (fused_ext.gemm_silu_*,
        # decode_attention_f16_amax, gemm_partial_f16_*): 7 kernels per layer instead of 9, same bits.
        # 3 is the default (fused=True) where it applies: batch <= 16, one GPU.
        # (A level 4 -- the MLP half of a layer as ONE persistent launch with in-kernel hand-offs -- was built in round 4, measured
        #  slower than level 3 (2.37 vs 2.17 ms per step) and moved out of the product: tools/experiments/mlp_fused.hip, HISTORY.md.)
        # 4 (round 6) = 3 with the two 1 -> N edges of the layer as single launches: (add + norm + quant) -> qkv and
        # (add + norm + quant) -> gate_up + SiLU (fused_ext.norm_gemm_fused, csrc/norm_gemv_fused.h: the rows and the GEMV's tiles in
        # one grid, the tiles request their whole weight part and then wait for the rows): 5 launches per layer, same bits.
        # Opt-in (fused=4): measured SLOWER than level 3 on the MI355X (2.24 vs 2.11 ms per step; profiles/r06_a: the hand-off --
        # write-through publish + a poll behind the tile CUs' own weight requests + the activation round trip -- costs what the
        # kernel boundary costs, and the rows run 1.5-3 us slower beside the stream), so fused=True still means level 3.
        want_pairs = fused is not True and int(fused) >= 4
        self.fused = 3 if fused is True else min(int(fused), 3)
        # the attention-side fusions of level 2 (split merge inside the quantiser, q / k / v from the qkv projection's slabs)
        # involve no row-parallel projection, so they also apply under tensor parallelism, where the level drops to 1
        self.l2_attn = self.fused >= 2 and batch <= 128 and bool(tp_l2_attn)
        if (self.tp_size > 1 or batch > 512) and self.fused > 1:
            # tensor parallel: the all-reduce needs the fp16 projection; batch > 512: the prefill tile's slab-only form
            # (omni_*_gemm_partial) stops there -- no deferred epilogue in either case.  (batch 129 .. 512: o_proj / down_proj
            # run on the 128 x 256 tile with K slices over grid.y and leave slabs for the norm, as at smaller batches)
            self.fused = 1
        # level 3 wants the plans its entry points accept (omni_gemm_rowfree_ok: the launchers' own conditions -- gate_up
        # without a grid-level K split, i.e. hidden <= 4096; one rider workgroup per row in a grid row of hidden / 64; the
        # rider's LDS copy of a row) and the wide attention merge's 4 heads per wave; otherwise level 2, which has no such
        # limits (a hidden = 5120 layer used to pass the old size test here and fail in its first step)
        if self.fused >= 3 and not (self.hl % 4 == 0 and int(max_fused) >= 3 and
                                    _lib.lib().omni_gemm_rowfree_ok(batch, cfg.hidden, self.hl * cfg.head_dim, self.il,
                                                                    0 if cfg.group_size == -1 else 1) == 1):
            self.fused = 2
        # L2 weight prefetch riding on the row kernels (fused extension; a hint, results are unaffected): MiB of the
        # next GEMV's weights each row kernel pulls into the L2s (0 = off), with how many extra workgroups, and
        # whether the GEMV on a prefetched tensor then uses plain instead of non-temporal weight loads (per call: the arm
        # names the tensor, omni_prefetch_arm_gemm; un-armed projections always stream non-temporally).  Defaults: on with the fused
        # entry points (prefetch_mb / prefetch_blocks / weight_policy arguments for sweeps).
        # level 4 where level 3 applies and both pair forms take the shapes (M <= 16, hidden <= 4096, grids resident at once)
        self.pairs = (want_pairs and self.fused >= 3 and int(max_fused) >= 4 and
                      fused_ext.norm_gemm_fused_ok(batch, (self.hl + 2 * self.kl) * cfg.head_dim, cfg.hidden, cfg.group_size, False) and
                      fused_ext.norm_gemm_fused_ok(batch, 2 * self.il, cfg.hidden, cfg.group_size, True))
        if prefetch_mb is None:
            # measured (profiles/r02_*): +6-7 % at bs = 16 with 28-40 MiB per row kernel (the L2s hold 32 MiB; the
            # excess lands in MALL), nothing at bs = 128, -4 % at bs = 64 where the row kernels are no longer idle
            # (batch 33..64: 12 MiB per carrier measured best at configs[2] -- 3.50 -> 3.43 ms per step, 24 MiB and more lose.
            #  A tensor-parallel shard's projections are small enough to be fetched whole: one Llama-2-70B TP = 8 rank at
            #  bs = 128 7.22-7.26 -> 6.59-6.65 ms per step with 12 .. 48 MiB.  Other batches > 64: not measured, off)
            dflt = 40.0 if batch <= 32 else (12.0 if batch <= 64 else (24.0 if self.tp_size > 1 else 0.0))
            prefetch_mb = dflt if self.fused else 0.0
        self.prefetch_bytes = int(float(prefetch_mb) * (1 << 20)) if self.fused else 0
        # (fetching workgroups per carrier: 240 was round 2's optimum; with down_proj's 29.6 MB on the norm in front of gate_up
        #  128-192 measure 1.7 % faster per step at bs = 16 -- 2.28 -> 2.24 ms --, 64-96 slower; bs = 64 / TP / LServe: flat)
        self.prefetch_blocks = int(prefetch_blocks)
        self.weight_policy = int(weight_policy) if self.prefetch_bytes > 0 else 0
        c = cfg
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        self.gen = gen
        d = c.head_dim
        hl, kl, il, r, w = self.hl, self.kl, self.il, self.tp_rank, self.tp_size
        qkv_n = (hl + 2 * kl) * d
        self.layers = []
        for _ in range(c.layers):
            ln1 = (1.0 + 0.05 * torch.randn(c.hidden, device=device, generator=gen)).half()
            ln2 = (1.0 + 0.05 * torch.randn(c.hidden, device=device, generator=gen)).half()
            if w > 1 and shard_full:
                qkv = W4A8Linear((c.heads + 2 * c.kv_heads) * d, c.hidden, c.group_size, gen, device).select_rows(
                    [(r * hl * d, (r + 1) * hl * d), (c.heads * d + r * kl * d, c.heads * d + (r + 1) * kl * d),
                     ((c.heads + c.kv_heads) * d + r * kl * d, (c.heads + c.kv_heads) * d + (r + 1) * kl * d)])
                o = W4A8Linear(c.hidden, c.heads * d, c.group_size, gen, device).shard_k(r, w)
                gate_up = W4A8Linear(2 * c.inter, c.hidden, c.group_size, gen, device).select_rows(
                    [(r * il, (r + 1) * il), (c.inter + r * il, c.inter + (r + 1) * il)])
                down = W4A8Linear(c.hidden, c.inter, c.group_size, gen, device).shard_k(r, w)
            else:
                qkv = W4A8Linear(qkv_n, c.hidden, c.group_size, gen, device)
                o = W4A8Linear(c.hidden, hl * d, c.group_size, gen, device)
                gate_up = W4A8Linear(2 * il, c.hidden, c.group_size, gen, device)
                down = W4A8Linear(c.hidden, il, c.group_size, gen, device)
            self.layers.append(dict(ln1=ln1, ln2=ln2, qkv=qkv, o=o, gate_up=gate_up, down=down))
        self.final_norm = torch.ones(c.hidden, device=device).half()
        self.embed = (0.02 * torch.randn(c.vocab, c.hidden, device=device, generator=gen)).half()
        self.lm_head = (0.02 * torch.randn(c.vocab, c.hidden, device=device, generator=gen)).half()

        # ---- paged KV4 cache: one K pool and one V pool per layer (cache_engine.py:117-136) ----
        self.tpb = 64
        self.max_context = context + max_new + 1
        pages_per_seq = (self.max_context + self.tpb - 1) // self.tpb
        self.page_bytes = kl * self.tpb * (c.head_dim // 2) + 2 * kl * self.tpb * 2
        n_pages = batch * pages_per_seq
        self.block_tables = []
        self.pools = []
        data_bytes = kl * self.tpb * (c.head_dim // 2)
        for _ in range(c.layers):
            pools = []
            tab = torch.empty((batch, 2, pages_per_seq), dtype=torch.int64, device=device)
            for kv in range(2):
                pool = torch.empty((n_pages, self.page_bytes), dtype=torch.uint8, device=device)
                pool[:, :data_bytes] = torch.randint(0, 256, (n_pages, data_bytes), dtype=torch.uint8,
                                                     device=device, generator=gen)
                tail = pool[:, data_bytes:].view(torch.float16).view(n_pages, 2, kl * self.tpb)
                tail[:, 0] = 0.25 * (0.5 + torch.rand((n_pages, kl * self.tpb), device=device, generator=gen))
                tail[:, 1] = 7.5
                perm = torch.randperm(n_pages, device=device, generator=gen).view(batch, pages_per_seq)
                tab[:, kv] = pool.data_ptr() + perm * self.page_bytes
                pools.append(pool)
            self.pools.append(pools)
            self.block_tables.append(tab)

        # ---- persistent activation buffers (the reference re-allocates them every step) ----------
        B = batch
        f16, i8 = torch.float16, torch.int8
        self.x = torch.empty((B, c.hidden), dtype=f16, device=device)
        self._q_hidden = torch.empty((B, c.hidden), dtype=i8, device=device)
        self._q_inter = torch.empty((B, il), dtype=i8, device=device)
        self._q_attn = torch.empty((B, hl * c.head_dim), dtype=i8, device=device)
        self.act_scale = torch.empty((B,), dtype=f16, device=device)   # written by norm kernels
        self.act_sum = torch.empty((B,), dtype=f16, device=device)
        self.act_scale2 = torch.empty((B,), dtype=f16, device=device)  # written by quant kernels
        self.act_sum2 = torch.empty((B,), dtype=f16, device=device)
        pws = _lib.lib().omni_gemm_partial_workspace_bytes     # (slab-only forms: at least one M x N slab up to 512 rows)
        need = max(int(pws(B, c.hidden, k)) for k in (hl * c.head_dim, il))
        need = max(need, int(pws(B, qkv_n, c.hidden)))     # (qkv slabs, see qkv_slabs)
        self.slab = torch.empty((max(need, 1 << 20),), dtype=torch.uint8, device=device)  # deferred split-K partial sums
        self.qkv_buf = torch.empty((B, qkv_n), dtype=f16, device=device)
        self.proj_buf = torch.empty((B, c.hidden), dtype=f16, device=device)
        self.gate_up_buf = torch.empty((B, 2 * il), dtype=f16, device=device)
        self.mlp_act = torch.empty((B, il), dtype=f16, device=device)
        self.attn_f16 = torch.empty((B, hl * c.head_dim), dtype=f16, device=device)
        # row-maximum candidates of the level-3 path: [layer][0 = attention output, 1 = MLP activation][AMAX_WORDS], zeroed once
        # per step (the producers raise them with atomicMax)
        # (one buffer with the level-4 hand-off words behind them: [layer][0 = norm -> qkv, 1 = norm -> gate_up][NGF_SYNC_WORDS]
        #  arrival counters + row pairs -- the step's first kernel zeroes all of it)
        n_amax = c.layers * 2 * fused_ext.AMAX_WORDS
        self._step_words = torch.zeros((n_amax + c.layers * 2 * fused_ext.NGF_SYNC_WORDS,), dtype=torch.int32, device=device)
        self.amax = self._step_words[:n_amax].view(c.layers, 2, fused_ext.AMAX_WORDS)
        self.ngf_sync = self._step_words[n_amax:].view(c.layers, 2, fused_ext.NGF_SYNC_WORDS)
        self.ngf_err = torch.zeros((4,), dtype=torch.int32, device=device)      # sticky: a hand-off wait gave up (check())
        self.tickets = fused_ext.new_tickets(device)      # ticket words of the single-launch attention (this runner's stream)
        self.ngf_clk = {}     # timeline probe (tools/pairs_ab.py): {(layer, site): int64 [grid, 8]} handed to that launch
        # level 3: the norm in front of gate_up prefetches ALL of DOWN's weights (29.6 MB fit the 32 MB of L2s) instead of
        # the head of gate_up's 58.7 MB; gate_up then streams cold with non-temporal loads (they do not displace the
        # prefetched lines) and down reads L2: 2.322-2.334 -> 2.294-2.314 ms per step on the same box (profiles/r03_g;
        # l3_prefetch_down=0: round 3's first arrangement, 2: gate_up with plain loads -- slower, 2.35)
        self.pf_down = int(l3_prefetch_down)
        # fused level >= 2: the qkv projection leaves int32 split-K slabs and the decode attention applies its epilogue in
        # its first load trip (fused_ext.decode_arm_qkv_slabs): no slab epilogue launch between the two.  "auto": on exactly
        # where the plain qkv GEMV's plan splits K (bs = 64: (96, 2) workgroups + a 4.9-us epilogue launch per layer; 3.51 ->
        # 3.47 ms per step); at bs = 16 the plan has no split and the slab form measured 1.5 % slower.  qkv_slabs=False / True
        # forces it off / on (A/B)
        if qkv_slabs == "auto":      # on exactly where the plain qkv GEMV would split K and launch a slab epilogue
            import ctypes
            sk_q = ctypes.c_int(1)
            _lib.lib().omni_gemm_get_plan(batch, qkv_n, c.hidden, 128 if c.group_size == 128 else 64, None, None,
                                          ctypes.byref(sk_q))
            want = sk_q.value > 1
        else:
            want = bool(qkv_slabs)
        self.qkv_slabs = (self.fused >= 2 or self.l2_attn) and want
        # (A/B knobs: qkv's / o_proj's weights prefetched by the norm in front of qkv / the kernel behind the attention)
        # level 3: the attention's split merge inside the attention launch (last-arriving workgroup; attn_single=False: the
        # two-launch form, A/B)
        self.attn_single = bool(attn_single)
        self.arm_qkv = bool(arm_qkv)
        self.arm_o = bool(arm_o)
        # level 3 also in the LAST layer: its down projection's slabs are consumed by the model's final norm
        # (fused_ext.splitk_add_rms_norm) instead of GEMV epilogue + residual add + rms_norm (l3_last=False: off, A/B)
        self.last_l3 = self.fused >= 3 and self.tp_size == 1 and self.comm is None and bool(l3_last)
        self.normed = torch.empty((B, c.hidden), dtype=f16, device=device)
        self.lengths = torch.full((B,), context, dtype=torch.int32, device=device)
        self.tokens = torch.randint(0, c.vocab, (B,), device=device, generator=gen)
        self._init_sampling(sampling, B, device, seed)
        if self.sampling:
            _lib.workspace(_lib.lib().omni_sample_workspace_bytes(8 * B, c.vocab), device, "sample")    # (verify: B * 8 rows)
        if self.logprobs is not None:
            self.token_logprob = torch.zeros((B,), dtype=torch.float32, device=device)
            self.token_rank = torch.zeros((B,), dtype=torch.int32, device=device)
            self.top_tokens = torch.full((B, self.logprobs), -1, dtype=torch.int64, device=device)
            self.top_logprobs = torch.zeros((B, self.logprobs), dtype=torch.float32, device=device)
            self._lse = torch.zeros((B,), dtype=torch.float32, device=device)
            # (verify_tree: B * 32 rows; sized now so that no later eager call moves the buffer a captured step points to)
            _lib.workspace(_lib.lib().omni_logprob_workspace_bytes(fused_ext.DECODE_TREE_MAX_Q * B, c.vocab, self.logprobs),
                           device, "logprob")
        self._score_rows = None       # score()'s tap on the context stage's rows (_next_from_last)
        self._prefill_bufs = None     # the context stage's activation buffers (_context_bufs)
        rope_table(self.max_context + 1, c.head_dim, c.rope_theta, 1.0, device)  # pre-build (capture safe)
        self.graph = None
        self.use_graph = use_graph
        self.graph_error = None       # set when a tensor-parallel graph capture failed and the runner fell back to eager
        self.steps_done = 0

    def step(self):
        """Decode one token for every sequence (one HIP-graph replay once captured)."""
        self._refill_u()      # outside the graph: the replay reads the buffer
        if not self.use_graph:
            self._eager_step()
            self.steps_done += 1
            return
        if self.graph is None:
            # warm up eagerly on a side stream (sizes the workspaces / RoPE table), roll the
            # sequence state back, then capture the identical step
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                saved = (self.lengths.clone(), self.tokens.clone())
                self._eager_step()
                self.lengths.copy_(saved[0])
                self.tokens.copy_(saved[1])
            torch.cuda.current_stream().wait_stream(s)
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._eager_step()
                self.graph = graph
            except RuntimeError as exc:  # (e.g. a collective that cannot be captured on this stack)
                if self.tp_size == 1:
                    raise
                import warnings
                warnings.warn("DecodeRunner: HIP-graph capture of the tensor-parallel step failed (%s); falling back to "
                              "eager launches" % exc)
                # tensor-parallel first contact: an RCCL all-reduce inside a captured HIP graph has never run on
                # hardware here; fall back to eager launches instead of losing the run, and say so
                torch.cuda.synchronize()
                self.use_graph = False
                self.graph_error = "%s: %s" % (type(exc).__name__, exc)
                if self.comm is not None:
                    self.comm.resync()      # the abandoned capture may have consumed an odd number of slots
                self.lengths.copy_(saved[0])
                self.tokens.copy_(saved[1])
                self._eager_step()
                self.steps_done += 1
                return
        self.graph.replay()
        self.steps_done += 1

    def check(self):
        """Raises if a peer wait of the last step timed out (tensor parallel, tp_comm = "peer").  Synchronises."""
        if self.comm is not None:
            self.comm.check_error()
        if self.pairs and int(self.ngf_err[0].item()) != 0:
            raise RuntimeError("DecodeRunner: a (norm -> GEMV) hand-off wait gave up (rows never arrived); the step's outputs "
                               "are NaN")

    def read_tokens(self):
        """The tokens of the last step on the host (synchronises).  Under tensor parallelism with the library's own
        collective this is also where a timed-out peer wait surfaces: the affected collectives returned NaN, the epoch did
        not advance, and this raises instead of handing back tokens computed from them."""
        toks = self.tokens.cpu()
        self.check()
        return toks

    def close(self):
        """Release the peer-mapped communication buffers (tensor parallel, tp_comm = "peer")."""
        if self.comm is not None:
            self.comm.close()
            self.comm = None

    def _partial(self, x_i8, lin):
        """o_proj / down_proj without its epilogue: int32 split-K slabs in self.slab, returns the slab count."""
        if lin.group == -1:
            return fused_ext.gemm_partial_per_chn(x_i8, lin.qweight, self.slab)
        return fused_ext.gemm_partial_per_group(x_i8, lin.qweight, lin.s2_zeros, lin.s2_scales, self.slab)

    def _partial_f16(self, act, amax, lin, sum_out, scale_out):
        """Level 3: o_proj / down_proj from fp16 activations + row maxima (codes computed inside the GEMV; sums / scales by
        rider workgroups): int32 split-K slabs in self.slab, returns the slab count."""
        if lin.group == -1:
            return fused_ext.gemm_partial_f16_per_chn(act, amax, lin.qweight, self.slab, sum_out, scale_out)
        return fused_ext.gemm_partial_f16_per_group(act, amax, lin.qweight, lin.s2_zeros, lin.s2_scales, self.slab,
                                                    sum_out, scale_out)

    def _consume(self, q_out, sk, lin, a_scale, a_sum, gamma, out_sum, out_scale):
        """residual += epilogue(sum of the slabs); norm + quant of it (the GEMM epilogue lives in this row kernel)."""
        if lin.group == -1:
            fused_ext.splitk_add_rms_norm_general_fuse_sum(q_out, self.x, self.slab, sk, lin.s1_scales, a_scale,
                                                           lin.s1_szeros, a_sum, gamma, out_sum, out_scale, self.cfg.eps)
        else:
            fused_ext.splitk_w8_add_rms_norm_general_fuse_sum(q_out, self.x, self.slab, sk, lin.s1_scales, a_scale, gamma,
                                                              out_sum, out_scale, self.cfg.eps)

    def _arm(self, lin, deferred=False, silu=False):
        """The next row kernel prefetches the head of `lin`'s weight stream into the L2s (no-op when disabled).
        silu: `lin` will run as fused_ext.gemm_silu_* (gate / up tile rows paired per workgroup)."""
        if self.prefetch_bytes > 0:      # (weight_policy 0: the consuming GEMV keeps its non-temporal loads -- A/B)
            fused_ext.prefetch_arm_gemm(lin.qweight, self.B, lin.n, lin.k,
                                        (0 if lin.group == -1 else 1) | (0x10 if silu else 0) | (0 if self.weight_policy else 0x20),
                                        deferred, self.prefetch_bytes, self.prefetch_blocks)

    def _eager_step(self):
        try:
            self._eager_step_body()
        finally:
            if self.prefetch_bytes > 0:
                fused_ext.prefetch_disarm()     # a step that raised may leave a descriptor armed
            if self.qkv_slabs:
                fused_ext.decode_arm_qkv_slabs(None, 0, 0, 0, 0, 0, 0, None, None)     # ... and the q / k / v slab source

    def _eager_step_body(self):
        # one decoder layer at decode shape = llama_w4a8_unpad.py:406-438
        c = self.cfg
        if self.fused:     # one launch: embedding rows (torch's index_select takes 12.6 us for 16 rows) + lengths += 1 + the
            fused_ext.decode_step_begin(self.x, self.embed, self.tokens, self.lengths,      # step's row-maximum slots zeroed
                                        self._step_words if self.fused >= 3 else None)
        else:
            self.lengths.add_(1)
            torch.index_select(self.embed, 0, self.tokens, out=self.x)
        B = self.B
        hq, hk, d = self.hl, self.kl, c.head_dim     # this rank's heads
        sA, mA = self.act_scale2, self.act_sum2   # scales / sums produced by quant-type kernels
        sB, mB = self.act_scale, self.act_sum     # ... by norm kernels
        per_chn = c.group_size == -1
        if not per_chn:    # g128: no activation sums anywhere (llama_w4a8_unpad.py:81,212-215,395-401): the reference calls
            mA = mB = None # rms_norm_general / invoke_quant, and the fused entry points skip the second row reduction
        pending = None                             # (sk, linear) of a down_proj whose epilogue is deferred
        nl = len(self.layers)
        for li, L in enumerate(self.layers):
            qa_h, qa_i = self._q_hidden, self._q_inter
            l3 = self.fused >= 3 and (li < nl - 1 or self.last_l3)     # row-kernel-free MLP half in this layer
            if self.pairs and l3:
                # level 4: (add + norm + quant) -> qkv as one launch (rows from the previous layer's down_proj slabs; first
                # layer: the embedding rows as they are)
                if pending is not None:
                    sk, lin = pending
                    fused_ext.norm_gemm_fused(qa_h, self.x, L["ln1"], mB, sB, c.eps, L["qkv"], self.qkv_buf, self.ngf_sync[li, 0],
                                              self.ngf_err, slab=self.slab, sk=sk, producer=lin, p_ascales=sA, p_asums=mA,
                                              clk=self.ngf_clk.get((li, 0)))
                    pending = None
                else:
                    fused_ext.norm_gemm_fused(qa_h, self.x, L["ln1"], mB, sB, c.eps, L["qkv"], self.qkv_buf, self.ngf_sync[li, 0],
                                              self.ngf_err)
            elif self.arm_qkv:
                self._arm(L["qkv"], deferred=self.qkv_slabs)
            if self.pairs and l3:
                pass
            elif pending is not None:     # residual += down_proj(prev layer) [deferred epilogue], norm + quant
                sk, lin = pending
                self._consume(qa_h, sk, lin, sA, mA, L["ln1"], mB, sB)
                pending = None
            elif self.fused and li > 0 and self.comm is not None:
                self.comm.add_rms_norm(qa_h, self.x, L["ln1"], mB, sB, c.eps)      # all-reduce(down_proj) + add + norm + quant
            elif self.fused and li > 0:
                fused_ext.add_rms_norm_general_fuse_sum(qa_h, self.x, self.proj_buf, L["ln1"], mB, sB, c.eps)
            elif per_chn:
                layernorm_ops.rms_norm_general_fuse_sum(qa_h, self.x, L["ln1"], mB, sB, c.eps, True)
            else:
                layernorm_ops.rms_norm_general(qa_h, self.x, L["ln1"], sB, c.eps, True)
            if self.pairs and l3:
                pass
            elif self.qkv_slabs:      # slabs only; the attention kernel reads q / k / v from them (qkv_buf: shapes only)
                lin = L["qkv"]
                fused_ext.decode_arm_qkv_slabs(self.slab, self._partial(qa_h, lin), B, lin.n, 0, hq * d, (hq + hk) * d,
                                               lin.s1_scales, sB, lin.s1_szeros if per_chn else None,
                                               mB if per_chn else None)
            else:
                L["qkv"].forward(qa_h, sB, mB, self.qkv_buf)
            q = self.qkv_buf[:, : hq * d].view(B, hq, d)
            k = self.qkv_buf[:, hq * d:(hq + hk) * d].view(B, hk, d)
            v = self.qkv_buf[:, (hq + hk) * d:].view(B, hk, d)
            if self.arm_o:
                self._arm(L["o"], deferred=self.fused >= 2)      # rides on the quantiser after the attention
            if self.fused >= 3:     # merge as a wide kernel (fp16 + row maxima); o_proj quantises on the fly
                fused_ext.decode_attention_f16_amax(self.attn_f16, self.amax[li, 0], q, k, v, self.block_tables[li],
                                                    self.lengths, self.tpb, self.max_context, c.rope_theta,
                                                    single_launch=self.attn_single, tickets=self.tickets)
            elif self.fused >= 2 or self.l2_attn:   # attention with its split merge fused into the activation quant
                fused_ext.decode_attention_quant_fuse_sum(self._q_attn, q, k, v, self.block_tables[li], self.lengths,
                                                          self.tpb, self.max_context, c.rope_theta, mA, sA)
            else:
                attn = fused_attention_pure_dense.single_query_attention(
                    q, k, v, self.block_tables[li], self.lengths, None, 65536, self.tpb, hk * d // 2,
                    self.max_context, d, c.rope_theta, True, True, True)
                if per_chn:
                    fused_kernels.invoke_quant_fuse_sum(self._q_attn, attn.view(B, hq * d), mA, sA)
                else:
                    fused_kernels.invoke_quant(self._q_attn, attn.view(B, hq * d), sA)
            if self.fused >= 2:
                if self.fused >= 3:
                    sk = self._partial_f16(self.attn_f16, self.amax[li, 0], L["o"], mA, sA)
                else:
                    sk = self._partial(self._q_attn, L["o"])
                if self.pairs and l3:
                    # level 4: (add + norm + quant) -> gate_up + SiLU as one launch; down_proj quantises on the fly
                    G = L["gate_up"]
                    fused_ext.norm_gemm_fused(qa_h, self.x, L["ln2"], mB, sB, c.eps, G, self.mlp_act, self.ngf_sync[li, 1],
                                              self.ngf_err, slab=self.slab, sk=sk, producer=L["o"], p_ascales=sA, p_asums=mA,
                                              amax=self.amax[li, 1], clk=self.ngf_clk.get((li, 1)))
                    pending = (self._partial_f16(self.mlp_act, self.amax[li, 1], L["down"], mA, sA), L["down"])
                    continue
                if l3 and self.pf_down:
                    self._arm(L["down"], deferred=True)
                else:
                    self._arm(L["gate_up"], silu=l3)
                self._consume(qa_h, sk, L["o"], sA, mA, L["ln2"], mB, sB)
            else:
                peer = self.comm is not None and self.fused
                proj = self.comm.slot(B * c.hidden, (B, c.hidden)) if peer else self.proj_buf
                L["o"].forward(self._q_attn, sA, mA, proj)
                if not peer:
                    self._all_reduce(self.proj_buf)
                self._arm(L["gate_up"])
                if peer:
                    self.comm.add_rms_norm(qa_h, self.x, L["ln2"], mB, sB, c.eps)  # all-reduce(o_proj) + add + norm + quant
                elif self.fused:
                    fused_ext.add_rms_norm_general_fuse_sum(qa_h, self.x, self.proj_buf, L["ln2"], mB, sB, c.eps)
                else:
                    self.x.add_(self.proj_buf)
                    if per_chn:
                        layernorm_ops.rms_norm_general_fuse_sum(qa_h, self.x, L["ln2"], mB, sB, c.eps, True)
                    else:
                        layernorm_ops.rms_norm_general(qa_h, self.x, L["ln2"], sB, c.eps, True)
            if l3:
                # gate_up with silu_and_mul in its epilogue -> fp16 activation + row maxima; down_proj quantises on the fly
                G = L["gate_up"]       # (pf_down: not the armed tensor -> streams cold, non-temporal; down_proj then reads L2)
                if per_chn:
                    fused_ext.gemm_silu_per_chn(qa_h, G.qweight, G.s1_scales, sB, G.s1_szeros, mB, self.mlp_act,
                                                self.amax[li, 1])
                else:
                    fused_ext.gemm_silu_per_group(qa_h, G.qweight, G.s2_zeros, G.s2_scales, G.s1_scales, sB,
                                                  self.mlp_act, self.amax[li, 1])
                pending = (self._partial_f16(self.mlp_act, self.amax[li, 1], L["down"], mA, sA), L["down"])
                continue
            L["gate_up"].forward(qa_h, sB, mB, self.gate_up_buf)
            self._arm(L["down"], deferred=self.fused >= 2 and li < nl - 1)
            if self.fused:
                fused_ext.silu_mul_quant_fuse_sum(qa_i, self.gate_up_buf, mA, sA)
            else:
                activation_ops.silu_and_mul(self.mlp_act, self.gate_up_buf)
                if per_chn:
                    fused_kernels.invoke_quant_fuse_sum(qa_i, self.mlp_act, mA, sA)
                else:
                    fused_kernels.invoke_quant(qa_i, self.mlp_act, sA)
            if self.fused >= 2 and li < nl - 1:
                pending = (self._partial(qa_i, L["down"]), L["down"])
            else:
                peer = self.comm is not None and self.fused
                L["down"].forward(qa_i, sA, mA, self.comm.slot(B * c.hidden, (B, c.hidden)) if peer else self.proj_buf)
                if peer and li == nl - 1:
                    self.comm.all_reduce(self.proj_buf)
                elif not peer:
                    self._all_reduce(self.proj_buf)     # (peer: consumed by the next layer's add + norm)
                if not self.fused or li == nl - 1:
                    self.x.add_(self.proj_buf)
        if pending is not None:     # the last layer's down projection: epilogue + residual add inside the final norm
            sk, lin = pending
            fused_ext.splitk_add_rms_norm(self.normed, self.x, self.slab, sk, lin.s1_scales, sA,
                                          lin.s1_szeros if per_chn else None, mA if per_chn else None, self.final_norm, c.eps)
        else:
            layernorm_ops.rms_norm(self.normed, self.x, self.final_norm, c.eps, False)
        logits = torch.matmul(self.normed, self.lm_head.t())
        if self.sampling:
            fused_ext.sample(self.tokens, logits, self.s_temperature, self.s_top_k, self.s_top_p, self.s_u)
        elif self.fused:
            fused_ext.argmax(self.tokens, logits)      # same result as torch.argmax, 6 us instead of 47
        else:
            self.tokens.copy_(torch.argmax(logits, dim=-1))
        self._record_logprobs(logits)

    # ---- log-probabilities ------------------------------------------------------------
    def _record_logprobs(self, logits):
        """The runner's buffers <- the pending tokens' log-probability, rank and the top N of logits fp16 [B, vocab], the rows they
        were picked from (nothing on a runner built without `logprobs`).  Two launches, capturable."""
        if self.logprobs is None:
            return
        top = self.logprobs > 0
        fused_ext.logprobs(logits, target=self.tokens, n_top=self.logprobs, lse=self._lse, token_logprob=self.token_logprob,
                           rank=self.token_rank, top_tokens=self.top_tokens if top else None,
                           top_logprobs=self.top_logprobs if top else None)

    def _logprobs_of(self, logits, pred):
        """verify() / verify_tree(): ONE call over all B * n logits rows with target = pred (None without `logprobs`)."""
        if self.logprobs is None:
            return None
        return fused_ext.logprobs(logits, target=pred.reshape(-1).contiguous(), n_top=self.logprobs)

    # ---- prefill (context stage) ---------------------------------------------------------------------------
    def _context_bufs(self, T):
        """T rows of each of the context stage's activation buffers (self._prefill_bufs).  Grow-only: the first call sizes them
        to its own T (a chunked prefill's first chunk: the later ones are no longer), a call with more rows allocates anew,
        one with fewer gets the head of what is there."""
        c, dev, f16, i8 = self.cfg, self.device, torch.float16, torch.int8
        buf = self._prefill_bufs
        if buf is None or buf["T"] < T:
            width = dict(x=(c.hidden, f16), qh=(c.hidden, i8), qi=(self.il, i8), qa=(self.hl * c.head_dim, i8),
                         qkv=((self.hl + 2 * self.kl) * c.head_dim, f16), proj=(c.hidden, f16), gu=(2 * self.il, f16))
            buf = dict(T=T)
            buf.update((name, torch.empty((T, w), dtype=dt, device=dev)) for name, (w, dt) in width.items())
            buf.update((name, torch.empty((T,), dtype=f16, device=dev)) for name in ("s1", "m1", "s2", "m2"))
            self._prefill_bufs = buf
        return [buf[name][:T] for name in ("x", "qh", "qi", "qa", "qkv", "proj", "gu", "s1", "m1", "s2", "m2")]

    def _context_layers(self, n, tokens, write, attention):
        """The ONE copy of the context stage's decoder layers (the sequence prefill() documents) on B * n rows, n per sequence, sequence
        after sequence.  Its callers differ in two calls: write(qkv, lens, pad, table) -- RoPE on q / k in place + the rows' KV4 page
        write (lens int32 [B] = n, pad: the padding offsets, table: the layer's block table) -- and attention(q, k, v, cu, table)
        -> fp16 [B * n, heads, head_dim] (q / k / v: views of qkv, cu int32 [B + 1]).  Returns the rows' final hidden states [B * n,
        hidden], a view of a buffer the next call reuses.  self.lengths is left alone."""
        c, B, dev = self.cfg, self.B, self.device
        T = B * n
        hq, hk, d = self.hl, self.kl, c.head_dim
        x, qh, qi, qa, qkv, proj, gu, sB, mB, sA, mA = self._context_bufs(T)
        torch.index_select(self.embed, 0, tokens.reshape(-1), out=x)
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * n
        pad = fused_attention_fine_grained_dense.compute_padding_offsets(cu, n, T)
        q = qkv[:, : hq * d].view(T, hq, d)
        k = qkv[:, hq * d:(hq + hk) * d].view(T, hk, d)
        v = qkv[:, (hq + hk) * d:].view(T, hk, d)
        per_chn = c.group_size == -1
        if not per_chn:
            mA = mB = None      # g128: no activation sums (see _eager_step_body)
        for li, Ly in enumerate(self.layers):
            if li == 0 and per_chn:
                layernorm_ops.rms_norm_general_fuse_sum(qh, x, Ly["ln1"], mB, sB, c.eps, True)
            elif li == 0:
                layernorm_ops.rms_norm_general(qh, x, Ly["ln1"], sB, c.eps, True)
            else:
                fused_ext.add_rms_norm_general_fuse_sum(qh, x, proj, Ly["ln1"], mB, sB, c.eps)
            Ly["qkv"].forward(qh, sB, mB, qkv)
            write(qkv, lens, pad, self.block_tables[li])
            attn = attention(q, k, v, cu, self.block_tables[li])
            if per_chn:
                fused_kernels.invoke_quant_fuse_sum(qa, attn.view(T, hq * d), mA, sA)
            else:
                fused_kernels.invoke_quant(qa, attn.view(T, hq * d), sA)
            Ly["o"].forward(qa, sA, mA, proj)
            self._all_reduce(proj)
            fused_ext.add_rms_norm_general_fuse_sum(qh, x, proj, Ly["ln2"], mB, sB, c.eps)
            Ly["gate_up"].forward(qh, sB, mB, gu)
            fused_ext.silu_mul_quant_fuse_sum(qi, gu, mA, sA)
            Ly["down"].forward(qi, sA, mA, proj)
            self._all_reduce(proj)
        x.add_(proj)
        return x

    def _token_ids(self, tokens, count, expects):
        """The caller's `count` token ids, or as many random ones.  expects: the error's head, e.g. "extend expects %d tokens"."""
        if tokens is None:
            return torch.randint(0, self.cfg.vocab, (count,), device=self.device, generator=self.gen)
        if tokens.numel() != count:
            raise ValueError("%s, got %d" % (expects % count, tokens.numel()))
        return tokens

    def _prompt(self, prompt_len, tokens):
        """prefill()'s arguments checked: -> (the prompt length, the B * length token ids)."""
        L = int(prompt_len if prompt_len is not None else self.lengths[0].item())
        if L < 1 or L + 1 > self.max_context:
            raise ValueError("prompt length does not fit the runner's KV pools")
        return L, self._token_ids(tokens, self.B * L, "prefill expects %d prompt tokens")

    def _next_from_last(self, x, n):
        """The context stage's tail: the last of each sequence's n rows of x -> self.x, final norm -> self.normed, lm_head, and the
        next token (arg-max, or a fresh draw on a sampling runner) -> self.tokens."""
        c = self.cfg
        if self._score_rows is not None:
            self._score_rows(x, n)
        self.x.copy_(x.view(self.B, n, c.hidden)[:, n - 1])
        layernorm_ops.rms_norm(self.normed, self.x, self.final_norm, c.eps, False)
        self._refill_u()
        logits = torch.matmul(self.normed, self.lm_head.t())
        self._pick(logits, fused_argmax=False)
        self._record_logprobs(logits)

    def prefill(self, prompt_len=None, tokens=None, chunk=None):
        """One context-stage pass over `prompt_len` tokens per sequence in the order of the reference's decoder
        layer at prefill shape (llama_w4a8_unpad.py:406-438 with M = B * prompt_len; ctx_update_kv.py:96-135;
        ctx_attn_func.py:68-73): norm+quant -> qkv GEMM -> RoPE in place + KV4 page write -> varlen causal
        attention -> quant -> o GEMM -> add -> norm+quant -> gate_up GEMM -> silu*mul -> quant -> down GEMM -> add.
        Fills the KV pools for positions [0, prompt_len) and leaves the first generated token in self.tokens
        (self.lengths = prompt_len), i.e. the qserve_benchmark.py protocol's prefill step.  Eager launches.
        `tokens`: the B * prompt_len prompt token ids, sequence after sequence (default: random ids).
        `chunk`: chunked prefill -- the prompt goes through in ceil(prompt_len / chunk) extend() calls of at most `chunk` tokens
        per sequence, with activation buffers of B * chunk rows instead of B * prompt_len.  Later chunks see the earlier ones
        through the KV4 pages, as every decode step does, so the result is close to but not bit-identical with the
        whole-prompt pass; chunk >= prompt_len is the whole-prompt pass."""
        if chunk is not None:
            return self._prefill_chunked(prompt_len, tokens, int(chunk))
        from .backend.prefill_attn import flash_attn_varlen_func
        c, dev = self.cfg, self.device
        hq, hk, d = self.hl, self.kl, c.head_dim
        L, tokens = self._prompt(prompt_len, tokens)
        flags = torch.ones((hk,), dtype=torch.int32, device=dev)
        rank = torch.arange(hk, dtype=torch.int32, device=dev)

        def write(qkv, lens, pad, table):      # the reference's writer with every head dense (ctx_update_kv.py:96-135)
            fused_attention_fine_grained_dense.apply_bias_rope_update_kv_cache(
                qkv, lens, None, pad, table, None, flags, rank, hq, hk, L, self.tpb, hk * d // 2, 0, 0, 0, 0, 0, hk, 0, d,
                c.rope_theta, 1.0, 1 << 20, True, True, True)

        def attention(q, k, v, cu, table):
            return flash_attn_varlen_func(q, k, v, cu, cu, L, L, causal=True)

        self._next_from_last(self._context_layers(L, tokens, write, attention), L)
        self.lengths.fill_(L)

    def _prefill_chunked(self, prompt_len, tokens, chunk):
        if chunk < 1:
            raise ValueError("chunk must be at least one token")
        L, tokens = self._prompt(prompt_len, tokens)
        tokens = tokens.view(self.B, L)
        self.lengths.zero_()
        for s in range(0, L, chunk):
            self.extend(min(chunk, L - s), tokens[:, s:s + chunk].reshape(-1))

    def score(self, tokens, chunk=None, top=0, block_rows=1024):
        """prefill(L, tokens, chunk=chunk) of tokens int64 [B, L], L >= 2 -- the same calls and the same state afterwards, byte for
        byte -- that also scores the prompt: logprob f32 / rank int32 [B, L - 1] and, with top in 1 .. 20, top_tokens int64 /
        top_logprobs f32 [B, L - 1, top] (else None), where entry [b, j] describes tokens[b, j + 1] given tokens[b, : j + 1] under
        the model's RAW distribution (what the reference's prompt_logprobs asks for; perplexity() turns logprob into the accuracy
        figure).  The context stage's rows go through final norm and lm_head in blocks of at most block_rows rows into ONE
        reusable logits buffer [block_rows, vocab] (never [B * L, vocab]), one fused_ext.logprobs call per block; in chunked mode
        chunk by chunk as extend() produces the rows, the target of a chunk's last row being the next chunk's first token.  The
        result does not depend on block_rows.  Works whatever the runner's `logprobs` and `sampling` are.  -> ScoreResult."""
        c, B, dev = self.cfg, self.B, self.device
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.shape[0] != B or tokens.dtype != torch.int64:
            raise ValueError("score expects int64 [B, L] tokens")
        L = int(tokens.shape[1])
        if L < 2:
            raise ValueError("score needs at least two tokens per sequence, got %d" % L)
        if L + 1 > self.max_context:
            raise ValueError("prompt length does not fit the runner's KV pools")
        top, block_rows = int(top), int(block_rows)
        if not 0 <= top <= fused_ext.LOGPROB_MAX_TOP:
            raise ValueError("score takes top in 0 .. %d, got %d" % (fused_ext.LOGPROB_MAX_TOP, top))
        if block_rows < 1:
            raise ValueError("block_rows must be at least one row")
        tokens = tokens.to(dev).contiguous()
        logprob = torch.empty((B, L - 1), dtype=torch.float32, device=dev)
        rank = torch.empty((B, L - 1), dtype=torch.int32, device=dev)
        top_tokens = torch.empty((B, L - 1, top), dtype=torch.int64, device=dev) if top else None
        top_logprobs = torch.empty((B, L - 1, top), dtype=torch.float32, device=dev) if top else None
        bufs = {}      # sized by the first block, the largest
        done = [0]     # positions per sequence that the context stage has been through

        def rows(x, n):
            s = done[0]
            done[0] = s + n
            k = min(n, L - 1 - s)      # the prompt's last row has no token behind it
            if k < 1:
                return
            h = x.view(B, n, c.hidden)[:, :k].reshape(B * k, c.hidden)
            tgt = tokens[:, s + 1:s + 1 + k].reshape(-1)
            lp = torch.empty((B * k,), dtype=torch.float32, device=dev)
            rk = torch.empty((B * k,), dtype=torch.int32, device=dev)
            tt = torch.empty((B * k, top), dtype=torch.int64, device=dev) if top else None
            tl = torch.empty((B * k, top), dtype=torch.float32, device=dev) if top else None
            if not bufs:
                m = min(block_rows, B * k)
                bufs["normed"] = torch.empty((m, c.hidden), dtype=torch.float16, device=dev)
                bufs["logits"] = torch.empty((m, c.vocab), dtype=torch.float16, device=dev)
            for r0 in range(0, B * k, block_rows):
                r1 = min(B * k, r0 + block_rows)
                normed, logits = bufs["normed"][: r1 - r0], bufs["logits"][: r1 - r0]
                layernorm_ops.rms_norm(normed, h[r0:r1], self.final_norm, c.eps, False)
                torch.matmul(normed, self.lm_head.t(), out=logits)
                fused_ext.logprobs(logits, target=tgt[r0:r1].contiguous(), n_top=top, token_logprob=lp[r0:r1], rank=rk[r0:r1],
                                   top_tokens=tt[r0:r1] if top else None, top_logprobs=tl[r0:r1] if top else None)
            logprob[:, s:s + k] = lp.view(B, k)
            rank[:, s:s + k] = rk.view(B, k)
            if top:
                top_tokens[:, s:s + k] = tt.view(B, k, top)
                top_logprobs[:, s:s + k] = tl.view(B, k, top)

        self._score_rows = rows
        try:
            self.prefill(L, tokens.reshape(-1), chunk=chunk)
        finally:
            self._score_rows = None
        return ScoreResult(logprob, rank, top_tokens, top_logprobs)

    def extend(self, new_len, tokens=None):
        """Append `new_len` tokens per sequence behind the self.lengths tokens (which may differ per sequence) already in the
        KV pools: chunked prefill, a further turn of a conversation, the suffix behind a shared prefix.  The layer sequence of
        prefill() with the writer at an offset (fused_ext.kv4_prefill_write_at) and the attention that continues from the pages
        (fused_ext.prefill_attention_paged_kv4: quantised past, fresh chunk) in place of its writer / attention pair.  Updates
        self.lengths and leaves the next token in self.tokens.  `tokens`: B * new_len ids, sequence after sequence (default:
        random ids).  With nothing in the pools yet (every length 0) this is prefill(new_len, tokens) itself."""
        n = int(new_len)
        past_max = int(self.lengths.max().item())
        if n < 1:
            raise ValueError("extend needs at least one new token per sequence")
        if past_max + n + 1 > self.max_context:
            raise ValueError("lengths + new_len does not fit the runner's KV pools")
        if past_max == 0:
            return self.prefill(n, tokens)
        tokens = self._token_ids(tokens, self.B * n, "extend expects %d tokens")
        self._next_from_last(self._extend_rows(n, tokens, past_max, fused_ext.prefill_attention_paged_kv4), n)
        self.lengths.add_(n)

    def _extend_rows(self, n, tokens, past_max, attention, rope_offsets=None):
        """The decoder layers on B * n rows that continue the sequences in the KV pools (extend(), verify()): writes the rows'
        keys / values at positions lengths + i and returns the rows' final hidden states [B * n, hidden] (a view of a buffer
        the next call reuses).  `attention(q, k, v, cu, past, table, tpb, n)`: the attention over quantised past + fresh rows.
        rope_offsets (verify_tree(): int32 [B * n], the nodes' depths): the rows still go to the slots lengths + i but are rotated
        at lengths + rope_offsets (fused_ext.kv4_prefill_write_at_pos); None: the plain writer at an offset.
        self.lengths is left alone."""
        c, hq, hk = self.cfg, self.hl, self.kl
        past = self.lengths.clone()

        def write(qkv, lens, pad, table):
            if rope_offsets is None:
                fused_ext.kv4_prefill_write_at(qkv, lens, past, pad, table, hq, hk, n, self.tpb, past_max + n, c.rope_theta, 1.0,
                                               1 << 20)
            else:
                fused_ext.kv4_prefill_write_at_pos(qkv, lens, past, rope_offsets, pad, table, hq, hk, n, self.tpb, past_max + n,
                                                   c.rope_theta, 1.0, 1 << 20)

        return self._context_layers(n, tokens, write, lambda q, k, v, cu, table: attention(q, k, v, cu, past, table, self.tpb, n))

    def _pending_rows(self, what, rows, limit, expects, unit, size):
        """The entry checks of verify() / verify_tree() on their int64 [B, n] token rows, whose column 0 must be the pending
        tokens and which must fit the pools behind the longest sequence.  what: the calling method; expects / unit / size: its
        words for the rows (the last word of expects names them), one of them and their count.  -> (rows on the device, n,
        the longest sequence's length)."""
        if rows.dim() != 2 or rows.shape[0] != self.B or rows.dtype != torch.int64:
            raise ValueError("%s expects %s" % (what, expects))
        n = int(rows.shape[1])
        if n < 1 or n > limit:
            raise ValueError("%s takes 1 to %d %s per sequence, got %d" % (what, limit, unit, n))
        rows = rows.to(self.device)
        if not bool((rows[:, 0] == self.tokens).all().item()):
            raise ValueError("%s: column 0 of the %s must be the runner's pending tokens" % (what, expects.split()[-1]))
        past_max = int(self.lengths.max().item())
        if past_max + n + 1 > self.max_context:
            raise ValueError("lengths + %s does not fit the runner's KV pools" % size)
        return rows, n, past_max

    def _keep(self, x, normed, pred, last, counts, lp=None):
        """The tail of verify() / verify_tree(): position last[b] (int64 [B, 1]) of sequence b's n scored ones is the one kept --
        its hidden state -> self.x, its normed state -> self.normed, the model's token behind it -> self.tokens -- and the
        sequence grows by counts[b] (int32 [B]).  lp (_logprobs_of's result, or None): its row of each -> the runner's buffers."""
        B, n = pred.shape
        if lp is not None:
            self.token_logprob.copy_(lp.token_logprob.view(B, n).gather(1, last).squeeze(1))
            self.token_rank.copy_(lp.rank.view(B, n).gather(1, last).squeeze(1))
            if self.logprobs > 0:
                pick_top = last.view(B, 1, 1).expand(B, 1, self.logprobs)
                self.top_tokens.copy_(lp.top_tokens.view(B, n, -1).gather(1, pick_top).squeeze(1))
                self.top_logprobs.copy_(lp.top_logprobs.view(B, n, -1).gather(1, pick_top).squeeze(1))
        pick = last.view(B, 1, 1).expand(B, 1, self.cfg.hidden)
        self.x.copy_(x.view(B, n, -1).gather(1, pick).squeeze(1))
        self.normed.copy_(normed.view(B, n, -1).gather(1, pick).squeeze(1))
        self.tokens.copy_(pred.gather(1, last).squeeze(1))
        self.lengths.add_(counts)

    def verify(self, draft, sampled=None, uniforms=None):
        """One multi-token decode step (the verify step of speculative decoding): score n = draft.shape[1] <= 8 positions per
        sequence in one pass over the weights.  draft int64 [B, n]: column 0 is self.tokens (the pending token, not yet in the
        pools), columns 1 .. the drafted continuation.  extend()'s layer sequence on B * n rows with the split-KV multi-token
        attention (fused_ext.decode_attention_multi_kv4) in place of the paged prefill attention, then final norm, lm_head and
        arg-max at ALL n positions: pred int64 [B, n], pred[b, j] = the model's token behind draft[b, :j + 1].  m =
        accept_lengths(draft, pred) tokens per sequence are kept: lengths += m, tokens = pred[b, m - 1], self.x / self.normed =
        the hidden state of the last accepted position (as extend() leaves them).  Rollback: the rejected tokens' page slots
        keep their bytes; they lie at positions >= lengths, which no kernel reads and later appends overwrite.  Eager launches
        (capturing the step in a HIP graph is the follow-up).  -> (pred, m).
        sampled (default: the runner's `sampling`): the rejection rule of speculative sampling in place of "the draft equals the
        arg-max".  ONE fused_ext.sample call over all B * n logits rows with probe = exclude = draft[b, j + 1] (-1 in the last
        column) gives the drafted token's probability under the filtered distribution and a draw without it; m, tokens =
        accept_sampled(probe_prob, u_acc, drawn); the state is left as above.  uniforms = (u_draw, u_acc), f32 [B, n] each:
        the draws to use instead of fresh ones from the runner's generator (replay, tests).  -> (drawn, m)."""
        c, B = self.cfg, self.B
        sampled = self.sampling if sampled is None else bool(sampled)
        if sampled and not self.sampling:
            raise RuntimeError("verify(sampled=True) needs a runner built with sampling=True")
        draft, n, past_max = self._pending_rows("verify", draft, fused_ext.DECODE_MULTI_MAX_Q, "an int64 [B, n] draft",
                                                "positions", "draft length")

        def attention(q, k, v, cu, past, table, tpb, n_):
            return fused_ext.decode_attention_multi_kv4(q, k, v, cu, past, table, tpb, n_, past_max)

        x = self._extend_rows(n, draft.reshape(-1), past_max, attention)
        normed = torch.empty_like(x)
        layernorm_ops.rms_norm(normed, x, self.final_norm, c.eps, False)
        logits = torch.matmul(normed, self.lm_head.t())
        if sampled:
            u_draw, u_acc = uniforms if uniforms is not None else self._uniforms(2, B, n)
            guess = torch.cat([draft[:, 1:], torch.full((B, 1), -1, dtype=torch.int64, device=self.device)], dim=1).reshape(-1)
            pred = torch.empty((B * n,), dtype=torch.int64, device=self.device)
            prob = torch.empty((B * n,), dtype=torch.float32, device=self.device)
            fused_ext.sample(pred, logits, self.s_temperature.repeat_interleave(n), self.s_top_k.repeat_interleave(n),
                             self.s_top_p.repeat_interleave(n), u_draw.to(self.device).reshape(-1).contiguous(),
                             probe=guess, exclude=guess, probe_prob=prob)
            pred = pred.view(B, n)
            m, _ = accept_sampled(prob.view(B, n), u_acc.to(self.device).view(B, n), pred)
        else:
            pred = torch.argmax(logits, dim=-1).view(B, n)
            m = accept_lengths(draft, pred)
        self._keep(x, normed, pred, (m - 1).view(B, 1), m.to(torch.int32), self._logprobs_of(logits, pred))
        return pred, m

    def verify_tree(self, tokens, parents):
        """verify() over a token TREE (Medusa / EAGLE heads, top-k branching, n-gram alternatives): score n = tokens.shape[1] <=
        32 nodes per sequence in one pass over the weights.  tokens int64 [B, n]: column 0 is self.tokens (the pending token),
        column i the token of node i; parents: n ints, ONE topology for the batch, parents[0] = -1 and 0 <= parents[i] < i
        (checked here, on the host).  Node i is written to slot lengths + i but rotated at position lengths + depth(i)
        (fused_ext.kv4_prefill_write_at_pos) and attends to the past and to its ancestors only
        (fused_ext.decode_attention_tree_kv4 with fused_ext.tree_masks); then final norm, lm_head and arg-max at ALL n nodes:
        pred[b, i] = the model's token behind node i's path.  (path, m) = accept_paths(parents, tokens, pred); every layer's K / V
        rows of the path move from the slots lengths + path[b, j] to lengths + j (fused_ext.kv4_compact_rows), then lengths += m,
        tokens = pred[b, path[b, m - 1]] and self.x / self.normed = that node's hidden state.  The rejected nodes' slots lie at
        positions >= lengths, as after verify().  Eager launches.  -> (pred, path, m)."""
        c, B = self.cfg, self.B
        if self.sampling:
            raise NotImplementedError("verify_tree on a sampling runner: multi-branch rejection sampling is not built; the tree "
                                      "step is greedy only (use verify() for sampled speculative decoding)")
        tokens, n, past_max = self._pending_rows("verify_tree", tokens, fused_ext.DECODE_TREE_MAX_Q, "int64 [B, n] tokens",
                                                 "nodes", "tree size")
        par = [int(p) for p in (parents.tolist() if torch.is_tensor(parents) else parents)]
        if len(par) != n or par[0] != -1 or any(not 0 <= par[i] < i for i in range(1, n)):
            raise ValueError("verify_tree: parents must hold n entries with parents[0] = -1 and 0 <= parents[i] < i")
        mask1, depth1 = fused_ext.tree_masks(torch.tensor(par, dtype=torch.int64))
        mask = mask1.repeat(B).to(self.device)
        depth = depth1.repeat(B).to(self.device)

        def attention(q, k, v, cu, past, table, tpb, n_):
            return fused_ext.decode_attention_tree_kv4(q, k, v, cu, past, mask, table, tpb, n_, past_max)

        x = self._extend_rows(n, tokens.reshape(-1), past_max, attention, rope_offsets=depth)
        normed = torch.empty_like(x)
        layernorm_ops.rms_norm(normed, x, self.final_norm, c.eps, False)
        logits = torch.matmul(normed, self.lm_head.t())
        pred = torch.argmax(logits, dim=-1).view(B, n)
        path, m = accept_paths(par, tokens, pred)
        src, counts = path.to(torch.int32).contiguous(), m.to(torch.int32)
        for table in self.block_tables:
            fused_ext.kv4_compact_rows(table, self.lengths, src, counts, self.tpb, self.kl)
        self._keep(x, normed, pred, path.gather(1, (m - 1).view(B, 1)), counts, self._logprobs_of(logits, pred))
        return pred, path, m

    def _all_reduce(self, buf):
        if self.tp_size > 1:
            from . import tp
            tp.all_reduce_(buf, self.tp_group)

    # ---- accounting -----------------------------------------------------------
    def gemm_weight_bytes_per_step(self):
        return sum(L[n].weight_bytes() for L in self.layers for n in ("qkv", "o", "gate_up", "down"))

    def kv_bytes_per_step(self, context):
        c = self.cfg
        per_tok = 2 * (self.kl * c.head_dim // 2 + self.kl * 4)
        return per_tok * context * self.B * c.layers
