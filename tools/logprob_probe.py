"""Log-probabilities: fused_ext.logprobs against torch on the same rows, the cost on the decode step, and score()'s peak
memory against the torch route.

    python -m tools.logprob_probe [--out FILE] [--step] [--score]

Side A: fused_ext.logprobs(logits, target, n_top) for n_top 0, 5 and 20.  Side B: torch.log_softmax(logits.float()), gather of
the target and, with n_top > 0, torch.topk.  Shapes [16, 128256], [128, 128256] and [1024, 32000].  Per side and shape: 7 repeats
of 10 launches between device events, the sides alternating; median over the repeats, spread = max - min over the repeats.
--step also times DecodeRunner.step() at Llama-3-8B, batch 16, 1024 cached tokens, captured, with logprobs None, 0 and 5, the
same way.  --score: score() of 4096 tokens x batch 1 at Llama-3-8B with 4 layers, torch.cuda.max_memory_allocated above what is
allocated before the call, against the torch route over the same hidden states (the whole [T, vocab] logits and their f32
log-softmax).  Needs a GPU: no fallback."""
import argparse
import json
import sys

import torch

from tools.sampling_probe import alternate

SHAPES = ((16, 128256), (128, 128256), (1024, 32000))
N_TOPS = (0, 5, 20)


def torch_route(logits, target, n_top):
    lp = torch.log_softmax(logits.float(), dim=-1)
    tok = lp.gather(1, target.view(-1, 1))
    return (tok, torch.topk(lp, n_top, dim=-1)) if n_top else tok


def probe_kernels(dev):
    from omniserve_amd.backend import fused_ext
    rows_out = []
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for rows, cols in SHAPES:
        logits = (torch.randn((rows, cols), device=dev, generator=g) * 2.5).half()
        target = torch.randint(0, cols, (rows,), device=dev, generator=g)
        for n_top in N_TOPS:
            out = fused_ext.logprobs(logits, target=target, n_top=n_top)      # the outputs, allocated once
            kw = dict(lse=out.lse, token_logprob=out.token_logprob, rank=out.rank, top_tokens=out.top_tokens,
                      top_logprobs=out.top_logprobs)
            res = alternate({"logprobs": lambda: fused_ext.logprobs(logits, target=target, n_top=n_top, **kw),
                             "torch": lambda: torch_route(logits, target, n_top)})
            rows_out.append(dict(shape=[rows, cols], n_top=n_top,
                                 **{n: dict(median_us=round(m, 2), spread_us=round(s, 2)) for n, (m, s) in res.items()}))
            rows_out[-1]["faster_by_more_than_the_spread"] = \
                res["torch"][0] - res["logprobs"][0] > max(res["torch"][1], res["logprobs"][1])
    return rows_out


def probe_step(dev):
    from omniserve_amd.runtime import DecodeRunner, LlamaConfig
    cfg = LlamaConfig.llama3_8b()
    runners = {"none": DecodeRunner(cfg, 16, 1024, 200, dev, seed=1)}
    for n in (0, 5):
        runners["logprobs_%d" % n] = DecodeRunner(cfg, 16, 1024, 200, dev, seed=1, logprobs=n)
    res = alternate({name: r.step for name, r in runners.items()})
    return {n: dict(median_ms=round(m / 1000.0, 4), spread_ms=round(s / 1000.0, 4)) for n, (m, s) in res.items()}


def probe_score(dev, T=4096, layers=4):
    import dataclasses
    from omniserve_amd.backend import layernorm_ops
    from omniserve_amd.runtime import DecodeRunner, LlamaConfig
    cfg = dataclasses.replace(LlamaConfig.llama3_8b(), layers=layers)
    r = DecodeRunner(cfg, 1, T, 8, dev, seed=1, use_graph=False)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    tokens = torch.randint(0, cfg.vocab, (1, T), device=dev, generator=g)
    r.score(tokens[:, :64])      # warm-up: code objects, workspaces
    r._prefill_bufs = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = r.score(tokens)
    torch.cuda.synchronize()
    peak_score = torch.cuda.max_memory_allocated() - base
    # the torch route over the same rows: the context stage's hidden states are still in the runner's buffer
    x = r._prefill_bufs["x"][:T]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    normed = torch.empty_like(x)
    layernorm_ops.rms_norm(normed, x, r.final_norm, cfg.eps, False)
    lp = torch.log_softmax(torch.matmul(normed, r.lm_head.t()).float(), dim=-1)
    ref = lp[:-1].gather(1, tokens[0, 1:].view(-1, 1)).view(-1)
    torch.cuda.synchronize()
    peak_torch = torch.cuda.max_memory_allocated() - base
    return dict(tokens=T, layers=layers, score_peak_mib=round(peak_score / 2 ** 20, 1), torch_peak_mib=round(peak_torch / 2 ** 20, 1),
                max_abs_difference=float((res.logprob.view(-1) - ref).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--score", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logprob_probe needs a GPU")
    dev = torch.device("cuda:0")
    result = dict(kernels=probe_kernels(dev))
    if args.step:
        result["step_llama3_8b_bs16_ctx1024"] = probe_step(dev)
    if args.score:
        result["score_llama3_8b"] = probe_score(dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
