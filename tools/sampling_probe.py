"""Sampled decoding: fused_ext.sample against the reference sampler's pipeline restated in torch on the device, and
fused_ext.argmax on the same logits.

    python -m tools.sampling_probe [--out FILE] [--step]

Side A: fused_ext.sample (temperature 0.8, top_k 50, top_p 0.9).  Side B: scale, sort, cumulative softmax, top-p mask, top-k
mask, softmax, multinomial -- what omniserve/modeling/layers/sampler.py's warpers and draw run.  Shapes [16, 128256],
[128, 128256] and [64, 128256] (16 sequences x 4 verify positions).  Per side and shape: 7 repeats of 10 launches between
device events, the sides alternating; median over the repeats, spread = max - min over the repeats.  --step also times
DecodeRunner.step() at Llama-3-8B, batch 16, 1024 cached tokens, greedy against sampling=True, the same way.
Needs a GPU: no fallback."""
import argparse
import json
import statistics
import sys

import torch

REPEATS, LAUNCHES = 7, 10
SHAPES = ((16, 128256), (128, 128256), (64, 128256))


def torch_pipeline(logits, temperature, top_k, top_p):
    s = logits.float() / temperature
    srt, idx = torch.sort(s, dim=-1, descending=False)
    cum = srt.softmax(dim=-1).cumsum(dim=-1)
    remove = cum <= (1.0 - top_p)
    remove[..., -1:] = False
    s = s.masked_fill(remove.scatter(1, idx, remove), float("-inf"))
    kth = torch.topk(s, top_k, dim=-1)[0][..., -1, None]
    s = s.masked_fill(s < kth, float("-inf"))
    return torch.multinomial(torch.softmax(s, dim=-1), num_samples=1).view(-1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / LAUNCHES      # us per launch


def alternate(sides):
    """sides: {name: fn}.  -> {name: (median us, spread us)}"""
    for fn in sides.values():      # warm-up: code objects, workspaces, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in sides}
    for _ in range(REPEATS):
        for name, fn in sides.items():
            runs[name].append(timed(fn))
    return {name: (statistics.median(v), max(v) - min(v)) for name, v in runs.items()}


def probe_kernels(dev):
    from omniserve_amd.backend import fused_ext
    rows_out = []
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for rows, cols in SHAPES:
        logits = (torch.randn((rows, cols), device=dev, generator=g) * 2.5).half()
        out = torch.empty((rows,), dtype=torch.int64, device=dev)
        t = torch.full((rows,), 0.8, dtype=torch.float32, device=dev)
        k = torch.full((rows,), 50, dtype=torch.int32, device=dev)
        p = torch.full((rows,), 0.9, dtype=torch.float32, device=dev)
        u = torch.rand((rows,), device=dev, generator=g)
        res = alternate({"sample": lambda: fused_ext.sample(out, logits, t, k, p, u),
                         "torch": lambda: torch_pipeline(logits, 0.8, 50, 0.9),
                         "argmax": lambda: fused_ext.argmax(out, logits)})
        rows_out.append(dict(shape=[rows, cols], **{n: dict(median_us=round(m, 2), spread_us=round(s, 2))
                                                   for n, (m, s) in res.items()}))
        rows_out[-1]["faster_by_more_than_the_spread"] = \
            res["torch"][0] - res["sample"][0] > max(res["torch"][1], res["sample"][1])
    return rows_out


def probe_step(dev):
    from omniserve_amd.runtime import DecodeRunner, LlamaConfig
    cfg = LlamaConfig.llama3_8b()
    greedy = DecodeRunner(cfg, 16, 1024, 200, dev, seed=1)
    sampled = DecodeRunner(cfg, 16, 1024, 200, dev, seed=1, sampling=True)
    sampled.set_sampling(temperature=0.8, top_k=50, top_p=0.9, seed=1)
    res = alternate({"greedy": greedy.step, "sampled": sampled.step})
    return {n: dict(median_ms=round(m / 1000.0, 4), spread_ms=round(s / 1000.0, 4)) for n, (m, s) in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampling_probe needs a GPU")
    dev = torch.device("cuda:0")
    result = dict(kernels=probe_kernels(dev))
    if args.step:
        result["step_llama3_8b_bs16_ctx1024"] = probe_step(dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
