"""What does it cost to take the past of a prefill from the KV4 pages?

1. Kernel: omni_prefill_attention_paged_kv4 at (past 16 K, len_q 2 K, 32 q heads over 8 kv heads, one sequence) against
   omni_prefill_attention at len_q = 2 K, len_k = 18 K on fp16 K / V -- the same flops; the first dequantises 16 K keys and values
   per (q tile, q head) workgroup on its way to LDS, the second streams them by LDS-DMA.
2. Runner: DecodeRunner.prefill(16 K, chunk=2 K) against prefill(16 K), Llama-3-8B-shaped layers (4 of them), batch 1.

Timed with HIP events around REPLAYS back-to-back launches; the two sides alternate, REPEATS times each, and the spread
(max - min over the repeats) is printed next to the medians.  Nothing is gated on these numbers.

    python tools/paged_prefill_probe.py [--out FILE.json] [--skip-runner]

The measurement runs in a child process under its own time limit; the parent only starts it and relays its JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAST, LQ, HQ, HK, D, TPB, REPEATS, REPLAYS = 16384, 2048, 32, 8, 128, 64, 5, 4
RUN_L, RUN_CHUNK, RUN_LAYERS = 16384, 2048, 4


def measure(skip_runner):
    import statistics
    import torch
    sys.path.insert(0, ROOT)
    from omniserve_amd.backend import fused_ext
    from omniserve_amd.backend.prefill_attn import flash_attn_varlen_func
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    pps = (PAST + LQ) // TPB
    data = HK * TPB * D // 2
    page_bytes = data + 2 * HK * TPB * 2
    tab = torch.empty((1, 2, pps), dtype=torch.int64, device=dev)
    keep = []
    for kv in range(2):
        pool = torch.empty((pps, page_bytes), dtype=torch.uint8, device=dev)
        pool[:, :data] = torch.randint(0, 256, (pps, data), dtype=torch.uint8, device=dev, generator=gen)
        tail = pool[:, data:].view(torch.float16).view(pps, 2, HK * TPB)
        tail[:, 0] = 0.25 * (0.5 + torch.rand((pps, HK * TPB), device=dev, generator=gen))
        tail[:, 1] = 7.5
        tab[:, kv] = pool.data_ptr() + torch.randperm(pps, device=dev, generator=gen).view(1, pps) * page_bytes
        keep.append(pool)
    q = (0.5 * torch.randn((LQ, HQ, D), device=dev, generator=gen)).half()
    k_new = torch.randn((LQ, HK, D), device=dev, generator=gen).half()
    v_new = torch.randn((LQ, HK, D), device=dev, generator=gen).half()
    k_all = torch.randn((PAST + LQ, HK, D), device=dev, generator=gen).half()
    v_all = torch.randn((PAST + LQ, HK, D), device=dev, generator=gen).half()
    cu_q = torch.tensor([0, LQ], dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0, PAST + LQ], dtype=torch.int32, device=dev)
    past = torch.tensor([PAST], dtype=torch.int32, device=dev)

    def paged():
        return fused_ext.prefill_attention_paged_kv4(q, k_new, v_new, cu_q, past, tab, TPB, LQ)

    def fresh():
        return flash_attn_varlen_func(q, k_all, v_all, cu_q, cu_k, LQ, PAST + LQ, causal=True)

    def time_ms(fn, n):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    ms = {"paged": [], "fresh": []}
    for _ in range(REPEATS):
        ms["paged"].append(time_ms(paged, REPLAYS))
        ms["fresh"].append(time_ms(fresh, REPLAYS))
    flops = 4.0 * LQ * HQ * D * (PAST + (LQ + 1) / 2.0)
    res = {"what": "prefill attention, past %d + len_q %d, %d / %d heads, one sequence: KV4 pages for the past (paged) vs fp16 K / V "
                   "(fresh), ms per launch; %d repeats x %d launches, alternating" % (PAST, LQ, HQ, HK, REPEATS, REPLAYS),
           "device": torch.cuda.get_device_name(0)}
    for name in ("paged", "fresh"):
        med = statistics.median(ms[name])
        res[name] = {"median_ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                     "tflops": round(flops / med / 1e9, 1)}
    res["spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
    res["paged_over_fresh"] = round(res["paged"]["median_ms"] / res["fresh"]["median_ms"], 3)
    if not skip_runner:
        from omniserve_amd.runtime import DecodeRunner, LlamaConfig
        cfg = LlamaConfig.llama3_8b()
        cfg.layers = RUN_LAYERS
        r = DecodeRunner(cfg, 1, RUN_L, 8, dev, seed=1, use_graph=False, fused=2)
        toks = torch.randint(0, cfg.vocab, (RUN_L,), device=dev, generator=gen)
        run = {"chunked": [], "whole": []}
        for _ in range(3):
            run["chunked"].append(time_ms(lambda: r.prefill(RUN_L, toks, chunk=RUN_CHUNK), 1))
            run["whole"].append(time_ms(lambda: r.prefill(RUN_L, toks), 1))
        res["runner"] = {"what": "DecodeRunner.prefill(%d, chunk=%d) vs prefill(%d), Llama-3-8B layers x %d, batch 1, ms" % (
                             RUN_L, RUN_CHUNK, RUN_L, RUN_LAYERS),
                         "chunked_ms": [round(x, 2) for x in run["chunked"]], "whole_ms": [round(x, 2) for x in run["whole"]],
                         "chunked_over_whole": round(statistics.median(run["chunked"]) / statistics.median(run["whole"]), 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true", help="(internal) run the measurement in this process")
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.measure:
        measure(a.skip_runner)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--measure"] + (["--skip-runner"] if a.skip_runner else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
