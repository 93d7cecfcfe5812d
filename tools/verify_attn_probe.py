"""What does the multi-token decode attention buy over the kernels on either side of it?

1. Kernel: omni_decode_attention_multi_kv4 against omni_prefill_attention_paged_kv4 (the same mathematics, one workgroup per q
   head and no KV split) in the same process, B = 16 sequences, 32 q heads over 8 kv heads, tokens_per_block 64, n = 4 new tokens,
   past 1024 / 4096 / 16384; and against n launches of the one-query decode kernel (single_query_attention, contexts past + 1 ...
   past + n) as a second reference.
2. Runner: DecodeRunner.verify(n = 4) against one eager step(), Llama-3-8B-shaped layers (4 of them), batch 16, context 4096.

Timed with HIP events around REPLAYS back-to-back launches; the sides alternate, REPEATS times each, and the run-to-run spread
(max - min over the repeats, the largest over the sides of a shape) is printed next to the medians.  "faster" in the result means:
the medians differ by more than that spread.

    python tools/verify_attn_probe.py [--out FILE.json] [--skip-runner]

The measurement runs in a child process under its own time limit; the parent only starts it and relays its JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HQ, HK, D, TPB, N, REPEATS, REPLAYS = 16, 32, 8, 128, 64, 4, 7, 10
PASTS = [1024, 4096, 16384]
RUN_CONTEXT, RUN_LAYERS = 4096, 4


def measure(skip_runner):
    import statistics
    import torch
    sys.path.insert(0, ROOT)
    from omniserve_amd.backend import fused_attention_pure_dense, fused_ext
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

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

    def summary(ms):
        out = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
               for name, v in ms.items()}
        out["spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
        return out

    res = {"what": "attention for %d new tokens per sequence over KV4 pages, B = %d, %d / %d heads, tokens_per_block %d: multi "
                   "(omni_decode_attention_multi_kv4) vs paged (omni_prefill_attention_paged_kv4) vs %d launches of the decode "
                   "kernel; ms per call, %d repeats x %d launches, alternating" % (N, B, HQ, HK, TPB, N, REPEATS, REPLAYS),
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    data = HK * TPB * D // 2
    page_bytes = data + 2 * HK * TPB * 2
    for past_len in PASTS:
        pps = (past_len + N) // TPB + 1
        tab = torch.empty((B, 2, pps), dtype=torch.int64, device=dev)
        keep = []
        for kv in range(2):
            pool = torch.empty((B * pps, page_bytes), dtype=torch.uint8, device=dev)
            pool[:, :data] = torch.randint(0, 256, (B * pps, data), dtype=torch.uint8, device=dev, generator=gen)
            tail = pool[:, data:].view(torch.float16).view(B * pps, 2, HK * TPB)
            tail[:, 0] = 0.25 * (0.5 + torch.rand((B * pps, HK * TPB), device=dev, generator=gen))
            tail[:, 1] = 7.5
            tab[:, kv] = pool.data_ptr() + torch.randperm(B * pps, device=dev, generator=gen).view(B, pps) * page_bytes
            keep.append(pool)
        q = (0.5 * torch.randn((B * N, HQ, D), device=dev, generator=gen)).half()
        k_new = torch.randn((B * N, HK, D), device=dev, generator=gen).half()
        v_new = torch.randn((B * N, HK, D), device=dev, generator=gen).half()
        cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * N
        past = torch.full((B,), past_len, dtype=torch.int32, device=dev)
        ws = torch.empty(fused_ext.decode_attention_multi_kv4_workspace_bytes(B, HQ, N, past_len), dtype=torch.uint8, device=dev)
        q1, k1, v1 = q[:B], k_new[:B], v_new[:B]
        lens = [torch.full((B,), past_len + i + 1, dtype=torch.int32, device=dev) for i in range(N)]

        def multi():
            return fused_ext.decode_attention_multi_kv4(q, k_new, v_new, cu, past, tab, TPB, N, past_len, workspace=ws)

        def paged():
            return fused_ext.prefill_attention_paged_kv4(q, k_new, v_new, cu, past, tab, TPB, N)

        def decode_n():      # (appends its token to the pages, at positions >= past: the other two never read those)
            for i in range(N):
                fused_attention_pure_dense.single_query_attention(q1, k1, v1, tab, lens[i], None, 65536, TPB, HK * D // 2,
                                                                  past_len + N, D, 500000.0, True, True, True)

        err = float((multi().float() - paged().float()).abs().max())
        ms = {"multi": [], "paged": [], "decode_x%d" % N: []}
        for _ in range(REPEATS):
            ms["multi"].append(time_ms(multi, REPLAYS))
            ms["paged"].append(time_ms(paged, REPLAYS))
            ms["decode_x%d" % N].append(time_ms(decode_n, REPLAYS))
        s = summary(ms)
        s["max_abs_diff_multi_vs_paged"] = round(err, 5)
        s["paged_over_multi"] = round(s["paged"]["median_ms"] / s["multi"]["median_ms"], 2)
        s["decode_over_multi"] = round(s["decode_x%d" % N]["median_ms"] / s["multi"]["median_ms"], 2)
        s["multi_faster_than_paged_by_more_than_spread"] = bool(s["paged"]["median_ms"] - s["multi"]["median_ms"] > s["spread_ms"])
        res["shapes"]["past_%d" % past_len] = s
        del keep, tab, ws
    if not skip_runner:
        from omniserve_amd.runtime import DecodeRunner, LlamaConfig
        cfg = LlamaConfig.llama3_8b()
        cfg.layers = RUN_LAYERS
        r = DecodeRunner(cfg, B, RUN_CONTEXT, 64, dev, seed=1, use_graph=False, fused=2)
        state = (r.lengths.clone(), r.tokens.clone())

        def restore():
            r.lengths.copy_(state[0])
            r.tokens.copy_(state[1])

        def step():
            restore()
            r.step()

        def verify():
            restore()
            draft = torch.cat([r.tokens.view(B, 1), torch.zeros((B, N - 1), dtype=torch.int64, device=dev)], dim=1)
            r.verify(draft)

        run = {"verify_%d" % N: [], "step": []}
        for _ in range(REPEATS):
            run["verify_%d" % N].append(time_ms(verify, 3))
            run["step"].append(time_ms(step, 3))
        s = summary(run)
        s["what"] = "DecodeRunner.verify(n = %d) vs one eager step(), Llama-3-8B layers x %d, batch %d, context %d, ms" % (
            N, RUN_LAYERS, B, RUN_CONTEXT)
        s["verify_over_step"] = round(s["verify_%d" % N]["median_ms"] / s["step"]["median_ms"], 2)
        res["runner"] = s
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
