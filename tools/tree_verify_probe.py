"""What does the tree form of the multi-token decode attention cost, and what does a tree verify step cost?

1. Kernel, gated: omni_decode_attention_tree_kv4 with CHAIN masks against omni_decode_attention_multi_kv4 on the same inputs in the
   same process, B = 16 sequences, 32 q heads over 8 kv heads, tokens_per_block 64, n = 8 new tokens, past 1024 / 4096 / 16384.
   The tree form must not be slower than the chain entry by more than the measured spread (the mask costs one AND per element of
   the fresh tile, one tile of many).
2. Reported: star trees of n = 16 and 32 nodes at the same pasts; the compaction launch (omni_kv4_compact_rows) at B = 16, 8 kv
   heads, m = 4 (path 0, 2, 4, 5 of 7 nodes).
3. Runner: DecodeRunner.verify_tree(n = 16, binary tree) against one eager step(), Llama-3-8B-shaped layers (4 of them), batch 16,
   context 4096.

tools/verify_attn_probe.py's protocol: HIP events around REPLAYS back-to-back launches; the sides alternate, REPEATS times each;
the run-to-run spread (max - min over the repeats, the largest over the sides of a shape) is printed next to the medians.

    python tools/tree_verify_probe.py [--out FILE.json] [--skip-runner]

The measurement runs in a child process under its own time limit; the parent only starts it and relays its JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HQ, HK, D, TPB, N, REPEATS, REPLAYS = 16, 32, 8, 128, 64, 8, 7, 10
PASTS = [1024, 4096, 16384]
STARS = [16, 32]
RUN_CONTEXT, RUN_LAYERS, RUN_N = 4096, 4, 16


def measure(skip_runner):
    import statistics
    import torch
    sys.path.insert(0, ROOT)
    from omniserve_amd.backend import fused_ext
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

    res = {"what": "tree form (omni_decode_attention_tree_kv4, chain masks) vs chain entry (omni_decode_attention_multi_kv4), n = %d "
                   "new tokens per sequence over KV4 pages, B = %d, %d / %d heads, tokens_per_block %d; star trees of %s nodes; ms "
                   "per call, %d repeats x %d launches, alternating" % (N, B, HQ, HK, TPB, STARS, REPEATS, REPLAYS),
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    data = HK * TPB * D // 2
    page_bytes = data + 2 * HK * TPB * 2
    n_max = max(STARS)
    for past_len in PASTS:
        pps = (past_len + n_max) // TPB + 1
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
        past = torch.full((B,), past_len, dtype=torch.int32, device=dev)

        def inputs(n):
            q = (0.5 * torch.randn((B * n, HQ, D), device=dev, generator=gen)).half()
            k_new = torch.randn((B * n, HK, D), device=dev, generator=gen).half()
            v_new = torch.randn((B * n, HK, D), device=dev, generator=gen).half()
            cu = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * n
            return q, k_new, v_new, cu

        q, k_new, v_new, cu = inputs(N)
        chain_mask = fused_ext.tree_masks(torch.arange(-1, N - 1))[0].repeat(B).to(dev)
        ws = torch.empty(fused_ext.decode_attention_tree_kv4_workspace_bytes(B, HQ, n_max, past_len), dtype=torch.uint8, device=dev)

        def chain():
            return fused_ext.decode_attention_multi_kv4(q, k_new, v_new, cu, past, tab, TPB, N, past_len, workspace=ws)

        def tree():
            return fused_ext.decode_attention_tree_kv4(q, k_new, v_new, cu, past, chain_mask, tab, TPB, N, past_len, workspace=ws)

        same = bool(torch.equal(chain().view(torch.int16), tree().view(torch.int16)))
        ms = {"chain": [], "tree": []}
        for _ in range(REPEATS):
            ms["chain"].append(time_ms(chain, REPLAYS))
            ms["tree"].append(time_ms(tree, REPLAYS))
        s = summary(ms)
        s["same_bits"] = same
        s["tree_minus_chain_ms"] = round(s["tree"]["median_ms"] - s["chain"]["median_ms"], 4)
        s["tree_not_slower_than_chain_by_more_than_spread"] = bool(s["tree_minus_chain_ms"] <= s["spread_ms"])
        for n in STARS:
            qs, ks, vs, cus = inputs(n)
            par = torch.zeros(n, dtype=torch.int64)
            par[0] = -1
            star_mask = fused_ext.tree_masks(par)[0].repeat(B).to(dev)

            def star():
                return fused_ext.decode_attention_tree_kv4(qs, ks, vs, cus, past, star_mask, tab, TPB, n, past_len, workspace=ws)
            v = [time_ms(star, REPLAYS) for _ in range(REPEATS)]
            s["star_%d" % n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if past_len == PASTS[0]:
            base = torch.full((B,), past_len - 8, dtype=torch.int32, device=dev)
            src = torch.tensor([[0, 2, 4, 5, -1, -1, -1]] * B, dtype=torch.int32, device=dev)
            cnt = torch.full((B,), 4, dtype=torch.int32, device=dev)
            v = [time_ms(lambda: fused_ext.kv4_compact_rows(tab, base, src, cnt, TPB, HK), REPLAYS) for _ in range(REPEATS)]
            res["compact_rows"] = {"what": "omni_kv4_compact_rows, B = %d, %d kv heads, path 0 2 4 5 of 7 nodes (m = 4), ms per launch "
                                           "(back to back: the launch floor)" % (B, HK),
                                   "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        res["shapes"]["past_%d" % past_len] = s
        del keep, tab, ws
    if not skip_runner:
        from omniserve_amd.runtime import DecodeRunner, LlamaConfig
        cfg = LlamaConfig.llama3_8b()
        cfg.layers = RUN_LAYERS
        r = DecodeRunner(cfg, B, RUN_CONTEXT, 64, dev, seed=1, use_graph=False, fused=2)
        state = (r.lengths.clone(), r.tokens.clone())
        parents = [-1] + [(i - 1) // 2 for i in range(1, RUN_N)]

        def restore():
            r.lengths.copy_(state[0])
            r.tokens.copy_(state[1])

        def step():
            restore()
            r.step()

        def verify_tree():
            restore()
            nodes = torch.cat([r.tokens.view(B, 1), torch.zeros((B, RUN_N - 1), dtype=torch.int64, device=dev)], dim=1)
            r.verify_tree(nodes, parents)

        run = {"verify_tree_%d" % RUN_N: [], "step": []}
        for _ in range(REPEATS):
            run["verify_tree_%d" % RUN_N].append(time_ms(verify_tree, 3))
            run["step"].append(time_ms(step, 3))
        s = summary(run)
        s["what"] = "DecodeRunner.verify_tree(n = %d, binary tree) vs one eager step(), Llama-3-8B layers x %d, batch %d, context %d, ms" % (
            RUN_N, RUN_LAYERS, B, RUN_CONTEXT)
        s["verify_tree_over_step"] = round(s["verify_tree_%d" % RUN_N]["median_ms"] / s["step"]["median_ms"], 2)
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
