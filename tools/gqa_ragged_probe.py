"""What does a ragged head tile cost?  Dense KV4 decode attention (single_query_attention: split partials + merge) at
Yi-34B's shape -- bs 16, 1024 cached tokens, 56 q heads over 8 kv heads: ratio 7, one tile of 8 with one padded slot per
kv head -- against 64 q heads over 8 kv heads (ratio 8: the same tile, whole) on the SAME KV pools.

Timed as bench.py times a kernel: one HIP graph of one launch per "layer" (32 pool sets, ~600 MB: cold), replayed, HIP
events around the replays; the two ratios alternate, REPEATS times each, and the spread (max - min over the repeats) is
reported next to the medians.  The padded slot does the work of a real head, so ratio 7 should take no longer than
ratio 8 plus that spread.

    python tools/gqa_ragged_probe.py [--out FILE.json]

The measurement runs in a child process under its own time limit; the parent only starts it and relays its JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, HK, D, TPB, NL, REPEATS, REPLAYS = 16, 1024, 8, 128, 64, 32, 7, 6
ROPE_BASE = 5000000.0


def measure():
    import statistics
    import torch
    sys.path.insert(0, ROOT)
    import omniserve_backend.fused_attention_pure_dense as fa
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    pps = (T + 1 + TPB - 1) // TPB
    n_pages, data = B * pps, HK * TPB * D // 2
    page_bytes = data + 2 * HK * TPB * 2
    tables = []
    keep = []
    for _ in range(NL):
        tab = torch.empty((B, 2, pps), dtype=torch.int64, device=dev)
        for kv in range(2):
            pool = torch.empty((n_pages, page_bytes), dtype=torch.uint8, device=dev)
            pool[:, :data] = torch.randint(0, 256, (n_pages, data), dtype=torch.uint8, device=dev, generator=gen)
            tail = pool[:, data:].view(torch.float16).view(n_pages, 2, HK * TPB)
            tail[:, 0] = 0.25 * (0.5 + torch.rand((n_pages, HK * TPB), device=dev, generator=gen))
            tail[:, 1] = 7.5
            tab[:, kv] = pool.data_ptr() + torch.randperm(n_pages, device=dev, generator=gen).view(B, pps) * page_bytes
            keep.append(pool)
        tables.append(tab)
    lens = torch.full((B,), T + 1, dtype=torch.int32, device=dev)
    k = torch.randn((B, HK, D), device=dev, generator=gen).half()
    v = torch.randn((B, HK, D), device=dev, generator=gen).half()
    qs = {hq: (0.5 * torch.randn((B, hq, D), device=dev, generator=gen)).half() for hq in (56, 64)}

    def graph_of(hq):
        def fn(i):
            return fa.single_query_attention(qs[hq], k, v, tables[i], lens, None, 65536, TPB, HK * D // 2, T + 1, D,
                                             ROPE_BASE, True, True, True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(NL):
                fn(i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(NL):
                fn(i)
        g.replay()
        torch.cuda.synchronize()
        return g

    def time_us(g):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(REPLAYS):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / (REPLAYS * NL)

    graphs = {hq: graph_of(hq) for hq in (56, 64)}
    us = {56: [], 64: []}
    for _ in range(REPEATS):
        for hq in (56, 64):
            us[hq].append(time_us(graphs[hq]))
    res = {"what": "dense KV4 decode attention (partials + merge), bs %d, %d cached tokens, %d kv heads, us per launch pair; "
                   "%d pool sets rotated (cold), %d repeats x %d graph replays, the two ratios alternating" % (B, T, HK, NL, REPEATS, REPLAYS),
           "device": torch.cuda.get_device_name(0)}
    for hq in (56, 64):
        res["ratio_%d" % (hq // HK)] = {"q_heads": hq, "median_us": round(statistics.median(us[hq]), 2),
                                        "min_us": round(min(us[hq]), 2), "max_us": round(max(us[hq]), 2),
                                        "repeats_us": [round(x, 2) for x in us[hq]]}
    spread = max(max(us[hq]) - min(us[hq]) for hq in (56, 64))
    d = res["ratio_7"]["median_us"] - res["ratio_8"]["median_us"]
    res["spread_us"] = round(spread, 2)
    res["ratio_7_minus_ratio_8_us"] = round(d, 2)
    res["ratio_7_no_slower_than_ratio_8_plus_spread"] = bool(d <= spread)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true", help="(internal) run the measurement in this process")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--timeout", type=int, default=180)
    a = ap.parse_args()
    if a.measure:
        measure()
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], capture_output=True, text=True, timeout=a.timeout)
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
