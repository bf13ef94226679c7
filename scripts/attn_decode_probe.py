"""Standalone perf probe for the per-stream paged decode attention kernel.

Llama-3-8B geometry (H=32, KVH=8, D=128, BS=16), every stream with its own
(disjoint, shuffled) blocks, B = 40 / 120 / 240 streams at ctx 576 / 2048, with
the bf16 and the fp8 cache. One call is the partial kernel plus the reduce, as
the engine issues them. Timed with device events around batches of launches,
several repeats; prints the median with [min..max] in us and the logical K+V
bytes over the median (each block streams its chunk once, so that rate is the
kernel's distance from the memory roofline).

Usage (GPU box): python scripts/attn_decode_probe.py [--json OUT]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kllms_amd import ops  # noqa: E402

DEV = "cuda:0"
H, KVH, D, BS = 32, 8, 128, 16
SHAPES = [(B, ctx) for ctx in (576, 2048) for B in (40, 120, 240)]


def build(B, ctx, fp8, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nblk = (ctx + BS - 1) // BS
    NB = B * nblk + 8
    k = (torch.randn(NB * BS, KVH, D, generator=g) * 0.3).bfloat16().to(DEV)
    v = (torch.randn(NB * BS, KVH, D, generator=g) * 0.3).bfloat16().to(DEV)
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc = torch.zeros(NB, KVH, BS, D, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    ks = vs = None
    if fp8:
        ks = torch.ones(NB, KVH, BS, device=DEV)
        vs = torch.ones_like(ks)
    ops.store_kv(k, v, kc, vc, torch.arange(NB * BS, device=DEV), ks, vs)
    bt = torch.randperm(NB - 8, generator=g)[: B * nblk].to(torch.int32).view(B, nblk).to(DEV)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    q = (torch.randn(B, H, D, generator=g) * 0.5).bfloat16().to(DEV)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, bt=bt, lens=lens)


def time_batch(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def measure(fn, iters, repeats):
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    return [time_batch(fn, iters) for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_decode_probe needs a GPU")

    scale = D ** -0.5
    results = []
    for B, ctx in SHAPES:
        for fp8 in (False, True):
            c = build(B, ctx, fp8)
            t = measure(lambda: ops.attn_decode_paged(
                c["q"], c["kc"], c["vc"], c["bt"], c["lens"], scale, c["ks"], c["vs"]),
                args.iters, args.repeats)
            med = statistics.median(t)
            kv_bytes = 2 * B * KVH * ctx * D * (1 if fp8 else 2)
            r = {"B": B, "ctx": ctx, "cache": "fp8" if fp8 else "bf16", "us": med,
                 "us_range": [min(t), max(t)], "kv_tb_s": kv_bytes / med / 1e6}
            results.append(r)
            print(f"B={B:3d} ctx={ctx:4d} {r['cache']:4s}: {med:7.1f} us "
                  f"[{min(t):.1f}..{max(t):.1f}] -> {r['kv_tb_s']:.2f} TB/s of K+V", flush=True)
            del c
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
