#!/usr/bin/env python3
"""Per-layer decode attention: per-stream path (shared=None) vs the
shared-prefix cascade, at kernel level.

Shapes (streams = groups x n; every group shares `shared` prompt keys, each
stream then owns its private suffix up to `ctx` keys):

  (a) headline     24 x 5   KVH=8 GQA=4  shared 512   ctx 576
  (b) parse16-like  2 x 16  KVH=8 GQA=4  shared 4096  ctx 4160
  (c) 70B-like     24 x 5   KVH=8 GQA=8  shared 512   ctx 576

each with the bf16 and the fp8 cache. The two paths are timed alternately
(device events around batches of launches, several repeats, median and range
reported) on the same seeded inputs, outputs compared first. Also prints the
logical K/V bytes each path reads (computed from the shapes).

Usage (GPU box): python scripts/bench_shared_prefix_decode.py [--json OUT]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kllms_amd import ops
from kllms_amd.engine.shared_prefix import build_shared_prefix_tiles

DEV = "cuda:0"
D, BS, CHUNK = 128, 16, 256

SHAPES = [
    ("a-headline", 24, 5, 8, 4, 512, 576),
    ("b-parse16", 2, 16, 8, 4, 4096, 4160),
    ("c-70b-like", 24, 5, 8, 8, 512, 576),
]


def build(groups, n, kvh, gqa, shared_keys, ctx, fp8, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B = groups * n
    sh_blocks = shared_keys // BS
    nblk = (ctx + BS - 1) // BS
    NB = groups * sh_blocks + B * (nblk - sh_blocks) + 1
    block_lists, fork_ids = [], []
    nxt = 0
    for gi in range(groups):
        shared = list(range(nxt, nxt + sh_blocks))
        nxt += sh_blocks
        for _ in range(n):
            block_lists.append(shared + list(range(nxt, nxt + nblk - sh_blocks)))
            nxt += nblk - sh_blocks
            fork_ids.append(gi)
    bt = torch.tensor(block_lists, dtype=torch.int32, device=DEV)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    q = (torch.randn(B, kvh * gqa, D, generator=g) * 0.5).bfloat16().to(DEV)
    k = (torch.randn(NB * BS, kvh, D, generator=g) * 0.3).bfloat16().to(DEV)
    v = (torch.randn(NB * BS, kvh, D, generator=g) * 0.3).bfloat16().to(DEV)
    slots = torch.arange(NB * BS, device=DEV)
    dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc = torch.zeros(NB, kvh, BS, D, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    ks = vs = None
    if fp8:
        ks = torch.ones(NB, kvh, BS, device=DEV)
        vs = torch.ones_like(ks)
    ops.store_kv(k, v, kc, vc, slots, ks, vs)
    tiles = build_shared_prefix_tiles(block_lists, fork_ids, BS, gqa)
    elem = 1 if fp8 else 2
    row_bytes = 2 * kvh * D * elem           # K + V, all kv heads, one key
    S = tiles.tile_chunks[0] if tiles.n_tiles else 0
    bytes_plain = B * ctx * row_bytes
    bytes_casc = (tiles.n_tiles * S * CHUNK + B * (ctx - S * CHUNK)) * row_bytes
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, bt=bt, lens=lens, tiles=tiles,
                shared=tiles.to_tensors(DEV), bytes_plain=bytes_plain, bytes_casc=bytes_casc)


def time_batch(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared_prefix_decode needs a GPU")

    scale = D ** -0.5
    results = []
    for name, groups, n, kvh, gqa, shared_keys, ctx in SHAPES:
        for fp8 in (False, True):
            c = build(groups, n, kvh, gqa, shared_keys, ctx, fp8)
            plain = lambda: ops.attn_decode_paged(
                c["q"], c["kc"], c["vc"], c["bt"], c["lens"], scale, c["ks"], c["vs"])
            casc = lambda: ops.attn_decode_paged(
                c["q"], c["kc"], c["vc"], c["bt"], c["lens"], scale, c["ks"], c["vs"],
                shared=c["shared"])
            err = (plain().float() - casc().float()).abs().max().item()
            for _ in range(30):
                plain()
                casc()
            torch.cuda.synchronize()
            tp, tc = [], []
            for _ in range(args.repeats):      # alternate the two paths
                tp.append(time_batch(plain, args.iters))
                tc.append(time_batch(casc, args.iters))
            r = {
                "shape": name, "cache": "fp8" if fp8 else "bf16",
                "streams": groups * n, "gqa": gqa, "shared_keys": shared_keys, "ctx": ctx,
                "n_tiles": c["tiles"].n_tiles,
                "plain_us": statistics.median(tp), "plain_us_range": [min(tp), max(tp)],
                "cascade_us": statistics.median(tc), "cascade_us_range": [min(tc), max(tc)],
                "speedup": statistics.median(tp) / statistics.median(tc),
                "kv_mb_plain": c["bytes_plain"] / 1e6, "kv_mb_cascade": c["bytes_casc"] / 1e6,
                "max_abs_diff": err,
            }
            results.append(r)
            print(f"{name:12s} {r['cache']:4s} tiles={r['n_tiles']:3d}  "
                  f"per-stream {r['plain_us']:8.1f} us [{min(tp):.1f}..{max(tp):.1f}]  "
                  f"cascade {r['cascade_us']:8.1f} us [{min(tc):.1f}..{max(tc):.1f}]  "
                  f"x{r['speedup']:.2f}  K/V MB {r['kv_mb_plain']:.0f} -> {r['kv_mb_cascade']:.0f}  "
                  f"max|diff| {err:.4f}", flush=True)
            del c
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
