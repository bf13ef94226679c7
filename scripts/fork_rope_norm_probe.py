"""Standalone perf probe for the fork's tail-block copies, the fused RoPE +
KV-store kernel and fused_add_rmsnorm.

Llama-3-8B geometry (H=32, KVH=8, D=128, BS=16, 32 layers). Three groups:

  copy     one fork of 24 prompts x 5 streams (120 tail blocks) on a
           production-sized cache (--blocks per layer; above 65 536 a layer of
           the block array spans more than 2^31 bytes), as ``fork_batch`` where
           the tree has it, and as the 240 per-layer-split ``copy_`` calls it
           replaces. Device time (events) and host wall time up to a final
           synchronise, per fork.
  rope     rope_inplace, store_kv, the two back to back and (where the tree has
           it) rope_store_kv, at T = 128 (decode) and T = 12 288 (packed
           prefill), bf16 and fp8 cache.
  rmsnorm  fused_add_rmsnorm at 128 x 4096 and 128 x 8192.

Timed with device events around batches of calls; prints the median with
[min..max] of the repeats in us. The rope and rmsnorm batches are captured
into a graph and replayed (the decode forward runs that way, and eager launches
of kernels this short measure the host); ``--eager`` times plain launches. ``--tree DIR`` imports kllms_amd from another
checkout (a build of the parent commit), so that a job can alternate the two.

Usage (GPU box): python scripts/fork_rope_norm_probe.py [--tree DIR] [--json OUT]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

DEV = "cuda:0"
H, KVH, D, BS, LAYERS = 32, 8, 128, 16, 32


def time_batch(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


USE_GRAPH = True


def measure(fn, iters, repeats, warm=30):
    """us per call over `repeats` batches of `iters` calls. With USE_GRAPH the
    batch is captured once and replayed, as the engine's decode forward is:
    kernels of a few us are otherwise timed at the host's launch rate."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    if not USE_GRAPH:
        return [time_batch(fn, iters) for _ in range(repeats)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return [time_batch(graph.replay, 1) / iters for _ in range(repeats)]


def report(results, group, name, t, **extra):
    med = statistics.median(t)
    r = {"group": group, "name": name, "us": med, "us_range": [min(t), max(t)], **extra}
    results.append(r)
    print(f"{group:8s} {name:34s}: {med:9.1f} us [{min(t):.1f}..{max(t):.1f}]", flush=True)


def probe_copy(results, args):
    from kllms_amd.engine.kvcache import PagedKVCache
    free, _ = torch.cuda.mem_get_info()
    layers = LAYERS
    per_layer = 2 * args.blocks * KVH * BS * D * 2
    while layers > 1 and layers * per_layer > 0.8 * free:
        layers //= 2
    kv = PagedKVCache(layers, KVH, D, BS, args.blocks, DEV)
    parents = [kv.alloc_sequence(520) for _ in range(24)]      # tail of 8 tokens
    print(f"copy: cache of {layers} layers x {args.blocks} blocks "
          f"({layers * per_layer / 2**30:.0f} GiB), 24 parents x 5 streams", flush=True)

    def legacy():
        kids = []
        for p in parents:
            for _ in range(5):
                dst = kv.allocator.alloc()
                kv.k_all[:, dst].copy_(kv.k_all[:, p.blocks[-1]])
                kv.v_all[:, dst].copy_(kv.v_all[:, p.blocks[-1]])
                kids.append(dst)
        return kids

    def batched():
        return [b for ks in kv.fork_batch([(p, 5) for p in parents]) for k in ks
                for b in k.blocks]

    def release(blocks):
        for b in blocks:
            kv.allocator.free(b)

    variants = [("240 copy_ calls", legacy)]
    if hasattr(kv, "fork_batch"):
        variants.append(("fork_batch 24 x 5", batched))
    for name, fn in variants:
        dev_us, wall_us = [], []
        for rep in range(args.repeats + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            taken = [fn() for _ in range(args.copy_iters)]
            e1.record()
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            for blocks in taken:
                release(blocks)
            if rep:                                     # the first round warms up
                dev_us.append(e0.elapsed_time(e1) * 1e3 / args.copy_iters)
                wall_us.append((w1 - w0) * 1e6 / args.copy_iters)
        report(results, "copy", name + " (device)", dev_us, layers=layers)
        report(results, "copy", name + " (host wall)", wall_us, layers=layers)
    del kv
    torch.cuda.empty_cache()


def probe_rope(results, args, ops):
    from kllms_amd.ops import torch_ref
    cs = torch_ref.build_cos_sin_cache(D, 8192, 500000.0, "cpu").to(DEV)
    for T in (128, 12288):
        for fp8 in (False, True):
            g = torch.Generator().manual_seed(T)
            fused = (torch.randn(T, (H + 2 * KVH) * D, generator=g) * 0.5).bfloat16().to(DEV)
            q = fused[:, : H * D].view(T, H, D)
            k = fused[:, H * D: (H + KVH) * D].view(T, KVH, D)
            v = fused[:, (H + KVH) * D:].view(T, KVH, D)
            pos = torch.randint(0, 8192, (T,), generator=g).to(DEV)
            NB = T // BS + 64
            slots = torch.randperm(NB * BS, generator=g)[:T].to(DEV)
            dt = torch.float8_e4m3fn if fp8 else torch.bfloat16
            kc = torch.zeros(NB, KVH, BS, D, dtype=dt, device=DEV)
            vc = torch.zeros_like(kc)
            ks = torch.ones(NB, KVH, BS, device=DEV) if fp8 else None
            vs = torch.ones_like(ks) if fp8 else None

            def rope():
                ops.rope_inplace(q, k, pos, cs)

            def store():
                ops.store_kv(k, v, kc, vc, slots, ks, vs)

            def both():
                rope()
                store()

            def one():
                ops.rope_store_kv(q, k, v, pos, cs, kc, vc, slots, ks, vs)

            tag = f"T={T} {'fp8' if fp8 else 'bf16'}"
            iters = args.iters if T == 128 else max(20, args.iters // 4)
            todo = [("rope_inplace", rope), ("store_kv", store), ("rope_inplace + store_kv", both)]
            if hasattr(ops, "rope_store_kv"):
                todo.append(("rope_store_kv", one))
            for name, fn in todo:
                report(results, "rope", f"{name} {tag}", measure(fn, iters, args.repeats),
                       T=T, cache="fp8" if fp8 else "bf16")


def probe_rmsnorm(results, args, ops):
    for rows, n in ((128, 4096), (128, 8192)):
        g = torch.Generator().manual_seed(n)
        x = (torch.randn(rows, n, generator=g) * 0.01).bfloat16().to(DEV)
        res = torch.randn(rows, n, generator=g).bfloat16().to(DEV)
        w = (torch.randn(n, generator=g) * 0.5 + 1.0).bfloat16().to(DEV)
        report(results, "rmsnorm", f"fused_add_rmsnorm {rows} x {n}",
               measure(lambda: ops.fused_add_rmsnorm(x, res, w, 1e-5), args.iters, args.repeats),
               rows=rows, n=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import kllms_amd from (default: this one)")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--groups", default="copy,rope,rmsnorm")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--copy-iters", type=int, default=5, help="forks per timed round")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=70000, help="cache blocks per layer")
    ap.add_argument("--eager", action="store_true",
                    help="time eager launches instead of a replayed graph (rope, rmsnorm)")
    args = ap.parse_args()
    global USE_GRAPH
    USE_GRAPH = not args.eager
    if not torch.cuda.is_available():
        raise SystemExit("fork_rope_norm_probe needs a GPU")
    sys.path.insert(0, os.path.abspath(args.tree))
    from kllms_amd import ops
    print(f"tree: {os.path.abspath(args.tree)}", flush=True)

    results = []
    groups = args.groups.split(",")
    if "rope" in groups:
        probe_rope(results, args, ops)
    if "rmsnorm" in groups:
        probe_rmsnorm(results, args, ops)
    if "copy" in groups:
        probe_copy(results, args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
