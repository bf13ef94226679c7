#!/usr/bin/env python3
"""Where a prefix-cache hit starts to pay (`prefix_cache_min_tokens`): the
forward pass of a prompt's TAIL over a cached head of h tokens
(`LLMEngine._prefill_tails`, the path a hit takes) against the packed prefill
of the whole prompt (the path a miss takes), host time included, for several
h and prompt lengths, with `paged_prefill_attention` off and on (on: with
auto key splits).

The two paths are timed alternately (wall clock around a synchronised call,
several repeats, median and range in ms) on one engine per mode, random-init
weights.

Usage (GPU box): python scripts/bench_prefix_threshold.py [--model llama-3-8b] [--json OUT]
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from kllms_amd.engine.config import EngineConfig  # noqa: E402
from kllms_amd.engine.engine import LLMEngine  # noqa: E402
from kllms_amd.models.llama import ForwardBatch  # noqa: E402

DEV = "cuda:0"
HEADS = (16, 32, 64, 128, 256)
PROMPTS = (320, 1024)


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefix_threshold needs a GPU")
    results = []
    for paged in (False, True):
        eng = LLMEngine(EngineConfig(
            model=args.model, device=DEV, use_hip_graphs=False, seed=0, max_kv_blocks=1024,
            paged_prefill_attention=paged, paged_prefill_key_splits=0 if paged else 1))
        for P in PROMPTS:
            ids = [(i * 37) % 1900 + 1 for i in range(P)]
            seq = eng.kv.alloc_sequence(P)
            slots = torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV)
            tok = torch.tensor(ids, device=DEV)

            def packed():
                batch = ForwardBatch(
                    mode="prefill", positions=torch.arange(P, device=DEV), slot_mapping=slots,
                    kv_caches=eng.kv.layer_caches(),
                    cu_seqlens=torch.tensor([0, P], dtype=torch.int32, device=DEV))
                return eng.model.forward_prefill(tok, batch)

            packed()                      # fills the cache: every head below is "cached"
            for h in HEADS:
                tail = lambda: eng._prefill_tails([seq], [ids], [h])
                tail()
                t_p, t_t = [], []
                for _ in range(args.repeats):
                    t_p += timed(packed, 1)
                    t_t += timed(tail, 1)
                r = {"paged_prefill_attention": paged, "prompt": P, "head": h,
                     "packed_ms": [statistics.median(t_p), min(t_p), max(t_p)],
                     "tail_ms": [statistics.median(t_t), min(t_t), max(t_t)]}
                results.append(r)
                print(f"paged={int(paged)} prompt {P:5d} cached head {h:4d}  packed prefill "
                      f"{r['packed_ms'][0]:7.2f} ms [{r['packed_ms'][1]:.2f}..{r['packed_ms'][2]:.2f}]  "
                      f"tail forward {r['tail_ms'][0]:7.2f} ms [{r['tail_ms'][1]:.2f}..{r['tail_ms'][2]:.2f}]  "
                      f"hit pays: {r['tail_ms'][2] < r['packed_ms'][1]}", flush=True)
            eng.kv.free_sequence(seq)
        del eng
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
