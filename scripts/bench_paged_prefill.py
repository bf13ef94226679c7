#!/usr/bin/env python3
"""Per-layer attention of a chunk of new tokens over the paged cache: the
paged MFMA prefill kernel (`ops.attn_prefill_paged`) against the path it
replaces (`ops.attn_decode_paged` on one row per new token, the [T, nb]
expanded table and context start+i+1), at kernel level.

Llama-3-8B heads (H=32, KVH=8, D=128), one sequence, bf16 and fp8 cache,
(start, q_len) in {(0,2048), (2048,2048), (14336,2048), (4096,128)}; the
packed varlen kernel at (0,2048) for scale. Where the default tile packing of
`build_paged_prefill` is not 8 tiles per workgroup, 8 per workgroup is timed
too.

Key splits (`build_paged_prefill(key_splits=...)`): a second table times, in
the same way and alternately in one run, the unsplit plan (key_splits=1), the
auto plan (key_splits=0) and forced split counts with all of a sequence's
q-tiles packed into one workgroup, on the short-tail shapes that splitting is
meant for, on a batch of 8 sequences and on (14336, 2048), where auto must
return the unsplit plan.

The paths are timed alternately (device events around batches of launches
sized to ~0.25 s each, several repeats, median and range reported) on the
same seeded inputs, outputs compared first. Also prints the logical K/V bytes
each path reads (computed from the shapes: the decode path reads every row's
whole context, the tiled kernel each workgroup's key range once per q-head).

Usage (GPU box): python scripts/bench_paged_prefill.py [--json OUT] [--table all|base|splits]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kllms_amd import ops

DEV = "cuda:0"
H, KVH, D, BS = 32, 8, 128, 16
SHAPES = [(0, 2048), (2048, 2048), (14336, 2048), (4096, 128)]
# the key-split table: batches of (start, q_len)
SPLIT_BATCHES = [[(4096, 128)], [(4096, 32)], [(16384, 128)], [(1024, 64)], [(2048, 64)] * 8,
                 [(14336, 2048)]]
FORCED_SPLITS = (2, 4, 8, 16)


def build(start, n, fp8, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = start + n
    nb = (L + BS - 1) // BS
    NB = nb + 1
    blocks = torch.randperm(NB, generator=g)[:nb].tolist()
    fused = (torch.randn(n, (H + 2 * KVH) * D, generator=g) * 0.5).bfloat16().to(DEV)
    q = fused[:, : H * D].view(n, H, D)            # strided, as in the model
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
    meta = ops.build_paged_prefill([n], [start], [blocks], DEV, BS)
    meta8 = ops.build_paged_prefill([n], [start], [blocks], DEV, BS, tiles_per_group=8)
    bt = torch.tensor(blocks, dtype=torch.int32, device=DEV).unsqueeze(0).expand(n, nb).contiguous()
    ctx = torch.arange(start + 1, L + 1, dtype=torch.int32, device=DEV)
    # the new keys' fresh K/V, for the packed kernel at start == 0
    slots = torch.tensor([blocks[p // BS] * BS + p % BS for p in range(start, L)], device=DEV)
    elem = 1 if fp8 else 2
    row_bytes = 2 * D * elem                        # K + V of one key, one kv head
    bytes_decode = sum(start + i + 1 for i in range(n)) * KVH * row_bytes

    def tiled_bytes(m):
        qpos = m.grp_qpos0.view(-1, 8).tolist()
        return sum(start + min(n, max(r) + 32) for r in qpos) * H * row_bytes

    return dict(q=q, fused=fused, kc=kc, vc=vc, ks=ks, vs=vs, meta=meta, meta8=meta8, bt=bt,
                ctx=ctx, k_new=k[slots], v_new=v[slots], bytes_decode=bytes_decode,
                bytes_new=tiled_bytes(meta), bytes_new8=tiled_bytes(meta8),
                same_packing=meta.n_groups == meta8.n_groups)


def build_batch(seqs, fp8, seed=0):
    """Caches, strided q and block lists of a batch of (start, q_len)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    need = [(s + n + BS - 1) // BS for s, n in seqs]
    NB = sum(need) + 1
    perm = torch.randperm(NB, generator=g).tolist()
    blocks, at = [], 0
    for nb in need:
        blocks.append(perm[at: at + nb])
        at += nb
    T = sum(n for _, n in seqs)
    fused = (torch.randn(T, (H + 2 * KVH) * D, generator=g) * 0.5).bfloat16().to(DEV)
    q = fused[:, : H * D].view(T, H, D)
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
    return dict(q=q, fused=fused, kc=kc, vc=vc, ks=ks, vs=vs, blocks=blocks,
                lens=[n for _, n in seqs], starts=[s for s, _ in seqs])


def split_table(repeats):
    """Unsplit, auto and forced key splits, timed alternately per batch."""
    scale = D ** -0.5
    results = []
    for seqs in SPLIT_BATCHES:
        for fp8 in (False, True):
            c = build_batch(seqs, fp8)
            plan = lambda **kw: ops.build_paged_prefill(
                c["lens"], c["starts"], c["blocks"], DEV, BS, num_q_heads=H, **kw)
            run = lambda m: (lambda: ops.attn_prefill_paged(
                c["q"], c["kc"], c["vc"], m, scale, c["ks"], c["vs"]))
            unsplit, auto = plan(key_splits=1), plan(key_splits=0)
            names, fns = ["unsplit", "auto"], [run(unsplit), run(auto)]
            if len(seqs) == 1 and seqs[0][1] <= 256:
                for k in FORCED_SPLITS:
                    m = plan(key_splits=k, tiles_per_group=8)
                    if m.has_splits and m.max_splits == k:
                        names.append(f"k={k}")
                        fns.append(run(m))
            err = (fns[0]().float() - fns[1]().float()).abs().max().item()
            ts, iters = measure(fns, repeats)
            label = (f"{len(seqs)} x ({seqs[0][0]}, {seqs[0][1]})" if len(seqs) > 1
                     else f"({seqs[0][0]}, {seqs[0][1]})")
            r = {"batch": label, "cache": "fp8" if fp8 else "bf16",
                 "auto_splits": auto.seq_nsplit.tolist() if auto.has_splits else None,
                 "workgroups_unsplit": unsplit.n_groups * H, "workgroups_auto": auto.n_groups * H,
                 "max_abs_diff_auto_vs_unsplit": err, "iters": iters,
                 "us": {n: {"median": t[0], "min": t[1], "max": t[2]} for n, t in zip(names, ts)}}
            results.append(r)
            print(f"{label:18s} {r['cache']:4s} auto splits {r['auto_splits']} "
                  f"wgs {r['workgroups_unsplit']} -> {r['workgroups_auto']}  "
                  + "  ".join(f"{n} {t[0]:.1f} us [{t[1]:.1f}..{t[2]:.1f}]"
                              for n, t in zip(names, ts))
                  + f"  max|auto - unsplit| {err:.4f}", flush=True)
            del c, fns
            torch.cuda.empty_cache()
    return results


def time_batch(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters   # us per call


def measure(fns, repeats, target_s=0.25):
    """Median and range (us) of each fn; the fns are timed alternately."""
    iters = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        one = max(time_batch(fn, 3), 1.0)
        iters.append(int(min(2000, max(5, target_s * 1e6 / one))))
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ts[i].append(time_batch(fn, iters[i]))
    return [(statistics.median(t), min(t), max(t)) for t in ts], iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--table", choices=("all", "base", "splits"), default="all")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_prefill needs a GPU")

    scale = D ** -0.5
    results = []
    for start, n in (SHAPES if args.table != "splits" else []):
        for fp8 in (False, True):
            c = build(start, n, fp8)
            old = lambda: ops.attn_decode_paged(
                c["q"], c["kc"], c["vc"], c["bt"], c["ctx"], scale, c["ks"], c["vs"])
            new = lambda: ops.attn_prefill_paged(
                c["q"], c["kc"], c["vc"], c["meta"], scale, c["ks"], c["vs"])
            new8 = lambda: ops.attn_prefill_paged(
                c["q"], c["kc"], c["vc"], c["meta8"], scale, c["ks"], c["vs"])
            err = (old().float() - new().float()).abs().max().item()
            fns = [old, new] + ([] if c["same_packing"] else [new8])
            if start == 0 and not fp8:
                cu = torch.tensor([0, n], dtype=torch.int32, device=DEV)
                fns.append(lambda: ops.attn_prefill_varlen(c["q"], c["k_new"], c["v_new"], cu, scale))
            (t_old, t_new, *rest), iters = measure(fns, args.repeats)
            r = {
                "start": start, "q_len": n, "cache": "fp8" if fp8 else "bf16",
                "tiles_per_group": int((c["meta"].grp_qpos0.view(-1, 8) >= 0).sum(1).max()),
                "decode_path_us": t_old[0], "decode_path_us_range": list(t_old[1:]),
                "paged_prefill_us": t_new[0], "paged_prefill_us_range": list(t_new[1:]),
                "speedup": t_old[0] / t_new[0],
                "speedup_worst": t_old[1] / t_new[2],
                "kv_mb_decode_path": c["bytes_decode"] / 1e6, "kv_mb_paged_prefill": c["bytes_new"] / 1e6,
                "max_abs_diff": err, "iters": iters,
            }
            line = (f"start {start:5d} q_len {n:4d} {r['cache']:4s} tiles/wg={r['tiles_per_group']}  "
                    f"decode path {t_old[0]:10.1f} us [{t_old[1]:.1f}..{t_old[2]:.1f}]  "
                    f"paged prefill {t_new[0]:8.1f} us [{t_new[1]:.1f}..{t_new[2]:.1f}]  "
                    f"x{r['speedup']:.1f} (worst x{r['speedup_worst']:.1f})  "
                    f"K/V MB {r['kv_mb_decode_path']:.0f} -> {r['kv_mb_paged_prefill']:.0f}  "
                    f"max|diff| {err:.4f}")
            if not c["same_packing"]:
                t8 = rest.pop(0)
                r["paged_prefill_8_per_wg_us"] = t8[0]
                r["paged_prefill_8_per_wg_us_range"] = list(t8[1:])
                line += f"  | 8 tiles/wg {t8[0]:8.1f} us [{t8[1]:.1f}..{t8[2]:.1f}]"
            if rest:
                tp = rest.pop(0)
                r["packed_prefill_us"] = tp[0]
                r["packed_prefill_us_range"] = list(tp[1:])
                line += f"  | packed kernel {tp[0]:8.1f} us [{tp[1]:.1f}..{tp[2]:.1f}]"
            results.append(r)
            print(line, flush=True)
            del c
            torch.cuda.empty_cache()
    if args.table != "base":
        results.append({"key_splits": split_table(args.repeats)})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
