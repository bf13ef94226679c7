"""A/B probe for fp8 (e4m3) Mixtral expert weights against bf16 experts.

    python scripts/bench_moe_fp8.py [--reps 7] [--iters 20] [--json PATH]

Part 1, the dense decode path of ``MixtralMoE``: ``ops.linear_fp8w_batched``
against ``torch.bmm`` on bf16 weights (shipped TunableOp picks loaded, as
bench.py does), E = 8, the Mixtral-8x7B expert shapes gate_up N=28672 K=4096
(x shared by the experts) and down N=4096 K=14336 (x per expert), at M in
{1, 8, 16, 32, 64}. Both arms run in the same process, alternating, on the same
activations. One set of experts is 0.9 GB in fp8 and 1.9 GB in bf16, several
times the 256 MB Infinity Cache; each arm still cycles over two sets, so that
no call starts on the tail the previous call left in the cache. The --iters
calls of an arm are captured into one hipGraph and the replay is timed, as the
engine runs decode; --eager times plain calls instead.

Part 2, the grouped prefill kernels: fp8 against bf16 ``ops.moe_gateup`` /
``ops.moe_down`` at S = --tokens sorted rows spread evenly over the experts
(the shape of scripts/bench_moe.py), plain calls, in TF/s.

Reported per arm: the median over --reps repetitions of --iters calls (device
events) with the min..max spread of the repetitions; part 1 in microseconds
per call and TB/s of WEIGHT BYTES ACTUALLY READ (E*N*K for fp8, 2*E*N*K for
bf16).
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_fp8_weights import load_tunableop, make_runner, time_calls  # noqa: E402
from kllms_amd import ops  # noqa: E402

E = 8
SHAPES = [  # (N, K, name, x shared by the experts)
    (28672, 4096, "gate_up", True),
    (4096, 14336, "down", False),
]
MS = [1, 8, 16, 32, 64]
N_SETS = 2


def expert_set(N, K, g, dev):
    """(q [E, N, K] e4m3, scale [E, N], w [E, N, K] bf16) from one random
    expert (the timing does not depend on the values)."""
    w0 = torch.randn(N, K, generator=g, device=dev, dtype=torch.float32) * 0.02
    q0, s0 = ops.quantize_fp8_rows(w0)
    q = q0.unsqueeze(0).repeat(E, 1, 1)
    s = s0.unsqueeze(0).repeat(E, 1)
    w = w0.bfloat16().unsqueeze(0).repeat(E, 1, 1)
    return q, s, w


def spread(ts, digits=1):
    return f"{min(ts):7.{digits}f}..{max(ts):<7.{digits}f}"


def dense_part(args, dev, g, rows):
    print(f"# dense path, E={E}: {'shape':>20} {'M':>3} | {'fp8 us':>8} {'spread':>16} {'TB/s':>5} | "
          f"{'bf16 us':>8} {'spread':>16} {'TB/s':>5} | fp8/bf16 time")
    for N, K, name, shared in SHAPES:
        q, s, w = expert_set(N, K, g, dev)
        qs = [q] + [q.clone() for _ in range(N_SETS - 1)]
        ws = [w] + [w.clone() for _ in range(N_SETS - 1)]
        wts = [t.transpose(1, 2) for t in ws]
        for M in MS:
            x = torch.randn(M, K, generator=g, device=dev, dtype=torch.float32).bfloat16()
            if shared:
                x8, x16 = x, x.unsqueeze(0).expand(E, M, K)
            else:
                x8 = x16 = x.unsqueeze(0).repeat(E, 1, 1)
            fp8 = lambda i: ops.linear_fp8w_batched(x8, qs[i], s)
            bf16 = lambda i: torch.bmm(x16, wts[i])
            for _ in range(3):
                fp8(0), bf16(0)
            torch.cuda.synchronize()
            run8 = make_runner(fp8, N_SETS, args.iters, args.eager)
            run16 = make_runner(bf16, N_SETS, args.iters, args.eager)
            run8(), run16()
            torch.cuda.synchronize()
            t8, t16 = [], []
            for _ in range(args.reps):                      # alternate the arms
                t8.append(time_calls(run8, args.iters))
                t16.append(time_calls(run16, args.iters))
            del run8, run16
            m8, m16 = statistics.median(t8), statistics.median(t16)
            tb8 = E * N * K / (m8 * 1e-6) / 1e12
            tb16 = 2 * E * N * K / (m16 * 1e-6) / 1e12
            print(f"  {name + f' {N}x{K}':>36} {M:>3} | {m8:8.1f} {spread(t8)} {tb8:5.2f} | "
                  f"{m16:8.1f} {spread(t16)} {tb16:5.2f} | {m8 / m16:5.2f}")
            rows.append(dict(part="dense", name=name, N=N, K=K, M=M, fp8_us=m8, fp8_min=min(t8),
                             fp8_max=max(t8), fp8_tbs=tb8, bf16_us=m16, bf16_min=min(t16),
                             bf16_max=max(t16), bf16_tbs=tb16))
        del qs, ws, wts, q, s, w
        torch.cuda.empty_cache()


def grouped_part(args, dev, g, rows):
    I, H, S, BM = 14336, 4096, args.tokens, 128
    per = (S // E + BM - 1) // BM * BM
    S_pad = per * E
    x = torch.randn(S, H, generator=g, device=dev, dtype=torch.float32).bfloat16() * 0.1
    pad_off = torch.arange(E + 1, dtype=torch.int32, device=dev) * per
    sorted_ids = torch.full((S_pad,), -1, dtype=torch.int32, device=dev)
    n = S // E
    for e in range(E):
        sorted_ids[e * per: e * per + n] = torch.arange(e * n, (e + 1) * n, dtype=torch.int32)
    zeros = torch.zeros(H, dtype=torch.bfloat16, device=dev)
    act = torch.randn(S_pad, I, generator=g, device=dev, dtype=torch.float32).bfloat16()
    act_out = torch.empty(S_pad, I, dtype=torch.bfloat16, device=dev)
    y = torch.empty(S_pad, H, dtype=torch.bfloat16, device=dev)
    print(f"# grouped path, E={E} S_pad={S_pad}: {'kernel':>8} | {'fp8 TF/s':>8} {'ms':>7} {'spread ms':>16} | "
          f"{'bf16 TF/s':>9} {'ms':>7} {'spread ms':>16} | fp8/bf16 time")
    for name, N, K, flops in (("gateup", 2 * I, H, 2 * S_pad * 2 * I * H),
                              ("down", H, I, 2 * S_pad * H * I)):
        q, s, w = expert_set(N, K, g, dev)
        if name == "gateup":
            fp8 = lambda i: ops.moe_gateup(act_out, x, q, sorted_ids, pad_off, zeros, scale=s)
            bf16 = lambda i: ops.moe_gateup(act_out, x, w, sorted_ids, pad_off, zeros)
        else:
            fp8 = lambda i: ops.moe_down(y, act, q, pad_off, scale=s)
            bf16 = lambda i: ops.moe_down(y, act, w, pad_off)
        for _ in range(3):
            fp8(0), bf16(0)
        torch.cuda.synchronize()
        run8 = make_runner(fp8, 1, args.iters, True)
        run16 = make_runner(bf16, 1, args.iters, True)
        t8, t16 = [], []
        for _ in range(args.reps):
            t8.append(time_calls(run8, args.iters) / 1e3)   # ms per call
            t16.append(time_calls(run16, args.iters) / 1e3)
        m8, m16 = statistics.median(t8), statistics.median(t16)
        print(f"  {name:>44} | {flops / m8 / 1e9:8.1f} {m8:7.3f} {spread(t8, 3)} | "
              f"{flops / m16 / 1e9:9.1f} {m16:7.3f} {spread(t16, 3)} | {m8 / m16:5.2f}")
        rows.append(dict(part="grouped", name=name, S_pad=S_pad, fp8_ms=m8, fp8_min=min(t8),
                         fp8_max=max(t8), fp8_tfs=flops / m8 / 1e9, bf16_ms=m16, bf16_min=min(t16),
                         bf16_max=max(t16), bf16_tfs=flops / m16 / 1e9))
        del q, s, w
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=2048)   # sorted rows of the grouped part
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--eager", action="store_true", help="time plain calls, not a graph replay")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_fp8.py needs a GPU")
    dev = "cuda"
    tuned = load_tunableop()
    print(f"# TunableOp picks loaded: {tuned}; reps={args.reps} iters={args.iters} "
          f"dense mode={'eager' if args.eager else 'graph replay'}")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    dense_part(args, dev, g, rows)
    grouped_part(args, dev, g, rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(tunableop=tuned, reps=args.reps, iters=args.iters,
                           mode="eager" if args.eager else "graph", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
