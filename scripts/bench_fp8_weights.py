"""A/B probe: weight-only fp8 GEMM (ops.linear_fp8w) vs F.linear on bf16 weights.

    python scripts/bench_fp8_weights.py [--reps 7] [--iters 40] [--json PATH]

The four Llama-3-8B decode projections at M in {1, 16, 120, 256}. For every
(shape, M) both arms run in the same process, alternating, on the same
activations; the bf16 arm runs with the shipped TunableOp picks loaded (as
bench.py does). Each arm cycles through enough weight copies (>= 1 GiB) that
no call finds its weight in the 256 MB Infinity Cache: a decode step streams
16 GB of weights, so a cached weight would flatter both arms.

The --iters calls of an arm are captured into one hipGraph and the replay is
timed, because that is how the engine runs decode (the layers are graph-
replayed, so host launch cost is not part of a step); --eager times plain
calls instead, host launch cost included.

Reported per arm: median microseconds per call over --reps repetitions of
--iters calls (device events), the min..max spread of the repetitions, and
TB/s of WEIGHT BYTES ACTUALLY READ (N*K for fp8, 2*N*K for bf16).
"""

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kllms_amd import ops  # noqa: E402

SHAPES = [  # (N, K, name): the 8B decode projections
    (6144, 4096, "qkv"),
    (4096, 4096, "o"),
    (28672, 4096, "gate_up"),
    (4096, 14336, "down"),
]
MS = [1, 16, 120, 256]


def load_tunableop() -> bool:
    """The shipped offline picks, read-only (same recipe as bench.py)."""
    shipped = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "kllms_amd", "tunableop", "tunableop_gfx9500.csv")
    if not os.path.exists(shipped):
        return False
    tmp = tempfile.mkdtemp(prefix="kllms_tunableop_")
    for i in range(8):
        shutil.copy(shipped, os.path.join(tmp, f"tunableop_gfx950{i}.csv"))
    try:
        torch.cuda.tunable.enable(True)
        torch.cuda.tunable.tuning_enable(False)
        torch.cuda.tunable.set_filename(os.path.join(tmp, "tunableop_gfx950.csv"),
                                        insert_device_ordinal=True)
        torch.cuda.tunable.read_file()
        return True
    except Exception as e:  # report, keep measuring on the default picks
        print(f"tunableop not loaded ({e})", file=sys.stderr)
        return False


def make_runner(fn, n_copies, iters, eager):
    """A callable running `iters` calls that cycle over the weight copies:
    a hipGraph replay, or the plain loop with --eager."""
    def loop():
        for i in range(iters):
            fn(i % n_copies)

    if eager:
        return loop
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loop()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loop()
    return g.replay


def time_calls(run, iters):
    """Microseconds per call of one run of `iters` calls."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    run()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--eager", action="store_true", help="time plain calls, not a graph replay")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8_weights.py needs a GPU")
    dev = "cuda"
    tuned = load_tunableop()
    print(f"# TunableOp picks loaded: {tuned}; reps={args.reps} iters={args.iters} "
          f"mode={'eager' if args.eager else 'graph replay'}")
    print(f"# {'shape':>20} {'M':>4} | {'fp8 us':>8} {'spread':>15} {'TB/s':>6} | "
          f"{'bf16 us':>8} {'spread':>15} {'TB/s':>6} | fp8/bf16 time")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for N, K, name in SHAPES:
        n_copies = max(2, -(-(1 << 30) // (N * K)))        # >= 1 GiB of fp8 bytes
        w0 = torch.randn(N, K, generator=g, device=dev, dtype=torch.float32) * 0.02
        q0, s0 = ops.quantize_fp8_rows(w0)
        qs = [q0.clone() for _ in range(n_copies)]
        n_bf = max(2, n_copies // 2)                        # >= 1 GiB of bf16 bytes
        ws = [w0.bfloat16().clone() for _ in range(n_bf)]
        del w0
        for M in MS:
            x = torch.randn(M, K, generator=g, device=dev, dtype=torch.float32).bfloat16()
            fp8 = lambda i: ops.linear_fp8w(x, qs[i], s0)
            bf16 = lambda i: torch.nn.functional.linear(x, ws[i % n_bf])
            for _ in range(3):
                fp8(0), bf16(0)
            torch.cuda.synchronize()
            run8 = make_runner(fp8, n_copies, args.iters, args.eager)
            run16 = make_runner(bf16, n_bf, args.iters, args.eager)
            run8(), run16()
            torch.cuda.synchronize()
            t8, t16 = [], []
            for _ in range(args.reps):                      # alternate the arms
                t8.append(time_calls(run8, args.iters))
                t16.append(time_calls(run16, args.iters))
            del run8, run16
            m8, m16 = statistics.median(t8), statistics.median(t16)
            tb8 = N * K / (m8 * 1e-6) / 1e12
            tb16 = 2 * N * K / (m16 * 1e-6) / 1e12
            print(f"  {name + f' {N}x{K}':>20} {M:>4} | {m8:8.1f} {min(t8):6.1f}..{max(t8):<7.1f} "
                  f"{tb8:6.2f} | {m16:8.1f} {min(t16):6.1f}..{max(t16):<7.1f} {tb16:6.2f} | "
                  f"{m8 / m16:5.2f}")
            rows.append(dict(name=name, N=N, K=K, M=M, fp8_us=m8, fp8_min=min(t8), fp8_max=max(t8),
                             fp8_tbs=tb8, bf16_us=m16, bf16_min=min(t16), bf16_max=max(t16),
                             bf16_tbs=tb16))
        del qs, ws
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(tunableop=tuned, reps=args.reps, iters=args.iters,
                           mode="eager" if args.eager else "graph", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
