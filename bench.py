#!/usr/bin/env python3
"""Flagship benchmark: end-to-end n-way consensus serving on MI355X.

Measures the BASELINE.json headline metric — end-to-end consensus requests/sec
(and per-request latency) at n=5 on Llama-3-8B TP=1 — on synthetic prompts and
random-init weights (no network). Each timed step serves a fixed batch of
consensus requests END TO END **through the public client API**
(``AsyncKLLMs().chat.completions.create`` — the literal L4 contract,
reference k_llms/client.py:31-72): concurrent create() calls merge in the
continuous-batching scheduler (shared prefill, n fanned decode streams per
request, HIP kernels, paged KV, hipGraph decode), and each call returns a
consolidated KLLMsChatCompletion with likelihoods — consensus inside the
timed region.

Configs (BASELINE.json):
  --config llama8b   (default) chat.completions.create n=5, Llama-3-8B
  --config parse16   chat.completions.parse, nested Pydantic schema,
                     n=16 + likelihoods (BASELINE config 3)
  --config mixtral8  Mixtral-8x7B parse() n=8 (BASELINE config 5)
  --config llama70b  Llama-3-70B create n=5 (BASELINE config 4; TP=8 with
                     --parallel tp under an 8-rank launch)

Multi-GPU (--gpus N, launched by torch.distributed.run with one rank per GPU):
default is data-parallel weak scaling — each rank runs an independent TP=1
engine serving its own request stream; the reported value is the whole-job
aggregate. ``--parallel tp`` instead shards ONE engine across all ranks
(column/row-parallel layers + RCCL/xGMI all-reduce): rank 0 runs the client
and scheduler, other ranks follow in lockstep (parallel/serve.py).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
Rank 0 prints exactly one JSON result line.

A plain run does only what the headline figure needs: build the engine, warm
up, time the K steps, print the line. ``--dump-outputs DIR`` additionally
writes what the LAST timed step returned to its callers (see dump_outputs)
so two builds can be compared output for output; prompts, request seeds and
weight-init seed depend only on the arguments. ``--full`` is where any
measurement beyond the headline belongs (baselines, other configs, per-kernel
figures); the benchmark has none today, so it currently adds nothing.
"""

import argparse
import asyncio
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REFERENCE_BASELINE = {
    # BASELINE.md rows (remote OpenAI API numbers, context bar)
    "llama8b": 1.2,    # consensus n=3 throughput (req/s)
    "llama70b": 1.2,
    "parse16": 0.7,    # structured output throughput
    "mixtral8": 0.7,
}


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(msg, file=sys.stderr, flush=True)


def _likelihood_leaves(node) -> list:
    """Leaf confidences in traversal order (dict insertion / list order)."""
    leaves = []

    def walk(v):
        if isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
        elif isinstance(v, (int, float)):
            leaves.append(float(v))

    walk(node)
    return leaves


def _mean_likelihood(node) -> float:
    """Average of all leaf confidences — the reference's 'consensus quality'
    scale (README_TESTS.md:269-273: 0.8-0.9 good)."""
    leaves = _likelihood_leaves(node)
    return sum(leaves) / len(leaves) if leaves else 0.0


def _enable_tunableop(local_rank: int) -> None:
    """Load the shipped offline GEMM tuning results (read-only). The decode-
    shape GEMMs (M = graph bucket) are ~30% faster under the tuned algorithm
    picks than the default heuristics (see kllms_amd/tunableop/)."""
    import shutil
    import tempfile

    shipped = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "kllms_amd", "tunableop", "tunableop_gfx9500.csv")
    if not os.path.exists(shipped):
        return
    tmp = tempfile.mkdtemp(prefix="kllms_tunableop_")
    # TunableOp inserts the device ordinal before ".csv"; provide every ordinal
    for i in range(8):
        shutil.copy(shipped, os.path.join(tmp, f"tunableop_gfx950{i}.csv"))
    try:
        torch.cuda.tunable.enable(True)
        # KLLMS_TUNE=1 re-runs the offline tuning and leaves results in the
        # temp dir (printed) for refreshing kllms_amd/tunableop/.
        tune = os.environ.get("KLLMS_TUNE", "0") == "1"
        torch.cuda.tunable.tuning_enable(tune)
        torch.cuda.tunable.set_filename(os.path.join(tmp, "tunableop_gfx950.csv"), insert_device_ordinal=True)
        torch.cuda.tunable.read_file()
        if tune:
            log(f"[bench] tunableop TUNING, results dir: {tmp}")
            import atexit

            atexit.register(torch.cuda.tunable.write_file)
            atexit.register(lambda: log(f"[bench] tuned results in {tmp}"))
    except Exception as e:
        log(f"[bench] tunableop disabled ({e})")


def dump_outputs(out_dir: str, responses: list) -> None:
    """Write what the last timed step's create()/parse() calls returned, one
    row per request in request order, as float .npy arrays (padding = -1):

      content.npy      float32 [batch, n+1, L]  UTF-8 bytes of every choice's
                       message content (choice 0 = consensus, 1.. = originals)
      content_len.npy  float32 [batch, n+1]     byte length of each content
      likelihoods.npy  float64 [batch, K]       leaf confidences, traversal order
      usage.npy        float64 [batch, 3]       prompt/completion/total tokens

    A step is batch*(n+1) short strings, so the whole dump is far below a MB.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    texts = [[(ch.message.content or "").encode("utf-8") for ch in r.choices]
             for r in responses]
    n_choices = max((len(row) for row in texts), default=0)
    width = max((len(t) for row in texts for t in row), default=0)
    content = np.full((len(texts), n_choices, max(1, width)), -1.0, dtype=np.float32)
    content_len = np.full((len(texts), n_choices), -1.0, dtype=np.float32)
    for i, row in enumerate(texts):
        for j, t in enumerate(row):
            content[i, j, :len(t)] = np.frombuffer(t, dtype=np.uint8)
            content_len[i, j] = len(t)
    leaves = [_likelihood_leaves(r.likelihoods) for r in responses]
    k_max = max((len(l) for l in leaves), default=0)
    lik = np.full((len(leaves), max(1, k_max)), -1.0, dtype=np.float64)
    for i, l in enumerate(leaves):
        lik[i, :len(l)] = l
    usage = np.array(
        [[r.usage.prompt_tokens, r.usage.completion_tokens, r.usage.total_tokens]
         if r.usage is not None else [-1, -1, -1] for r in responses],
        dtype=np.float64).reshape(len(responses), 3)
    np.save(os.path.join(out_dir, "content.npy"), content)
    np.save(os.path.join(out_dir, "content_len.npy"), content_len)
    np.save(os.path.join(out_dir, "likelihoods.npy"), lik)
    np.save(os.path.join(out_dir, "usage.npy"), usage)


@contextlib.contextmanager
def _skip_default_param_init():
    """Setup-time only: the engine overwrites EVERY parameter right after it
    constructs the modules (seeded random init, or a checkpoint), so torch's
    default nn.Embedding / nn.Linear initialisers — ~1 G elements drawn on the
    CPU for the 8B vocab matrices, most of the engine build time — are wasted
    work. Make them no-ops while the engine is built; the weights the timed
    steps run on are unchanged."""
    init = torch.nn.init
    saved = init.normal_, init.kaiming_uniform_
    init.normal_ = init.kaiming_uniform_ = lambda tensor, *a, **kw: tensor
    try:
        yield
    finally:
        init.normal_, init.kaiming_uniform_ = saved


def make_prompt(rank: int, step: int, i: int, prompt_len_tokens: int) -> str:
    # deterministic synthetic prompt of roughly prompt_len_tokens byte-tokens
    seedtxt = f"Request {rank}-{step}-{i}: extract the entities. "
    body = ("The quick brown fox jumps over the lazy dog near the riverbank. " * 200)
    return (seedtxt + body)[:prompt_len_tokens]


def make_schema():
    """Nested Pydantic schema for parse() configs (mirrors the reference's
    Company/Department test shape, README_TESTS.md:63-73). Fields carry
    bounds (maxLength / maxItems / integer ranges) so the byte DFA forces
    structurally complete objects in a bounded token budget — on random-init
    weights an unbounded field would run to the max_tokens cap instead of
    closing (the round-1 schema_valid caveat)."""
    from typing import List

    from pydantic import BaseModel, Field

    class Employee(BaseModel):
        name: str = Field(max_length=16)
        role: str = Field(max_length=12)

    class Department(BaseModel):
        name: str = Field(max_length=16)
        headcount: int = Field(ge=0, le=9999)
        employees: List[Employee] = Field(max_length=2)

    class Company(BaseModel):
        company: str = Field(max_length=20)
        founded: int = Field(ge=0, le=9999)  # range the digit-count DFA bound can honor
        departments: List[Department] = Field(max_length=2)

    return Company


CONFIG_DEFAULTS = {
    # model, n, mode, batch, max_new
    "llama8b": dict(model="llama-3-8b", n=5, mode="create", batch=24, max_new=64),
    "parse16": dict(model="llama-3-8b", n=16, mode="parse", batch=4, max_new=352),
    "mixtral8": dict(model="mixtral-8x7b", n=8, mode="parse", batch=8, max_new=352),
    "llama70b": dict(model="llama-3-70b", n=5, mode="create", batch=4, max_new=64),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=str, default="llama8b", choices=list(CONFIG_DEFAULTS))
    ap.add_argument("--model", type=str, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None, help="consensus requests per step per engine")
    ap.add_argument("--prompt-len", type=int, default=512, help="approx prompt tokens")
    ap.add_argument("--max-new", type=int, default=None, help="decode tokens per stream")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--parallel", type=str, default="dp", choices=["dp", "tp"],
                    help="dp: one engine per rank (weak scaling); tp: ONE engine sharded over all ranks")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write the last step's responses as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline figure (none today)")
    args = ap.parse_args()

    cfgd = CONFIG_DEFAULTS[args.config]
    model = args.model or cfgd["model"]
    n = args.n if args.n is not None else cfgd["n"]
    batch = args.batch if args.batch is not None else cfgd["batch"]
    max_new = args.max_new if args.max_new is not None else cfgd["max_new"]
    mode = cfgd["mode"]

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    on_gpu = torch.cuda.is_available()
    dist = None
    if world_size > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        backend = "nccl" if on_gpu else "gloo"
        dist.init_process_group(backend=backend)
        if on_gpu:
            torch.cuda.set_device(local_rank)

    device = f"cuda:{local_rank}" if on_gpu else "cpu"
    tp_mode = args.parallel == "tp" and world_size > 1

    if on_gpu:
        _enable_tunableop(local_rank)

    from kllms_amd import AsyncKLLMs

    log(f"[bench] building engine: {model} on {device} ({'tp' + str(world_size) if tp_mode else 'tp1'})")
    t_build = time.perf_counter()
    client_kwargs = dict(
        model=model,
        device=device,
        use_hip_graphs=(on_gpu and not args.no_graphs),
        seed=0 if tp_mode else rank,
        default_max_new_tokens=max_new,
        max_seq_len=max(1024, args.prompt_len + max_new + 64),
    )
    if tp_mode:
        client_kwargs["tp_size"] = world_size
    if not on_gpu:
        client_kwargs["max_kv_blocks"] = 4096

    follower = None
    if tp_mode and rank != 0:
        # non-zero TP ranks run the lockstep follower loop; rank 0 drives the
        # public client below and broadcasts every engine action.
        from kllms_amd.engine.api import LocalEngineClient
        from kllms_amd.parallel.serve import TPFollower

        eng_client = LocalEngineClient(**client_kwargs)
        with _skip_default_param_init():
            follower = TPFollower(eng_client.engine)
        log(f"[bench] rank {rank}: follower ready in {time.perf_counter() - t_build:.1f}s")
        follower.run()  # blocks until rank 0 sends stop
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    k = AsyncKLLMs(**client_kwargs)
    eng_client = k.client
    with _skip_default_param_init():
        _ = eng_client.engine  # materialize weights now
    if tp_mode:
        from kllms_amd.parallel.serve import TPCoordinator

        eng_client.scheduler.coordinator = TPCoordinator(eng_client.engine)
    log(f"[bench] engine ready in {time.perf_counter() - t_build:.1f}s")

    schema = make_schema() if mode == "parse" else None
    quality_scores: list = []
    schema_valid = [0, 0]

    async def one_request(step_idx: int, i: int):
        msgs = [{"role": "user", "content": make_prompt(rank, step_idx, i, args.prompt_len)}]
        seed = 10_000 * rank + 100 * step_idx + i
        if mode == "parse":
            res = await k.chat.completions.parse(
                messages=msgs, model=model, response_format=schema,
                n=n, temperature=0.9, max_tokens=max_new, seed=seed,
            )
            for ch in res.choices[1:]:
                schema_valid[1] += 1
                if ch.message.parsed is not None:
                    schema_valid[0] += 1
        else:
            res = await k.chat.completions.create(
                messages=msgs, model=model,
                n=n, temperature=0.8, max_tokens=max_new, seed=seed,
            )
        quality_scores.append(_mean_likelihood(res.likelihoods))
        return res

    prev_stats = {}
    last_responses: list = []

    async def run_step(step_idx: int):
        import time as _t
        t0 = _t.perf_counter()
        last_responses[:] = await asyncio.gather(*(one_request(step_idx, i) for i in range(batch)))
        if os.environ.get("KLLMS_BENCH_VERBOSE"):
            sched = getattr(eng_client, "_scheduler", None)
            cur = dict(sched.stats) if sched else {}
            delta = {k: round(v - prev_stats.get(k, 0), 4) if isinstance(v, float)
                     else v - prev_stats.get(k, 0) for k, v in cur.items()}
            prev_stats.clear()
            prev_stats.update(cur)
            pc = getattr(eng_client.engine, "prefix_cache", None)
            log(f"[bench] step {step_idx}: wall={_t.perf_counter()-t0:.3f}s "
                f"sched_delta={delta} prefix={pc.stats if pc else None}")

    def barrier_sync():
        if dist is not None and not tp_mode:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    async def timed_run():
        # ONE event loop (and one to_thread pool) for the whole bench;
        # asyncio's default executor caps at 32 threads, which would split
        # a >32-request burst into two admission waves — size it to the batch
        import concurrent.futures as _cf
        asyncio.get_running_loop().set_default_executor(
            _cf.ThreadPoolExecutor(max_workers=batch + 8))
        for w in range(args.warmup):
            log(f"[bench] warmup {w + 1}/{args.warmup}")
            await run_step(-1 - w)
        barrier_sync()
        t0 = time.perf_counter()
        for s in range(args.steps):
            await run_step(s)
        barrier_sync()
        return time.perf_counter() - t0

    elapsed = asyncio.run(timed_run())

    # MAX over ranks (DP mode; in TP mode only rank 0 times the job)
    if dist is not None and not tp_mode:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs and rank == 0 and args.steps > 0:
        dump_outputs(args.dump_outputs, last_responses)

    n_engines = 1 if tp_mode else world_size
    total_requests = args.steps * batch * n_engines
    value = total_requests / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        config = {
            "model": model,
            "n": n,
            "mode": mode,
            "global_batch": batch * n_engines,
            "seq_len": args.prompt_len,
            "max_new_tokens": max_new,
            "parallelism": f"tp{world_size}" if tp_mode else f"dp{world_size} tp1",
            "api_path": "AsyncKLLMs.chat.completions." + ("parse" if mode == "parse" else "create"),
            "completions_per_s": round(value * n, 3),
            # amortized (throughput) latency and the user-perceived batch
            # wall time (a sync batch's requests all complete together)
            "consensus_latency_s_per_request": round(elapsed / (args.steps * batch), 4),
            "batch_wall_s": round(ms_per_step / 1000.0, 4),
            "mean_consensus_quality": round(sum(quality_scores) / len(quality_scores), 4) if quality_scores else None,
        }
        if mode == "parse":
            config["schema_valid_fraction"] = round(schema_valid[0] / max(1, schema_valid[1]), 4)
        result = {
            "metric": "end_to_end_consensus_requests_per_s",
            "value": round(value, 4),
            "unit": "req/s",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak" if not tp_mode else "strong",
            "vs_baseline": round(value / REFERENCE_BASELINE[args.config], 3),
            "dtype": "bf16" if on_gpu else "float32",
            "data": "synthetic prompts, random-init weights",
            "config": config,
        }
        print(json.dumps(result), flush=True)

    if tp_mode:
        sched = eng_client.scheduler
        coord = sched.coordinator
        sched.shutdown()      # join the worker thread first …
        coord.stop()          # … then release the followers
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
