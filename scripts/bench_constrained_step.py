#!/usr/bin/env python3
"""A/B: what the per-step host constraint-mask path costs the sampler.

Times N `LLMEngine._sample_state` steps at the parse16 benchmark's sampling
shape (B = 64 streams, V = 128256 byte vocab, bench.make_schema()'s DFA) with
the constraint state on the host (one [B, ceil(V/32)] mask assembled and
uploaded per step) and on the device (EngineConfig.device_constraints: no
upload). Only the sampler runs: the logits are one seeded random [B, V]
tensor, and the model behind the engine is a one-layer toy with the real
vocab width. Order: host, device, host, device; the spread between repeats of
one mode is printed next to the difference between the modes.

Needs a GPU. Usage: python scripts/bench_constrained_step.py [--steps 200]
Prints one JSON line.
"""

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B_REQ, N_PER_REQ, V = 4, 16, 128256


def build_engine(model_dir: str, device_constraints: bool):
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    os.environ.pop("KLLMS_DEVICE_CONSTRAINTS", None)
    return LLMEngine(EngineConfig(
        model=model_dir, device="cuda:0", use_hip_graphs=False, seed=0,
        max_kv_blocks=2048, max_seq_len=2048, default_max_new_tokens=1024,
        enable_prefix_caching=False, device_constraints=device_constraints))


def time_mode(eng, schema, logits, n_steps: int, warmup: int):
    """ms per _sample_state step over n_steps, one synchronise at the end."""
    from kllms_amd.engine.constrained import JsonSchemaConstraint
    from kllms_amd.engine.engine import GenRequest, _DecodeBatchState
    from kllms_amd.engine.sampling import SamplingParams

    con = JsonSchemaConstraint(schema, eng.tokenizer)
    reqs = [GenRequest(prompt_ids=eng.tokenizer.encode(f"record {i}"), n=N_PER_REQ,
                       sampling=SamplingParams(temperature=0.9, max_tokens=1024, seed=100 + i),
                       constraint=con) for i in range(B_REQ)]
    parents, streams = [], []
    with torch.inference_mode():
        eng.begin_requests(reqs, parents, streams)
        state = _DecodeBatchState(eng, streams)
        assert (state.fsm_state is not None) == eng.device_constraints
        for _ in range(warmup):
            eng._sample_state(state, logits)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            eng._sample_state(state, logits)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    tokens = [list(s.out.token_ids) for s in streams]
    for s in streams:
        eng.kv.free_sequence(s.seq)
    return dt * 1000.0 / n_steps, tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_constrained_step.py needs a GPU")

    import bench

    schema = bench.make_schema().model_json_schema()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump({"model_type": "llama", "vocab_size": V, "hidden_size": 128,
                       "intermediate_size": 256, "num_hidden_layers": 1,
                       "num_attention_heads": 1, "num_key_value_heads": 1,
                       "max_position_embeddings": 2048}, f)
        engines = {"host": build_engine(d, False), "device": build_engine(d, True)}

    B = B_REQ * N_PER_REQ
    g = torch.Generator(device="cuda:0").manual_seed(0)
    logits = torch.randn(B, V, generator=g, device="cuda:0") * 3.0

    from kllms_amd.engine.constrained import JsonSchemaConstraint

    n_states = int(JsonSchemaConstraint(schema, engines["host"].tokenizer).trans.shape[0])
    ms = {"host": [], "device": []}
    toks = {}
    for mode in ("host", "device", "host", "device"):
        t, tk = time_mode(engines[mode], schema, logits, args.steps, args.warmup)
        ms[mode].append(round(t, 4))
        assert toks.setdefault(mode, tk) == tk, f"{mode} path is not reproducible"
    assert toks["host"] == toks["device"], "host and device paths sampled different tokens"

    W = (V + 31) // 32
    mean = lambda xs: sum(xs) / len(xs)
    print(json.dumps({
        "probe": "constrained_step", "B": B, "V": V, "steps": args.steps,
        "dfa_states": n_states,
        "ms_per_step": ms,
        "spread_ms": {m: round(max(v) - min(v), 4) for m, v in ms.items()},
        "host_minus_device_ms": round(mean(ms["host"]) - mean(ms["device"]), 4),
        "h2d_bytes_per_step": {"host": B * W * 4, "device": 0},
        "d2h_bytes_per_step": {"host": 2 * B * 8, "device": 3 * B * 8},
        "tokens_identical": True,
    }))


if __name__ == "__main__":
    main()
