"""Device-resident constrained decoding (EngineConfig.device_constraints).

The per-stream DFA state and the constraint tables live on the engine device;
``ops.sample_fsm`` gathers the mask row by state and advances the state by a
byte walk of the chosen token. Everything here runs the CPU path (the same
engine code over ``torch_ref.sample_fsm``) and must match the host-mask path
exactly: tokens, logprobs, top_logprobs, finish reasons and text.
"""

import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from kllms_amd import ops
from kllms_amd.engine.config import EngineConfig
from kllms_amd.engine.constrained import JsonSchemaConstraint
from kllms_amd.engine.engine import GenRequest, LLMEngine
from kllms_amd.engine.sampling import SamplingParams
from kllms_amd.engine.tokenizer import ByteTokenizer, HFTokenizer

BPE_JSON = os.path.join(os.path.dirname(__file__), "data", "bpe_tokenizer.json")

# {name: str max_length 6, age: int 0..120, tag: enum}
PERSON_SCHEMA = {
    "type": "object",
    "properties": {
        "name": {"type": "string", "maxLength": 6},
        "age": {"type": "integer", "minimum": 0, "maximum": 120},
        "tag": {"enum": ["red", "green", "blue"]},
    },
    "required": ["name", "age", "tag"],
}
# a second, differently shaped DFA; after `{"ok":` + `t`/`f` and inside the
# "kind" const every state admits exactly one byte
FLAG_SCHEMA = {
    "type": "object",
    "properties": {
        "ok": {"type": "boolean"},
        "kind": {"const": "fixed-value"},
        "n": {"type": "integer", "minimum": 0, "maximum": 9},
    },
    "required": ["ok", "kind", "n"],
}


def walk_all(tabs, S, V):
    """Vectorised byte walk over DeviceTables held on the CPU: out[s, t] is
    where token t takes state s (stay on EOS, empty tokens and dead walks)."""
    trans = tabs.trans.numpy().view(np.uint16)
    off = tabs.tok_off.numpy()
    by = tabs.tok_bytes.numpy()
    out = np.empty((S, V), dtype=np.int64)
    start = np.arange(S, dtype=np.int64)
    for t in range(V):
        beg, end = int(off[t]), int(off[t + 1])
        if t == tabs.eos_id or end == beg:
            out[:, t] = start
            continue
        cur = start.copy()
        dead = np.zeros(S, dtype=bool)
        for b in by[beg:end]:
            nxt = trans[np.where(dead, 0, cur), b].astype(np.int64)
            dead |= nxt == 0xFFFF
            cur = nxt
        out[:, t] = np.where(dead, start, cur)
    return out


def dense_mask(constraints, states, V):
    """The host path's [B, W] mask (engine._constraint_mask)."""
    W = (V + 31) // 32
    m = torch.full((len(constraints), W), -1, dtype=torch.int32)
    for i, (c, st) in enumerate(zip(constraints, states)):
        if c is not None:
            m[i] = c.allowed_mask(st)
    return m


def sampling_rows(B, device="cpu"):
    """Mixed greedy / tempered rows with top-k and top-p, cycled over B."""
    temps = [0.9, 0.0, 0.9, 0.9, 0.0]
    top_ps = [1.0, 1.0, 0.8, 1.0, 0.9]
    top_ks = [0, 0, 0, 7, 5]
    pick = lambda xs: [xs[i % 5] for i in range(B)]
    return (torch.tensor(pick(temps), dtype=torch.float32, device=device),
            torch.tensor(pick(top_ps), dtype=torch.float32, device=device),
            torch.tensor(pick(top_ks), dtype=torch.int32, device=device),
            torch.tensor([1000 + 17 * i for i in range(B)], dtype=torch.int64, device=device))


def chained_reference(constraints, logits_steps, device="cpu"):
    """`ops.sample` with host-built dense masks + `constraint.advance`: the
    host path, step by step. Returns per-step (tokens, logprobs, states)."""
    B, V = logits_steps[0].shape
    temps, top_ps, top_ks, seeds = sampling_rows(B, device)
    states = [c.init_state() if c is not None else 0 for c in constraints]
    any_c = any(c is not None for c in constraints)
    out = []
    for step, logits in enumerate(logits_steps):
        mask = dense_mask(constraints, states, V).to(device) if any_c else None
        steps = torch.full((B,), step, dtype=torch.int64, device=device)
        toks, lps = ops.sample(logits.to(device), temps, top_ps, top_ks, seeds, steps, mask)
        toks_l = toks.tolist()
        states = [c.advance(st, t) if c is not None else st
                  for c, st, t in zip(constraints, states, toks_l)]
        out.append((toks_l, lps.cpu(), list(states)))
    return out


def chained_fsm(constraints, logits_steps, device="cpu"):
    """The same steps through `ops.sample_fsm`, state chained on the device."""
    B, V = logits_steps[0].shape
    temps, top_ps, top_ks, seeds = sampling_rows(B, device)
    tables = [c.device_tables(device) if c is not None else None for c in constraints]
    fsm_state = torch.tensor([c.init_state() if c is not None else 0 for c in constraints],
                             dtype=torch.int32, device=device)
    tabs = ops.fsm_descriptor(tables, device)
    out = []
    for step, logits in enumerate(logits_steps):
        steps = torch.full((B,), step, dtype=torch.int64, device=device)
        toks, lps = ops.sample_fsm(logits.to(device), temps, top_ps, top_ks, seeds, steps,
                                   fsm_state, tables, tabs)
        out.append((toks.tolist(), lps.cpu(), fsm_state.tolist()))
    return out


def assert_chains_equal(got, want):
    assert len(got) == len(want)
    for step, ((gt, gl, gs), (wt, wl, ws)) in enumerate(zip(got, want)):
        assert gt == wt, f"step {step}: tokens {gt} != {wt}"
        assert gs == ws, f"step {step}: states {gs} != {ws}"
        assert torch.equal(gl, wl), f"step {step}: logprobs {gl} != {wl}"


def five_streams(tok):
    """Two streams on one schema, two on another, one unconstrained."""
    a = JsonSchemaConstraint(PERSON_SCHEMA, tok)
    b = JsonSchemaConstraint(FLAG_SCHEMA, tok)
    return [a, a, b, b, None]


def seeded_logits(B, V, n_steps, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, V, generator=g) * 3.0 for _ in range(n_steps)]


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tokenizer", ["byte512", "bpe571"])
def test_byte_walk_equals_next_state_exhaustively(tokenizer):
    tok = ByteTokenizer(512) if tokenizer == "byte512" else HFTokenizer(BPE_JSON)
    c = JsonSchemaConstraint(PERSON_SCHEMA, tok)
    V = tok.vocab_size
    tabs = c.device_tables("cpu")
    S = c.next_state.shape[0]
    assert (tabs.S, tabs.W, tabs.eos_id) == (S, (V + 31) // 32, tok.eos_id)
    assert tabs.mask.shape == (S, tabs.W) and tabs.mask.dtype == torch.int32
    assert tabs.trans.shape == (S, 256) and tabs.trans.element_size() == 2
    assert tabs.tok_off.shape == (V + 1,) and tabs.tok_off.dtype == torch.int32
    assert tabs.tok_bytes.dtype == torch.uint8
    assert tabs.tok_bytes.numel() == int(tabs.tok_off[-1])
    assert c.device_tables("cpu") is tabs                            # cached per device
    assert JsonSchemaConstraint(PERSON_SCHEMA, tok).device_tables("cpu") is tabs
    # the cases the walk must get right are all present in this vocab
    lens = np.diff(tabs.tok_off.numpy())
    assert (lens == 0).any() and (lens > 1).any()
    assert (c.next_state == 0xFFFF).any()

    want = np.array([[c.advance(s, t) for t in range(V)] for s in range(S)], dtype=np.int64)
    got = walk_all(tabs, S, V)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first mismatch (state, token) = {bad[0]}"
    # DeviceTables.advance is the scalar form of the same walk
    rng = np.random.default_rng(0)
    for s, t in zip(rng.integers(0, S, 300), rng.integers(0, V, 300)):
        assert tabs.advance(int(s), int(t)) == want[s, t]


# ---------------------------------------------------------------------------
# op
# ---------------------------------------------------------------------------

def test_sample_fsm_cpu_matches_host_mask_loop():
    tok = ByteTokenizer(512)
    cons = five_streams(tok)
    logits = seeded_logits(5, 512, 12)
    want = chained_reference(cons, logits)
    got = chained_fsm(cons, logits)
    assert_chains_equal(got, want)
    # the unconstrained stream's state is never touched
    assert all(states[4] == 0 for _, _, states in got)
    # and the constrained ones really moved
    assert got[-1][2][0] != cons[0].init_state()


def test_sample_fsm_out_of_range_state_is_flagged():
    tok = ByteTokenizer(512)
    c = JsonSchemaConstraint(PERSON_SCHEMA, tok)
    tabs = c.device_tables("cpu")
    temps, top_ps, top_ks, seeds = sampling_rows(2)
    st = torch.tensor([tabs.S + 2, c.init_state()], dtype=torch.int32)
    logits = seeded_logits(2, 512, 1)[0]
    toks, _ = ops.sample_fsm(logits, temps, top_ps, top_ks, seeds,
                             torch.zeros(2, dtype=torch.int64), st, [tabs, tabs])
    assert st[0].item() == -1 and st[1].item() >= 0
    assert 0 <= toks[0].item() < 512


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------

def mk_engine(device_constraints, model="tiny-llama", device="cpu", **kw):
    return LLMEngine(EngineConfig(
        model=model, max_kv_blocks=512, use_hip_graphs=kw.pop("use_hip_graphs", False),
        device=device, seed=0, default_max_new_tokens=48, max_seq_len=512,
        enable_prefix_caching=False, device_constraints=device_constraints, **kw))


PARITY_SEED = 11
PARITY_PROMPT = "describe a person"


def parity_requests(eng, seed=PARITY_SEED, max_tokens=48):
    """Two parse-style requests, n=4, temperature 0.9; top_logprobs=3 on the
    second only."""
    ids = eng.tokenizer.encode(eng.tokenizer.apply_chat_template(
        [{"role": "user", "content": PARITY_PROMPT}]))
    mk = lambda schema, s, k: GenRequest(
        prompt_ids=ids, n=4,
        sampling=SamplingParams(temperature=0.9, max_tokens=max_tokens, seed=s,
                                logprobs=True, top_logprobs=k),
        constraint=JsonSchemaConstraint(schema, eng.tokenizer))
    return [mk(PERSON_SCHEMA, seed, 0), mk(FLAG_SCHEMA, seed + 1, 3)]


def flatten(outputs):
    return [(s.token_ids, s.logprobs, s.top_logprobs, s.finish_reason, s.text)
            for o in outputs for s in o.streams]


def assert_parity_preconditions(host):
    """The comparison means something only if streams ran a while and left
    the batch at different steps (so the batch state was rebuilt)."""
    lens = [len(toks) for toks, *_ in host]
    assert min(lens) >= 8, lens
    assert len(set(lens)) > 1, lens


def assert_outputs_identical(dev, host):
    assert len(dev) == len(host)
    for i, (d, h) in enumerate(zip(dev, host)):
        for what, a, b in zip(("token_ids", "logprobs", "top_logprobs", "finish_reason", "text"), d, h):
            assert a == b, f"stream {i}: {what} differs: {a!r} != {b!r}"


def count_sample_fsm_calls(monkeypatch):
    """Wrap ops.sample_fsm with a call counter; returns the one-element list
    that holds the count."""
    calls = [0]
    real = ops.sample_fsm

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "sample_fsm", counted)
    return calls


def test_engine_parity_with_host_path(monkeypatch):
    monkeypatch.delenv("KLLMS_DEVICE_CONSTRAINTS", raising=False)
    eng_h, eng_d = mk_engine(False), mk_engine(True)
    host = flatten(eng_h.generate(parity_requests(eng_h)))
    assert_parity_preconditions(host)
    assert any(tl for _, _, tl, _, _ in host)        # top_logprobs were produced

    fsm_calls = count_sample_fsm_calls(monkeypatch)
    monkeypatch.setattr(eng_d, "_constraint_mask",
                        lambda s: pytest.fail("host mask built on the device path"))
    dev = flatten(eng_d.generate(parity_requests(eng_d)))
    assert_outputs_identical(dev, host)
    assert fsm_calls[0] >= 8
    assert eng_d.kv.allocator.num_free == eng_h.kv.allocator.num_free


def test_unconstrained_batch_takes_the_plain_path(monkeypatch):
    monkeypatch.delenv("KLLMS_DEVICE_CONSTRAINTS", raising=False)
    eng = mk_engine(True)
    monkeypatch.setattr(ops, "sample_fsm", lambda *a, **k: pytest.fail("sample_fsm on an unconstrained batch"))
    out = eng.generate([GenRequest(prompt_ids=[1, 2, 3], n=2,
                                   sampling=SamplingParams(temperature=0.0, max_tokens=6))])[0]
    assert out.streams[0].token_ids == out.streams[1].token_ids


def test_scheduler_parity_with_unconstrained_neighbour(monkeypatch):
    from kllms_amd.engine.scheduler import BatchScheduler

    monkeypatch.delenv("KLLMS_DEVICE_CONSTRAINTS", raising=False)

    def run(device_constraints, spy=None):
        eng = mk_engine(device_constraints)
        if spy is not None:
            real = ops.sample_fsm

            def wrapped(*a, **k):
                spy.append([t is None for t in a[7]])
                return real(*a, **k)

            monkeypatch.setattr(ops, "sample_fsm", wrapped)
        con, _ = parity_requests(eng)
        free = GenRequest(prompt_ids=[5, 6, 7, 8], n=2,
                          sampling=SamplingParams(temperature=0.9, max_tokens=40, seed=3,
                                                  logprobs=True))
        sched = BatchScheduler(eng, admit_wait_s=0.05)
        futs = [sched.submit(con), sched.submit(free)]
        outs = [f.result(timeout=120) for f in futs]
        sched.shutdown()
        return flatten(outs)

    host = run(False)
    spy = []
    dev = run(True, spy)
    assert_outputs_identical(dev, host)
    # some step sampled constrained and unconstrained rows together
    assert any(any(row) and not all(row) for row in spy), spy[:4]


TP_PORT = 29851


def _tp_worker(rank, world, q, device_constraints):
    import torch.distributed as dist

    os.environ.pop("KLLMS_DEVICE_CONSTRAINTS", None)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(TP_PORT + int(device_constraints))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pydantic import BaseModel, Field

        from kllms_amd.engine.api import LocalEngineClient
        from kllms_amd.parallel.serve import TPCoordinator, TPFollower

        client = LocalEngineClient(model="tiny-llama", tp_size=world, max_kv_blocks=512,
                                   use_hip_graphs=False, device="cpu", seed=0,
                                   default_max_new_tokens=8, max_seq_len=512,
                                   device_constraints=device_constraints)
        eng = client.engine
        assert eng.device_constraints is device_constraints
        if rank != 0:
            TPFollower(eng).run()
            q.put((rank, "follower-done"))
            return
        sched = client.scheduler
        coord = TPCoordinator(eng)
        sched.coordinator = coord

        class Person(BaseModel):
            name: str = Field(max_length=6)
            age: int = Field(ge=0, le=120)

        r = client.chat_completions_parse(
            True, messages=[{"role": "user", "content": "describe a person"}],
            response_format=Person, n=4, temperature=0.9, max_tokens=40, seed=7,
            logprobs=True, top_logprobs=2)
        sched.shutdown()
        coord.stop()
        q.put((rank, [(c.message.content, c.finish_reason,
                       [(t.token, t.logprob, [(a.token, a.logprob) for a in t.top_logprobs])
                        for t in c.logprobs.content])
                      for c in r.choices]))
    finally:
        dist.destroy_process_group()


def _run_tp(device_constraints, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, world, q, device_constraints))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, payload = q.get(timeout=240)
        results[rank] = payload
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert results[1] == "follower-done"
    return results[0]


@pytest.mark.timeout(600)
def test_tp2_parity_with_host_path():
    host = _run_tp(False)
    dev = _run_tp(True)
    assert len(host) == 4
    assert all(len(toks) >= 8 for _, _, toks in host)
    assert dev == host


def test_env_override_and_client_kwarg(monkeypatch):
    from kllms_amd import KLLMs

    monkeypatch.delenv("KLLMS_DEVICE_CONSTRAINTS", raising=False)
    assert EngineConfig().device_constraints is False
    k = KLLMs(model="tiny-llama", device="cpu", max_kv_blocks=64, device_constraints=True)
    cfg = k._client.config
    assert isinstance(cfg, EngineConfig) and cfg.device_constraints is True
    assert LLMEngine(cfg).device_constraints is True
    assert mk_engine(False, max_batch_size=8).device_constraints is False

    monkeypatch.setenv("KLLMS_DEVICE_CONSTRAINTS", "1")
    eng = mk_engine(False)
    assert eng.device_constraints is True and eng.config.device_constraints is False
    monkeypatch.setenv("KLLMS_DEVICE_CONSTRAINTS", "0")
    eng = mk_engine(True)
    assert eng.device_constraints is False
    # read once, at construction
    monkeypatch.setenv("KLLMS_DEVICE_CONSTRAINTS", "1")
    assert eng.device_constraints is False
    monkeypatch.setenv("KLLMS_DEVICE_CONSTRAINTS", "yes")
    with pytest.raises(ValueError):
        mk_engine(False)


def test_corrupted_device_state_raises_and_frees_kv(monkeypatch):
    monkeypatch.delenv("KLLMS_DEVICE_CONSTRAINTS", raising=False)
    eng = mk_engine(True)
    free_before = eng.kv.allocator.num_free
    real = ops.sample_fsm
    n_calls = [0]

    def corrupting(*a, **k):
        out = real(*a, **k)
        n_calls[0] += 1
        if n_calls[0] == 4:              # a decode step, well past the first token
            fsm_state, tables = a[6], a[7]
            fsm_state[1] = (int(fsm_state[1]) + 1) % tables[1].S   # wrong, in range
        return out

    monkeypatch.setattr(ops, "sample_fsm", corrupting)
    with pytest.raises(RuntimeError, match=r"diverged.*stream 1.*device state \d+, host state \d+"):
        eng.generate(parity_requests(eng))
    assert n_calls[0] == 4
    assert eng.kv.allocator.num_free == free_before
    # the engine is still usable
    monkeypatch.setattr(ops, "sample_fsm", real)
    out = eng.generate(parity_requests(eng))
    assert all(s.token_ids for o in out for s in o.streams)
