"""Shared-prefix (cascade) decode attention on the GPU: the MFMA group kernel
against the fp32 oracle, proof that the shared path is really taken, the fp8
cache variant, null metadata, and the engine / hipGraph integration.

Run on an MI355X box: python -m pytest tests/test_gpu_shared_prefix.py -m gpu -q
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops
from kllms_amd.ops import torch_ref

import shared_prefix_cases as cases

DEV = "cuda:0"
BS = cases.BS

_cache = {}


def case(gqa):
    """The batch, its metadata, the fp32 oracle (computed once on the CPU
    from the true tables, shared and never modified) and device copies."""
    if gqa not in _cache:
        b = cases.build_batch(gqa)
        tiles = cases.build_tiles(b)
        oracle = torch_ref.attn_decode_paged(
            b["q"], b["kc"], b["vc"], b["bt"], b["lens"], b["scale"])
        dev = {k: b[k].to(DEV) for k in ("q", "kc", "vc", "bt", "lens")}
        _cache[gqa] = (b, tiles, oracle.to(DEV), dev)
    return _cache[gqa]


@pytest.mark.parametrize("gqa", [1, 2, 4, 8])
def test_kernel_vs_oracle(gqa):
    b, tiles, oracle, d = case(gqa)
    assert tiles.n_tiles == (4 if gqa == 8 else 2)
    shared = tiles.to_tensors(DEV)
    out = ops.attn_decode_paged(d["q"], d["kc"], d["vc"], d["bt"], d["lens"], b["scale"],
                                shared=shared)
    cases.assert_close_bf16(out, oracle, rtol=3e-2, atol=3e-2, msg=f"cascade gqa={gqa}")


@pytest.mark.parametrize("gqa", [1, 2, 4, 8])
def test_shared_path_is_really_used(gqa):
    """Every cascaded member but its tile's first gets the block-table entries
    of its skipped chunks pointed at junk blocks (finite, constant 100). The
    output still matches the oracle of the TRUE tables only if the per-stream
    kernel skipped those chunks and the group kernel supplied them."""
    b, tiles, oracle, d = case(gqa)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    junk = list(range(cases.NB - cases.JUNK_BLOCKS, cases.NB))
    kc[junk] = 100.0
    vc[junk] = 100.0
    bt = d["bt"].clone()
    repointed = 0
    for rows, nmem, S in zip(tiles.tile_rows, tiles.tile_nmembers, tiles.tile_chunks):
        for r in rows[1:nmem]:
            nblk = S * 256 // BS
            bt[r, :nblk] = torch.tensor([junk[j % len(junk)] for j in range(nblk)],
                                        dtype=torch.int32, device=DEV)
            repointed += 1
    assert repointed == (12 if gqa == 8 else 5)   # every member but each tile's first
    shared = tiles.to_tensors(DEV)
    out = ops.attn_decode_paged(d["q"], kc, vc, bt, d["lens"], b["scale"], shared=shared)
    cases.assert_close_bf16(out, oracle, rtol=3e-2, atol=3e-2, msg=f"junk tables gqa={gqa}")
    # and the junk is visible to the per-stream path alone
    plain = ops.attn_decode_paged(d["q"], kc, vc, bt, d["lens"], b["scale"])
    assert (plain.float() - oracle.float()).abs().max().item() > 1.0


def test_fp8_cache():
    b, tiles, _, d = case(4)
    NB, KVH, D = cases.NB, cases.KVH, cases.D
    kc8 = torch.zeros(NB, KVH, BS, D, dtype=torch.float8_e4m3fn, device=DEV)
    vc8 = torch.zeros_like(kc8)
    ks = torch.ones(NB, KVH, BS, device=DEV)
    vs = torch.ones_like(ks)
    # quantise the bf16 caches on the device, one (token, head) row per slot,
    # with per-row scales of very different sizes
    k_rows = d["kc"].permute(0, 2, 1, 3).reshape(NB * BS, KVH, D).clone()
    v_rows = d["vc"].permute(0, 2, 1, 3).reshape(NB * BS, KVH, D).clone()
    k_rows[::3] *= 4.0
    v_rows[1::5] *= 0.25
    ops.store_kv(k_rows, v_rows, kc8, vc8, torch.arange(NB * BS, device=DEV), ks, vs)
    ref = torch_ref.attn_decode_paged(d["q"], kc8, vc8, d["bt"], d["lens"], b["scale"], ks, vs)
    shared = tiles.to_tensors(DEV)
    out = ops.attn_decode_paged(d["q"], kc8, vc8, d["bt"], d["lens"], b["scale"], ks, vs,
                                shared=shared)
    cases.assert_close_bf16(out, ref, rtol=4e-2, atol=4e-2, msg="fp8 cascade")


@pytest.mark.parametrize("fp8", [False, True])
def test_null_metadata_is_todays_output(fp8):
    from kllms_amd import _C
    from kllms_amd.engine.shared_prefix import SharedPrefixTiles

    b, _, _, d = case(4)
    kc, vc = d["kc"], d["vc"]
    ks = vs = torch.empty(0, dtype=torch.float32, device=DEV)
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        ks = torch.rand(cases.NB, cases.KVH, BS, device=DEV) + 0.5
        vs = torch.rand(cases.NB, cases.KVH, BS, device=DEV) + 0.5
    today = torch.empty_like(d["q"])
    _C.attn_decode_paged(today, d["q"], kc, vc, d["bt"], d["lens"], b["scale"], ks, vs)
    sc = (ks, vs) if fp8 else (None, None)
    none = ops.attn_decode_paged(d["q"], kc, vc, d["bt"], d["lens"], b["scale"], *sc, shared=None)
    assert torch.equal(none, today)
    B = d["q"].shape[0]
    empty = SharedPrefixTiles(skip=[0] * B).to_tensors(DEV)
    assert empty.n_tiles == 0
    zero = ops.attn_decode_paged(d["q"], kc, vc, d["bt"], d["lens"], b["scale"], *sc, shared=empty)
    assert torch.equal(zero, today)
    # tiles present but all empty (a replayed graph with no group this step)
    idle = SharedPrefixTiles(skip=[0] * B, tile_rows=[[-1] * 64] * 3, tile_nmembers=[0] * 3,
                             tile_chunks=[0] * 3).to_tensors(DEV)
    out = ops.attn_decode_paged(d["q"], kc, vc, d["bt"], d["lens"], b["scale"], *sc, shared=idle)
    assert torch.equal(out, today)


def _engine(flag, **kw):
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    cfg = dict(model="mid-llama", max_kv_blocks=1024, use_hip_graphs=False, max_seq_len=2048,
               seed=11, enable_prefix_caching=False, shared_prefix_attention=flag)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _forked_state(eng, prompt, n):
    from kllms_amd.engine.engine import GenRequest, _DecodeBatchState
    from kllms_amd.engine.sampling import SamplingParams

    parents, streams = [], []
    eng.begin_requests([GenRequest(prompt_ids=prompt, n=n,
                                   sampling=SamplingParams(temperature=0.0, max_tokens=8))],
                       parents, streams)
    return _DecodeBatchState(eng, streams), streams


def test_engine_vs_flag_off(monkeypatch):
    from kllms_amd.engine.engine import GenRequest
    from kllms_amd.engine.sampling import SamplingParams
    from kllms_amd.models.llama import ForwardBatch

    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = _engine(True)
    prompt = [(i * 13) % 1900 + 1 for i in range(600)]
    out = eng.generate([GenRequest(prompt_ids=prompt, n=5,
                                   sampling=SamplingParams(temperature=0.0, max_tokens=8))])[0]
    assert eng.last_timings["shared_prefix_rows"] > 0
    toks = out.streams[0].token_ids
    assert all(s.token_ids == toks for s in out.streams)   # greedy streams agree
    assert all(np.isfinite(lp) for s in out.streams for lp in s.logprobs)

    # teacher-forced check: one prefill over prompt + decoded prefix
    full = prompt + toks[:-1]
    seq = eng.kv.alloc_sequence(len(full))
    batch = ForwardBatch(
        mode="prefill",
        positions=torch.arange(len(full), device=DEV),
        slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
        kv_caches=eng.kv.layer_caches(),
        cu_seqlens=torch.tensor([0, len(full)], dtype=torch.int32, device=DEV),
    )
    with torch.inference_mode():
        logits = eng.model.forward_prefill(torch.tensor(full, device=DEV), batch)
    eng.kv.free_sequence(seq)
    assert int(logits[0].argmax()) == toks[-1], "cascade decode diverged from prefill"

    # one decode step, flag on vs off, identical inputs
    state, streams = _forked_state(eng, prompt, 5)
    assert state.rows_cascaded == 5 and state.n_tiles == 1
    assert state.shared.tile_chunks.tolist() == [2]        # 37 full blocks = 592 keys
    on, off = cases.decode_step_batches(eng, state)
    with torch.inference_mode():
        l_on = eng.model.forward_decode(state.ids, on)
        l_off = eng.model.forward_decode(state.ids, off)
    cases.assert_logits_close(l_on, l_off, "cascade vs per-stream logits")
    for s in streams:
        eng.kv.free_sequence(s.seq)


def test_hip_graph(monkeypatch):
    from kllms_amd.engine.engine import GenRequest
    from kllms_amd.engine.sampling import SamplingParams

    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = _engine(True, use_hip_graphs=True, hip_graph_batch_sizes=[1, 2, 4, 8])
    runner = eng._graph_runner
    assert runner is not None
    long_p = [(i * 13) % 1900 + 1 for i in range(300)]
    short_p = [(i * 5) % 1900 + 1 for i in range(40)]

    out = eng.generate([GenRequest(prompt_ids=long_p, n=3,
                                   sampling=SamplingParams(temperature=0.0, max_tokens=16))])[0]
    assert runner._enabled, "hipGraph capture was disabled"
    assert 4 in runner.graphs
    assert eng.last_timings["shared_prefix_rows"] == 3
    assert all(np.isfinite(lp) for s in out.streams for lp in s.logprobs)

    # one step, graph replay against eager, same metadata
    state, streams = _forked_state(eng, long_p, 3)
    assert state.shared is not None and state.shared.tile_chunks.tolist() == [1]
    on, _ = cases.decode_step_batches(eng, state)
    with torch.inference_mode():
        l_graph = runner.run(state.ids, on)
        l_eager = eng.model.forward_decode(state.ids, on)
    assert runner._enabled
    cases.assert_logits_close(l_graph, l_eager, "graph vs eager with cascade")
    for s in streams:
        eng.kv.free_sequence(s.seq)

    # a 40-token prompt has no tiles: the same captured graphs replay as the
    # plain path and match a flag-off engine
    out = eng.generate([GenRequest(prompt_ids=short_p, n=3,
                                   sampling=SamplingParams(temperature=0.0, max_tokens=16))])[0]
    assert runner._enabled and eng.last_timings["shared_prefix_rows"] == 0
    assert all(np.isfinite(lp) for s in out.streams for lp in s.logprobs)
    state, streams = _forked_state(eng, short_p, 3)
    assert state.shared is None
    on, _ = cases.decode_step_batches(eng, state)
    with torch.inference_mode():
        l_graph = runner.run(state.ids, on)
    assert runner._enabled

    eng_off = _engine(False)
    state_off, streams_off = _forked_state(eng_off, short_p, 3)
    assert torch.equal(state_off.ids, state.ids)
    _, off = cases.decode_step_batches(eng_off, state_off)
    with torch.inference_mode():
        l_off = eng_off.model.forward_decode(state_off.ids, off)
    cases.assert_logits_close(l_graph, l_off, "zero-tile graph replay vs flag-off engine")
    for s in streams:
        eng.kv.free_sequence(s.seq)
    for s in streams_off:
        eng_off.kv.free_sequence(s.seq)
