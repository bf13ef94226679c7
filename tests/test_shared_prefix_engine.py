"""Shared-prefix cascade decode attention through the engine (CPU,
tiny-llama): the metadata reaches the attention op, generation survives
groups shrinking mid-run, and the flag / env override are honoured."""

import math

import pytest
import torch

from kllms_amd.engine.config import EngineConfig
from kllms_amd.engine.engine import GenRequest, LLMEngine, _DecodeBatchState
from kllms_amd.engine.sampling import SamplingParams

import shared_prefix_cases as cases


def mk_engine(flag, **kw):
    return LLMEngine(EngineConfig(
        model="tiny-llama", device="cpu", max_kv_blocks=256, max_seq_len=512, seed=4,
        enable_prefix_caching=False, shared_prefix_attention=flag, **kw))


def prompt(n, salt=0):
    return [(i * 7 + salt) % 200 + 1 for i in range(n)]


def test_decode_step_with_and_without_shared(monkeypatch):
    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = mk_engine(True)
    parents, streams = [], []
    eng.begin_requests(
        [GenRequest(prompt_ids=prompt(300), n=4,
                    sampling=SamplingParams(temperature=0.0, max_tokens=4)),
         GenRequest(prompt_ids=prompt(40, 3), n=2,
                    sampling=SamplingParams(temperature=0.0, max_tokens=4))],
        parents, streams)
    assert [s.fork_id for s in streams] == [0, 0, 0, 0, 1, 1]
    state = _DecodeBatchState(eng, streams)
    # 300 tokens = 18 full blocks = 288 shared keys: one chunk; 40 tokens: none
    assert state.shared is not None and state.n_tiles == 1 and state.rows_cascaded == 4
    assert state.shared.skip_chunks.tolist() == [1, 1, 1, 1, 0, 0]
    on, off = cases.decode_step_batches(eng, state)
    with torch.inference_mode():
        l_on = eng.model.forward_decode(state.ids, on)
        l_off = eng.model.forward_decode(state.ids, off)
    assert torch.isfinite(l_on).all()
    cases.assert_logits_close(l_on, l_off, "cascade vs per-stream decode step")
    for s in streams:
        eng.kv.free_sequence(s.seq)


def test_generate_with_shrinking_groups(monkeypatch):
    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = mk_engine(True)
    calls = []
    from kllms_amd.ops import torch_ref

    real = torch_ref.attn_decode_paged_shared
    monkeypatch.setattr(torch_ref, "attn_decode_paged_shared",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = eng.generate([
        GenRequest(prompt_ids=prompt(300), n=4,
                   sampling=SamplingParams(temperature=1.0, max_tokens=3, seed=1)),
        GenRequest(prompt_ids=prompt(310, 5), n=4,
                   sampling=SamplingParams(temperature=1.0, max_tokens=6, seed=2)),
    ])
    assert [len(o.streams) for o in outs] == [4, 4]
    for o in outs:
        for s in o.streams:
            assert len(s.token_ids) > 0 and s.finish_reason in ("stop", "length")
            assert all(math.isfinite(lp) for lp in s.logprobs)
    assert eng.last_timings["shared_prefix_rows"] > 0
    assert calls, "the cascade path was never taken"
    # every block went back to the pool
    assert eng.kv.allocator.num_free == eng.kv.num_blocks


def test_flag_off_builds_no_metadata(monkeypatch):
    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = mk_engine(False)
    from kllms_amd.ops import torch_ref

    monkeypatch.setattr(torch_ref, "attn_decode_paged_shared",
                        lambda *a, **k: pytest.fail("cascade path with the flag off"))
    eng.generate([GenRequest(prompt_ids=prompt(300), n=3,
                             sampling=SamplingParams(temperature=0.0, max_tokens=3))])
    assert eng.last_timings["shared_prefix_rows"] == 0


def test_min_keys_threshold(monkeypatch):
    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    eng = mk_engine(True, shared_prefix_min_keys=512)
    eng.generate([GenRequest(prompt_ids=prompt(300), n=3,
                             sampling=SamplingParams(temperature=0.0, max_tokens=2))])
    assert eng.last_timings["shared_prefix_rows"] == 0


def test_config_flag_env_override_and_client_kwarg(monkeypatch):
    from kllms_amd import KLLMs

    monkeypatch.delenv("KLLMS_SHARED_PREFIX_ATTN", raising=False)
    assert EngineConfig().shared_prefix_attention is False
    assert EngineConfig().shared_prefix_min_keys == 256
    k = KLLMs(model="tiny-llama", device="cpu", max_kv_blocks=64, shared_prefix_attention=True)
    cfg = k._client.config
    assert isinstance(cfg, EngineConfig) and cfg.shared_prefix_attention is True
    assert LLMEngine(cfg).shared_prefix_attention is True
    assert mk_engine(False).shared_prefix_attention is False

    monkeypatch.setenv("KLLMS_SHARED_PREFIX_ATTN", "1")
    eng = mk_engine(False)
    assert eng.shared_prefix_attention is True and eng.config.shared_prefix_attention is False
    monkeypatch.setenv("KLLMS_SHARED_PREFIX_ATTN", "0")
    assert mk_engine(True).shared_prefix_attention is False
    # read once, at construction
    monkeypatch.setenv("KLLMS_SHARED_PREFIX_ATTN", "1")
    assert eng.shared_prefix_attention is True
    monkeypatch.setenv("KLLMS_SHARED_PREFIX_ATTN", "yes")
    with pytest.raises(ValueError, match="KLLMS_SHARED_PREFIX_ATTN"):
        mk_engine(False)
