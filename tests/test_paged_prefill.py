"""Paged (append / extend) prefill attention on the CPU: the tile metadata, the
torch reference against the float64 oracle, proof that the bound rejects every
mutant, and the engine with ``paged_prefill_attention`` on against it off.

On the CPU ``ops.attn_prefill_paged`` is ``torch_ref.attn_prefill_paged``,
defined as ``attn_decode_paged`` over the per-token rows, so the engine must
give the SAME bits with the flag on as with it off; the HIP kernel is held to
the oracle in ``test_gpu_paged_prefill.py``.
"""

import pytest
import torch

from kllms_amd import ops
from kllms_amd.engine.config import EngineConfig
from kllms_amd.engine.engine import GenRequest, LLMEngine
from kllms_amd.engine.sampling import SamplingParams
from kllms_amd.engine.scheduler import BatchScheduler
from kllms_amd.ops import torch_ref

import kernel_oracles as ko
import paged_prefill_cases as pc

PARAMS, IDS = pc.all_params()


# --- metadata -------------------------------------------------------------------

def _tiles_of(meta):
    """[(sequence, first row)] of every non-idle workgroup slot."""
    seqs = meta.grp_seq.tolist()
    qpos = meta.grp_qpos0.tolist()
    assert len(qpos) == 8 * len(seqs)
    return [(seqs[g], qpos[8 * g + w]) for g in range(len(seqs)) for w in range(8)
            if qpos[8 * g + w] != -1]


@pytest.mark.parametrize("tpg", [None, 1, 3, 8])
@pytest.mark.parametrize("seqs", pc.CASES, ids=pc.case_id)
def test_metadata_tiles_every_row_once(seqs, tpg):
    BS = 16
    lens = [n for _, n in seqs]
    starts = [s for s, _ in seqs]
    blocks, nxt = [], 5
    for s, n in seqs:
        nb = (s + n + BS - 1) // BS
        blocks.append(list(range(nxt, nxt + nb)))
        nxt += nb
    meta = ops.build_paged_prefill(lens, starts, blocks, "cpu", BS, tiles_per_group=tpg)
    for t in (meta.cu_q, meta.q_start, meta.block_tables, meta.grp_seq, meta.grp_qpos0):
        assert t.dtype == torch.int32
    want = [(s, r) for s, n in enumerate(lens) for r in range(0, n, 32)]
    assert sorted(_tiles_of(meta)) == want, "every (sequence, 32-row tile) exactly once"
    assert all(q == -1 or q >= 0 for q in meta.grp_qpos0.tolist())
    # rows, starts and tables round-trip
    cu = meta.cu_q.tolist()
    assert [cu[i + 1] - cu[i] for i in range(len(lens))] == lens and cu[0] == 0
    assert meta.q_start.tolist() == starts
    assert meta.n_seq == len(seqs) and meta.n_groups == len(meta.grp_seq)
    assert meta.block_tables.shape == (len(seqs), max(len(b) for b in blocks))
    for s, b in enumerate(blocks):
        assert meta.block_tables[s, : len(b)].tolist() == b
    if tpg is not None:
        per_group = [sum(q != -1 for q in meta.grp_qpos0.tolist()[8 * g: 8 * g + 8])
                     for g in range(meta.n_groups)]
        assert max(per_group) <= tpg


def test_metadata_rejects_overflow_and_bad_input():
    ops.build_paged_prefill([16], [16], [[1, 2]], "cpu", 16)
    with pytest.raises(ValueError, match="exceeds"):
        ops.build_paged_prefill([17], [16], [[1, 2]], "cpu", 16)
    with pytest.raises(ValueError, match="exceeds"):
        ops.build_paged_prefill([4, 4], [0, 30], [[1], [2, 3]], "cpu", 16)
    with pytest.raises(ValueError):
        ops.build_paged_prefill([0], [0], [[1]], "cpu", 16)
    with pytest.raises(ValueError):
        ops.build_paged_prefill([1], [-1], [[1]], "cpu", 16)
    with pytest.raises(ValueError):
        ops.build_paged_prefill([1, 1], [0], [[1]], "cpu", 16)
    with pytest.raises(ValueError):
        ops.build_paged_prefill([1], [0], [[1]], "cpu", 16, tiles_per_group=9)


# --- oracle and reference -------------------------------------------------------

def test_oracle_matches_decode_oracle_on_expanded_rows():
    """The oracle against ``kernel_oracles.attn_decode`` over the per-token
    rows (table row repeated, context start+i+1), bf16 and fp8."""
    for fp8 in (False, True):
        case = pc.make_case([(16, 33), (0, 1)], 8, 2, 16, fp8)
        bt, lens = pc.expanded_rows(case)
        e, a = pc.oracle(case)
        e2, a2 = ko.attn_decode(case["q"], case["kc"], case["vc"], bt, lens, case["scale"],
                                case.get("ks"), case.get("vs"))
        assert torch.allclose(e, e2, rtol=1e-12, atol=1e-13)
        assert torch.allclose(a, a2, rtol=1e-12, atol=1e-13)


def _meta(case, **kw):
    return ops.build_paged_prefill(case["lens"], case["starts"], case["block_lists"], "cpu",
                                   case["BS"], **kw)


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8", PARAMS, ids=IDS)
def test_reference_within_bound(seqs, H, KVH, BS, fp8):
    """torch_ref (fp32, unrounded K/V) against the float64 oracle taken without
    the bf16 rounding of dequantised K/V; and the emulation of a correct
    MFMA kernel stays inside the same bound."""
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    e, a = pc.case_oracle(case)
    out = ops.attn_prefill_paged(case["q"], case["kc"], case["vc"], _meta(case), case["scale"],
                                 case.get("ks"), case.get("vs"))
    ratio, idx = pc.check(out, e, a, pc.C_MFMA)
    msg = ko.describe("torch_ref.attn_prefill_paged", case["name"], ratio, idx,
                      ("token", "head", "dim"), pc.where(case)(idx))
    assert ratio <= 1.0, msg
    emu = pc.oracle(case, p_bf16=True, round_kv_bf16=True)[0]
    e_r, a_r = pc.case_oracle(case, round_kv_bf16=True)
    ratio, idx = pc.check(emu, e_r, a_r, pc.C_MFMA)
    assert ratio <= 1.0, ko.describe("bf16-p emulation", case["name"], ratio, idx,
                                     ("token", "head", "dim"))


def test_reference_is_decode_over_rows():
    case = pc.make_case(pc.MULTI, 8, 2, 16, True)
    bt, lens = pc.expanded_rows(case)
    want = torch_ref.attn_decode_paged(case["q"], case["kc"], case["vc"], bt, lens,
                                       case["scale"], case["ks"], case["vs"])
    got = ops.attn_prefill_paged(case["q"], case["kc"], case["vc"], _meta(case), case["scale"],
                                 case["ks"], case["vs"])
    assert torch.equal(got, want)


# --- the bound rejects every mutant ---------------------------------------------

_SINGLE = [s for s in pc.CASES if len(s) == 1]


def _mutant_ratio(name, case):
    m = pc.MUTANTS[name](case)
    if m is None:
        return None
    e, a = pc.case_oracle(case)
    return pc.check(m, e, a, pc.C_MFMA)[0]


# h % KVH is the right head map without GQA: no such mutant at (4, 4)
_MUTANT_PARAMS = [(name, H, KVH, fp8) for name in pc.MUTANTS
                  for H, KVH, fp8 in [(4, 4, False), (8, 2, False), (8, 2, True)]
                  if not (name == "head map h % KVH" and H == KVH)]


@pytest.mark.parametrize("name,H,KVH,fp8", _MUTANT_PARAMS)
def test_mutant_rejected(name, H, KVH, fp8):
    """Each defect exceeds the bound on the multi-sequence batch and on at
    least one single-sequence case (some are marginal on the shortest rows of
    a long prefix, so not on every one); the one mutant that needs two
    sequences is exempt from the second half."""
    multi = _mutant_ratio(name, pc.make_case(pc.MULTI, H, KVH, 16, fp8))
    assert multi is not None and multi > 1.0, f"{name}: multi-sequence ratio {multi}"
    if name in pc.MULTI_ONLY:
        return
    ratios = {pc.case_id(s): _mutant_ratio(name, pc.make_case(s, H, KVH, 16, fp8))
              for s in _SINGLE}
    hit = {k: r for k, r in ratios.items() if r is not None and r > 1.0}
    assert hit, f"{name}: no single-sequence case rejects it: {ratios}"


# --- engine: flag on == flag off on the CPU -------------------------------------

def _cfg(model, **kw):
    base = dict(model=model, max_kv_blocks=512, use_hip_graphs=False, device="cpu", seed=0,
                max_batch_size=64, default_max_new_tokens=8, prefix_cache_min_tokens=16)
    base.update(kw)
    return EngineConfig(**base)


def _count_calls(monkeypatch):
    calls = {"n": 0}
    real = ops.attn_prefill_paged

    def spy(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "attn_prefill_paged", spy)
    return calls


def greedy(n=8):
    return SamplingParams(temperature=0.0, max_tokens=n)


IDS37 = [(i * 17) % 200 + 1 for i in range(37)]       # not a chunk multiple


def _chunked(eng):
    seq = eng.kv.alloc_sequence(len(IDS37))
    logits = None
    for a in range(0, len(IDS37), 8):
        e = min(a + 8, len(IDS37))
        r = eng.prefill_chunk(seq, IDS37, a, e, want_logits=(e == len(IDS37)))
        if r is not None:
            logits = r
    slots = torch.tensor(eng.kv.prefill_slot_mapping(seq))
    bs = eng.kv.block_size
    kv = [(kc[slots // bs, :, slots % bs].clone(), vc[slots // bs, :, slots % bs].clone())
          for (kc, vc, _ks, _vs) in eng.kv.layer_caches()]
    eng.kv.free_sequence(seq)
    return logits, kv


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-mixtral"])
def test_engine_prefill_chunk_bit_identical(model, monkeypatch):
    calls = _count_calls(monkeypatch)
    l_off, kv_off = _chunked(LLMEngine(_cfg(model)))
    assert calls["n"] == 0, "flag off must never call attn_prefill_paged"
    l_on, kv_on = _chunked(LLMEngine(_cfg(model, paged_prefill_attention=True)))
    assert calls["n"] > 0, "flag on must run attn_prefill_paged"
    assert l_on is not None and torch.equal(l_on, l_off)
    for (ka, va), (kb, vb) in zip(kv_on, kv_off):
        assert torch.equal(ka, kb) and torch.equal(va, vb)


HEAD32 = list(range(1, 33))       # two full blocks at block_size 16


def _prefix_hit(eng, monkeypatch):
    """Second of two requests sharing a 32-token head: the logits its tail
    prefill returned, and both requests' outputs."""
    got = []
    real = eng._prefill_tails

    def spy(*a, **kw):
        r = real(*a, **kw)
        got.append(r.clone())
        return r

    monkeypatch.setattr(eng, "_prefill_tails", spy)
    o1 = eng.generate([GenRequest(prompt_ids=HEAD32 + [40, 41, 42], n=1, sampling=greedy())])[0]
    assert not got, "the first request cannot hit the prefix cache"
    o2 = eng.generate([GenRequest(prompt_ids=HEAD32 + [50, 51, 52, 53, 54], n=2,
                                  sampling=greedy())])[0]
    assert len(got) == 1, "the second request must prefill its tail through the cache"
    return got[0], [s.token_ids for o in (o1, o2) for s in o.streams]


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-mixtral"])
def test_engine_prefix_cache_tail_bit_identical(model, monkeypatch):
    calls = _count_calls(monkeypatch)
    l_off, t_off = _prefix_hit(LLMEngine(_cfg(model)), monkeypatch)
    assert calls["n"] == 0
    l_on, t_on = _prefix_hit(LLMEngine(_cfg(model, paged_prefill_attention=True)), monkeypatch)
    assert calls["n"] > 0
    assert torch.equal(l_on, l_off)
    assert t_on == t_off


def _scheduled(eng):
    sched = BatchScheduler(eng, admit_wait_s=0.05)
    long_prompt = [(i * 13) % 150 + 1 for i in range(40)]
    f_long = sched.submit(GenRequest(prompt_ids=long_prompt, n=2, sampling=greedy(10)))
    f_short = sched.submit(GenRequest(prompt_ids=[3, 1, 4], n=1, sampling=greedy(6)))
    outs = [f_long.result(timeout=120), f_short.result(timeout=120)]
    sched.shutdown()
    return [s.token_ids for o in outs for s in o.streams]


@pytest.mark.parametrize("model", ["tiny-llama", "tiny-mixtral"])
def test_engine_scheduler_chunked_same_tokens(model, monkeypatch):
    calls = _count_calls(monkeypatch)
    t_off = _scheduled(LLMEngine(_cfg(model, prefill_chunk_tokens=8)))
    assert calls["n"] == 0
    t_on = _scheduled(LLMEngine(_cfg(model, prefill_chunk_tokens=8,
                                     paged_prefill_attention=True)))
    assert calls["n"] > 0
    assert t_on == t_off


def test_env_override(monkeypatch):
    monkeypatch.delenv("KLLMS_PAGED_PREFILL_ATTN", raising=False)
    assert LLMEngine(_cfg("tiny-llama")).paged_prefill_attention is False
    assert EngineConfig(model="tiny-llama").paged_prefill_attention is False
    monkeypatch.setenv("KLLMS_PAGED_PREFILL_ATTN", "1")
    assert LLMEngine(_cfg("tiny-llama")).paged_prefill_attention is True
    monkeypatch.setenv("KLLMS_PAGED_PREFILL_ATTN", "0")
    assert LLMEngine(_cfg("tiny-llama", paged_prefill_attention=True)).paged_prefill_attention is False
    monkeypatch.setenv("KLLMS_PAGED_PREFILL_ATTN", "yes")
    with pytest.raises(ValueError, match="KLLMS_PAGED_PREFILL_ATTN"):
        LLMEngine(_cfg("tiny-llama"))
