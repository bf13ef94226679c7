"""Key splits of paged prefill attention on the CPU: the planner's coverage
properties, ``key_splits=1`` and auto against the unsplit plan, the emulation
of a correct split kernel against the float64 oracle, proof that the bound
rejects a defective plan or merge, and the engine with
``paged_prefill_key_splits``.

The HIP kernels are held to the same oracle in
``test_gpu_paged_prefill_split.py``.
"""

import dataclasses

import pytest
import torch

from kllms_amd import ops
from kllms_amd.engine.config import EngineConfig
from kllms_amd.engine.engine import LLMEngine
from kllms_amd.ops import torch_ref

import kernel_oracles as ko
import paged_prefill_cases as pc
import paged_prefill_split_cases as sc

PARAMS, IDS = sc.all_params()


def _lists(seqs, BS=16):
    lens = [n for _, n in seqs]
    starts = [s for s, _ in seqs]
    blocks, nxt = [], 5
    for s, n in seqs:
        nb = (s + n + BS - 1) // BS
        blocks.append(list(range(nxt, nxt + nb)))
        nxt += nb
    return lens, starts, blocks


# --- planner ----------------------------------------------------------------------

@pytest.mark.parametrize("tpg", [1, 3, 8])
@pytest.mark.parametrize("k", sc.KEY_SPLITS)
@pytest.mark.parametrize("seqs", sc.SPLIT_CASES, ids=pc.case_id)
def test_plan_ranges_cover_every_key_once(seqs, k, tpg):
    lens, starts, blocks = _lists(seqs)
    meta = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, tiles_per_group=tpg,
                                   key_splits=k, num_q_heads=8)
    assert meta.has_splits
    for t in (meta.grp_krange, meta.grp_split, meta.seq_nsplit, meta.seq_ws_base):
        assert t.dtype == torch.int32
    G = meta.n_groups
    assert meta.grp_krange.numel() == 2 * G and meta.grp_split.numel() == G
    assert meta.grp_qpos0.numel() == 8 * G
    nsplit = meta.seq_nsplit.tolist()
    assert len(nsplit) == len(seqs) and meta.max_splits == max(nsplit)
    by_tile = {}
    for s, r0, kb, ke, j in sc.groups_of(meta):
        by_tile.setdefault((s, r0), []).append((kb, ke, j))
    want_tiles = sorted((s, r) for s, n in enumerate(lens) for r in range(0, n, 32))
    assert sorted(by_tile) == want_tiles, "every (sequence, 32-row tile) is planned"
    for (s, r0), ranges in by_tile.items():
        total = starts[s] + lens[s]
        rounds = (total + 63) // 64
        n = nsplit[s]
        assert 1 <= n <= min(k, rounds), "never more splits than requested or than rounds"
        assert len(ranges) == n
        if n == 1:
            assert ranges == [(0, 0x7FFFFFFF, -1)], "an unsplit sequence keeps the direct epilogue"
            continue
        assert sorted(j for _, _, j in ranges) == list(range(n)), "split indices 0..n-1 once each"
        ranges.sort()
        assert all(kb % 64 == 0 for kb, _, _ in ranges), "range starts are 64-aligned"
        assert [j for _, _, j in ranges] == list(range(n)), "ranges ascend with the split index"
        assert ranges[0][0] == 0 and ranges[-1][1] == total
        for (_, e0, _), (b1, _, _) in zip(ranges, ranges[1:]):
            assert e0 == b1, "contiguous: disjoint and without a gap"
        per = [(ke - kb + 63) // 64 for kb, ke, _ in ranges]
        assert all(p >= 1 for p in per) and max(per) - min(per) <= 1, f"uneven ranges {per}"
    # workspace: one slot per (row, split) of the split sequences, disjoint per sequence
    base = meta.seq_ws_base.tolist()
    nxt = 0
    for s, n in enumerate(nsplit):
        if n > 1:
            assert base[s] == nxt
            nxt += lens[s] * n
    assert meta.ws_rows == nxt
    assert meta.ws_rows * 8 * ops.PAGED_PREFILL_WS_CELL_BYTES <= ops.PAGED_PREFILL_WS_BYTES


def test_plan_reduces_splits_to_fit_the_budget(monkeypatch):
    lens, starts, blocks = _lists([(4096, 128), (0, 1)])
    cell = ops.PAGED_PREFILL_WS_CELL_BYTES * 32
    monkeypatch.setattr(ops, "PAGED_PREFILL_WS_BYTES", 128 * 5 * cell + 7)
    meta = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=16, num_q_heads=32)
    assert meta.seq_nsplit.tolist() == [5, 1]
    assert meta.ws_rows * cell <= ops.PAGED_PREFILL_WS_BYTES
    monkeypatch.setattr(ops, "PAGED_PREFILL_WS_BYTES", cell)
    meta = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=16, num_q_heads=32)
    assert not meta.has_splits, "no room for any partial: the unsplit plan"


def _same_plan(a, b):
    for f in dataclasses.fields(ops.PagedPrefill):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
            assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor), f.name
            assert x.dtype == y.dtype and torch.equal(x, y), f.name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("tpg", [None, 3])
@pytest.mark.parametrize("seqs", sc.SPLIT_CASES, ids=pc.case_id)
def test_key_splits_1_is_the_plan_without_the_argument(seqs, tpg):
    lens, starts, blocks = _lists(seqs)
    old = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, tiles_per_group=tpg)
    new = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, tiles_per_group=tpg,
                                  key_splits=1, num_q_heads=8)
    _same_plan(old, new)
    assert not new.has_splits and new.grp_krange is None and new.grp_split is None
    assert new.seq_nsplit is None and new.ws_rows == 0


@pytest.mark.parametrize("seqs", [[(0, 2048)], [(14336, 2048)], [(2048, 64)] * 8],
                         ids=["0+2048", "14336+2048", "8x2048+64"])
def test_auto_keeps_a_batch_that_fills_the_device(seqs):
    """64 q-tiles x 32 heads (or 8 groups x 32 heads) are at least 256
    workgroups: auto on a 256-CU device returns the unsplit plan itself."""
    lens, starts, blocks = _lists(seqs)
    old = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16)
    auto = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=0,
                                   num_q_heads=32, num_cus=256)
    assert old.n_groups * 32 >= 256
    _same_plan(old, auto)


def test_auto_splits_a_short_tail_after_a_long_prefix():
    lens, starts, blocks = _lists([(4096, 128)])
    auto = ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=0,
                                   num_q_heads=32, num_cus=256)
    assert auto.has_splits and auto.seq_nsplit.tolist() == [8]
    assert auto.n_groups * 32 == 256, "4 q-tiles packed into one workgroup x 8 key ranges"
    rounds = [(ke - kb + 63) // 64 for _, _, kb, ke, _ in sc.groups_of(auto)]
    assert min(rounds) >= ops.PAGED_PREFILL_AUTO_MIN_ROUNDS
    # no CU count to be had (the CPU): auto is the unsplit plan
    _same_plan(ops.build_paged_prefill(lens, starts, blocks, "cpu", 16),
               ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=0,
                                       num_q_heads=32))
    # too few rounds to give every split its minimum: unsplit
    lens, starts, blocks = _lists([(100, 33)])
    assert not ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=0,
                                       num_q_heads=32, num_cus=256).has_splits


def test_bad_arguments_raise():
    lens, starts, blocks = _lists([(100, 33)])
    with pytest.raises(ValueError, match="key_splits"):
        ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=-1)
    with pytest.raises(ValueError, match="key_splits"):
        ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=2.0)
    with pytest.raises(ValueError, match="num_q_heads"):
        ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=0)
    with pytest.raises(ValueError, match="num_q_heads"):
        ops.build_paged_prefill(lens, starts, blocks, "cpu", 16, key_splits=2, num_q_heads=0)


# --- the emulation of a correct split kernel stays inside the bound ---------------

_worst = {"ratio": 0.0, "id": None}


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8,k", PARAMS, ids=IDS)
def test_emulation_within_bound(seqs, H, KVH, BS, fp8, k):
    """bf16 probabilities, fp32 partials and merge, over the planner's own
    metadata, against the float64 oracle within the kernel's criterion. (The
    unsplit kernel reaches 0.65 of the bound on its cases and its emulation
    0.62; every case chosen here must stay at or below 1.0. Worst here: 0.56,
    and 0.58 for the HIP kernels on the same cases.)"""
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    meta = sc.plan(case, k)
    out = sc.emulate(case, meta)
    ratio, idx = sc.ratio_of(case, out)
    msg = ko.describe(f"split emulation k={k}", case["name"], ratio, idx,
                      ("token", "head", "dim"), pc.where(case)(idx))
    if ratio > _worst["ratio"]:
        _worst.update(ratio=ratio, id=msg)
    print("RATIO " + msg)
    print(f"WORST so far {_worst['ratio']:.3f}")
    assert ratio <= 1.0, msg


@pytest.mark.parametrize("tpg", [1, 3, 8])
def test_emulation_any_tile_packing(tpg):
    for seqs in (pc.MULTI, [(257, 257)]):
        case = pc.make_case(seqs, 8, 2, 16, False)
        out = sc.emulate(case, sc.plan(case, 3, tiles_per_group=tpg))
        ratio, _ = sc.ratio_of(case, out)
        assert ratio <= 1.0, (seqs, tpg, ratio)


def test_op_dispatches_on_the_metadata(monkeypatch):
    """On the CPU ``ops.attn_prefill_paged`` runs the plan-walking emulation
    when the metadata has splits, the per-row reference otherwise; the two
    agree to fp32 rounding."""
    case = pc.make_case(sc.MIXED, 8, 2, 16, True)
    calls = []
    real = torch_ref.attn_prefill_paged_split
    monkeypatch.setattr(torch_ref, "attn_prefill_paged_split",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    args = (case["q"], case["kc"], case["vc"])
    one = ops.attn_prefill_paged(*args, sc.plan(case, 1), case["scale"], case["ks"], case["vs"])
    assert not calls
    meta = sc.plan(case, 3)
    assert meta.seq_nsplit.tolist() == [1, 3, 2]
    got = ops.attn_prefill_paged(*args, meta, case["scale"], case["ks"], case["vs"])
    assert calls and got.dtype == one.dtype
    # both are bf16 roundings of fp32 results that differ by summation order
    assert torch.allclose(got.float(), one.float(), rtol=2 ** -7, atol=1e-3)


# --- the bound rejects every mutant --------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("name", list(sc.MUTANTS))
def test_mutant_rejected(name, fp8):
    """On the case each mutant names, the sound plan and merge pass the bound
    and the defective one exceeds it."""
    fn, seqs, k = sc.MUTANTS[name]
    case = pc.make_case(seqs, 8, 2, 16, fp8)
    meta = sc.plan(case, k)
    good, _ = sc.ratio_of(case, sc.emulate(case, meta))
    assert good <= 1.0
    out = fn(case, meta)
    assert out is not None, f"{name}: {seqs} does not hold it"
    ratio, idx = sc.ratio_of(case, out)
    print(f"MUTANT {name} [{case['name']}]: ratio {ratio:.2f}")
    assert ratio > 1.0, f"{name}: ratio {ratio} passes the bound on {case['name']}"


def test_mutants_absent_where_nothing_to_touch():
    case = pc.make_case([(64, 1)], 8, 2, 16, False)
    assert sc.empty_partial_weighs_one(case, sc.plan(case, 2)) is None


# --- engine -----------------------------------------------------------------------

PROMPT = [(i * 37) % 1900 + 1 for i in range(150)]
CHUNK = 48


def _engine(**kw):
    return LLMEngine(EngineConfig(
        model="mid-llama", max_kv_blocks=256, use_hip_graphs=False, device="cpu", seed=0,
        paged_prefill_attention=True, **kw))


def _chunked(eng):
    seq = eng.kv.alloc_sequence(len(PROMPT))
    logits = None
    for a in range(0, len(PROMPT), CHUNK):
        e = min(a + CHUNK, len(PROMPT))
        r = eng.prefill_chunk(seq, PROMPT, a, e, want_logits=(e == len(PROMPT)))
        if r is not None:
            logits = r
    slots = torch.tensor(eng.kv.prefill_slot_mapping(seq))
    bs = eng.kv.block_size
    kc, vc, _ks, _vs = eng.kv.layer_caches()[0]
    kv0 = (kc[slots // bs, :, slots % bs].clone(), vc[slots // bs, :, slots % bs].clone())
    eng.kv.free_sequence(seq)
    return logits[0].float(), kv0


def test_engine_chunked_prefill_with_splits(monkeypatch):
    """Chunks 2..4 of a 150-token prompt have 2 or 3 rounds of keys, so
    ``paged_prefill_key_splits=3`` splits them. The emulation differs from
    the per-row reference only in fp32 summation order; through two layers of
    bf16 activations that is a few bf16 ulps of the logits' scale."""
    calls = []
    real = torch_ref.attn_prefill_paged_split
    monkeypatch.setattr(torch_ref, "attn_prefill_paged_split",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    one, kv_one = _chunked(_engine())
    assert not calls, "key_splits=1 must never take the split path"
    three, kv_three = _chunked(_engine(paged_prefill_key_splits=3))
    assert calls, "key_splits=3 must take the split path"
    assert torch.equal(kv_one[0], kv_three[0]) and torch.equal(kv_one[1], kv_three[1])
    tol = 4 * 2.0 ** -8 * float(one.abs().max())
    err = float((one - three).abs().max())
    print(f"ERRORS max|logit(k=3) - logit(k=1)| {err:.5f}, tolerance {tol:.5f}")
    assert err <= tol


def test_config_and_env(monkeypatch):
    monkeypatch.delenv("KLLMS_PAGED_PREFILL_KEY_SPLITS", raising=False)
    assert EngineConfig(model="tiny-llama").paged_prefill_key_splits == 1
    cfg = dict(model="tiny-llama", max_kv_blocks=64, use_hip_graphs=False, device="cpu", seed=0)
    assert LLMEngine(EngineConfig(**cfg)).paged_prefill_key_splits == 1
    assert LLMEngine(EngineConfig(**cfg, paged_prefill_key_splits=0)).paged_prefill_key_splits == 0
    with pytest.raises(ValueError, match="paged_prefill_key_splits"):
        LLMEngine(EngineConfig(**cfg, paged_prefill_key_splits=-1))
    monkeypatch.setenv("KLLMS_PAGED_PREFILL_KEY_SPLITS", "4")
    assert LLMEngine(EngineConfig(**cfg)).paged_prefill_key_splits == 4
    monkeypatch.setenv("KLLMS_PAGED_PREFILL_KEY_SPLITS", "-2")
    with pytest.raises(ValueError, match="KLLMS_PAGED_PREFILL_KEY_SPLITS"):
        LLMEngine(EngineConfig(**cfg))
