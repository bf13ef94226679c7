"""The key-split mode of the paged MFMA prefill-attention kernel on the GPU:
split kernel + reduce against the float64 oracle of ``paged_prefill_cases``
within the unsplit kernel's own criterion, with guarded output and workspace
buffers, bitwise reproducible and independent of block placement, the
binding's argument checks, and inside the engine
(``paged_prefill_key_splits``) against the path it replaces.

``test_paged_prefill_split.py`` proves on the CPU, with the same cases, that
the plans cover every key once and that the bound rejects a dropped group, a
shifted or doubled range and three defective merges.

Run on an MI355X box: python -m pytest tests/test_gpu_paged_prefill_split.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops
from kllms_amd.engine.config import EngineConfig
from kllms_amd.engine.engine import GenRequest, LLMEngine
from kllms_amd.engine.sampling import SamplingParams
from kllms_amd.models.llama import ForwardBatch

import kernel_oracles as ko
import paged_prefill_cases as pc
import paged_prefill_split_cases as sc

DEV = "cuda:0"
PARAMS, IDS = sc.all_params()

_dev = {}


def on_dev(case):
    """Device copies of a case's tensors, made once."""
    key = case["name"]
    if key not in _dev:
        d = {k: v.to(DEV) for k, v in case.items() if isinstance(v, torch.Tensor)}
        T, H = case["q"].shape[:2]
        d["q"] = d["fused"][:, : H * pc.D].view(T, H, pc.D)
        assert T == 1 or d["q"].stride(0) == d["fused"].shape[1]
        _dev[key] = d
    return _dev[key]


def run(case, key_splits, **kw):
    d = on_dev(case)
    meta = sc.plan(case, key_splits, DEV, **kw)
    assert meta.has_splits
    return ops.attn_prefill_paged(d["q"], d["kc"], d["vc"], meta, case["scale"],
                                  d.get("ks"), d.get("vs"))


def accept(case, out, what="attn_prefill_paged_split"):
    e, a = pc.case_oracle(case, round_kv_bf16=True)
    ratio, idx = pc.check(out, e, a, pc.C_MFMA)
    msg = ko.describe(what, case["name"], ratio, idx, ("token", "head", "dim"),
                      pc.where(case)(idx))
    print("RATIO " + msg)
    assert ratio <= 1.0, msg


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8,k", PARAMS, ids=IDS)
def test_kernel_vs_oracle(seqs, H, KVH, BS, fp8, k):
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    accept(case, run(case, k), f"attn_prefill_paged_split key_splits={k}")


@pytest.mark.parametrize("tpg", [1, 3, 8])
@pytest.mark.parametrize("seqs", [pc.MULTI, [(257, 257)]], ids=pc.case_id)
def test_kernel_any_tile_packing(seqs, tpg):
    case = pc.make_case(seqs, 8, 2, 16, False)
    accept(case, run(case, 3, tiles_per_group=tpg),
           f"attn_prefill_paged_split key_splits=3 tiles_per_group={tpg}")


def _raw(case, meta, out, part_o, part_ml, **over):
    d = on_dev(case)
    none = torch.empty(0, dtype=torch.float32, device=DEV)
    a = dict(out=out, q=d["q"], kc=d["kc"], vc=d["vc"], bt=meta.block_tables, cu=meta.cu_q,
             q_start=meta.q_start, grp_seq=meta.grp_seq, grp_qpos0=meta.grp_qpos0,
             grp_krange=meta.grp_krange, grp_split=meta.grp_split, seq_nsplit=meta.seq_nsplit,
             seq_ws_base=meta.seq_ws_base, part_o=part_o, part_ml=part_ml,
             ws_rows=meta.ws_rows, max_splits=meta.max_splits,
             ks=d["ks"] if case["fp8"] else none, vs=d["vs"] if case["fp8"] else none)
    a.update(over)
    ops._C.attn_prefill_paged_split(
        a["out"], a["q"], a["kc"], a["vc"], a["bt"], a["cu"], a["q_start"], a["grp_seq"],
        a["grp_qpos0"], a["grp_krange"], a["grp_split"], a["seq_nsplit"], a["seq_ws_base"],
        a["part_o"], a["part_ml"], a["ws_rows"], a["max_splits"], case["scale"], a["ks"], a["vs"])


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8", [
    ([(16, 70)], 8, 2, 16, False), (pc.MULTI, 8, 2, 16, True), (sc.MIXED, 4, 4, 16, False),
], ids=["16+70-bf16", "multi-fp8", "mixed-mha"])
def test_guarded_output_and_workspace(seqs, H, KVH, BS, fp8):
    """``out`` and both workspace tensors are the middles of sentinel-filled
    buffers: the sentinels around them survive, every output row is written
    and so is every partial slot."""
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    meta = sc.plan(case, 3, DEV)
    T, W = case["q"].shape[0], meta.ws_rows
    pad, sentinel = 40, 12352.0            # exact in bf16, far from any output
    big = torch.full((T + 2 * pad, H, pc.D), sentinel, dtype=torch.bfloat16, device=DEV)
    big_o = torch.full((W + 2 * pad, H, pc.D), sentinel, dtype=torch.float32, device=DEV)
    big_ml = torch.full((W + 2 * pad, H, 2), sentinel, dtype=torch.float32, device=DEV)
    out, part_o, part_ml = big[pad: pad + T], big_o[pad: pad + W], big_ml[pad: pad + W]
    assert out.is_contiguous() and part_o.is_contiguous() and part_ml.is_contiguous()
    _raw(case, meta, out, part_o, part_ml)
    torch.cuda.synchronize()
    for name, b, n in (("out", big, T), ("part_o", big_o, W), ("part_ml", big_ml, W)):
        assert (b[:pad] == sentinel).all() and (b[pad + n:] == sentinel).all(), \
            f"the kernels wrote outside {name}"
    unwritten = (out == sentinel).any(dim=-1).nonzero().tolist()
    assert not unwritten, f"(row, head) never written: {unwritten[:8]}"
    assert not (part_ml == sentinel).any(), "a partial (m, l) slot was never written"
    assert not (part_o == sentinel).any(), "a partial O slot was never written"
    accept(case, out)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_reproducible_and_block_placement_independent(fp8):
    case = pc.make_case(pc.MULTI, 8, 2, 16, fp8)
    other = pc.permuted(case)
    assert not torch.equal(case["bt"], other["bt"])
    first = run(case, 3)
    assert torch.equal(first, run(case, 3)), "two runs differ"
    assert torch.equal(first, run(other, 3)), "the result depends on the block placement"


def test_binding_rejects_bad_arguments():
    case = pc.make_case([(100, 33)], 8, 2, 16, False)
    d = on_dev(case)
    meta = sc.plan(case, 3, DEV)
    H, W = 8, meta.ws_rows
    out = torch.empty(case["q"].shape, dtype=torch.bfloat16, device=DEV)
    part_o = torch.empty((W, H, 128), dtype=torch.float32, device=DEV)
    part_ml = torch.empty((W, H, 2), dtype=torch.float32, device=DEV)

    def call(**over):
        _raw(case, meta, over.pop("out", out), over.pop("part_o", part_o),
             over.pop("part_ml", part_ml), **over)

    call()
    bad = [
        dict(out=out.float()),                                   # dtypes
        dict(part_o=part_o.bfloat16()),
        dict(part_ml=part_ml.double()),
        dict(grp_split=meta.grp_split.long()),
        dict(grp_krange=meta.grp_krange.repeat(2)[::2]),         # non-contiguous metadata
        dict(grp_split=meta.grp_split.repeat(2)[::2]),
        dict(part_o=part_o[: W - 1]),                            # workspace too small
        dict(part_ml=part_ml[: W - 1]),
        dict(part_o=torch.empty((W, H + 1, 128), dtype=torch.float32, device=DEV)),
        dict(ws_rows=W * 1000),
        dict(max_splits=1),
        dict(max_splits=65),
        dict(seq_nsplit=meta.seq_nsplit.repeat(2)),              # wrong lengths
        dict(grp_krange=meta.grp_krange[:-2].contiguous()),
        dict(grp_split=meta.grp_split.repeat(2)),
    ]
    scales = torch.ones(d["kc"].shape[:3], dtype=torch.float32, device=DEV)
    bad.append(dict(ks=scales, vs=scales))                       # scales with a bf16 cache
    for over in bad:
        what = {k: (tuple(v.shape), v.dtype, v.is_contiguous()) if isinstance(v, torch.Tensor)
                else v for k, v in over.items()}
        with pytest.raises(RuntimeError):
            call(**over)
            pytest.fail(f"the binding accepted {what}")
    torch.cuda.synchronize()


# --- engine ---------------------------------------------------------------------

PROMPT = [(i * 37) % 1900 + 1 for i in range(150)]
HIT_PROMPT = PROMPT[:128] + [(i * 53) % 1900 + 7 for i in range(22)]
CHUNK = 48


def _engine(kv_dtype, on, **kw):
    return LLMEngine(EngineConfig(
        model="mid-llama", max_kv_blocks=256, use_hip_graphs=False, device=DEV, seed=0,
        kv_cache_dtype=kv_dtype, paged_prefill_attention=on, prefix_cache_min_tokens=64, **kw))


def _spy(monkeypatch):
    """Counts the launches of the split entry point."""
    calls = {"n": 0}
    real = ops._C.attn_prefill_paged_split

    def spy(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops._C, "attn_prefill_paged_split", spy)
    return calls


def _chunked(eng):
    """Last-token logits of PROMPT prefilled in chunks, and layer 0's K/V rows."""
    seq = eng.kv.alloc_sequence(len(PROMPT))
    logits = None
    for a in range(0, len(PROMPT), CHUNK):
        e = min(a + CHUNK, len(PROMPT))
        r = eng.prefill_chunk(seq, PROMPT, a, e, want_logits=(e == len(PROMPT)))
        if r is not None:
            logits = r
    slots = torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV)
    bs = eng.kv.block_size
    kc, vc, _ks, _vs = eng.kv.layer_caches()[0]
    kv0 = (kc[slots // bs, :, slots % bs].view(torch.uint8).clone(),
           vc[slots // bs, :, slots % bs].view(torch.uint8).clone())
    eng.kv.free_sequence(seq)
    return logits[0].float().cpu(), kv0


def _packed(eng, ids):
    seq = eng.kv.alloc_sequence(len(ids))
    batch = ForwardBatch(
        mode="prefill",
        positions=torch.arange(len(ids), device=DEV),
        slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
        kv_caches=eng.kv.layer_caches(),
        cu_seqlens=torch.tensor([0, len(ids)], dtype=torch.int32, device=DEV),
    )
    logits = eng.model.forward_prefill(torch.tensor(ids, device=DEV), batch)
    eng.kv.free_sequence(seq)
    return logits[0].float().cpu()


def _criterion(a, b, c, d, what):
    """The criterion of ``test_gpu_paged_prefill.py``: (a) torch reference,
    (b) flag off, (c) flag on, (d) packed prefill; err_c <= 2 * max(err_b,
    err_d) — (d) has the kernel's bf16-probability numerics, (b) is the path
    it replaces, the factor 2 allows for a different tiling drawing another
    sample of the same roundings."""
    err = lambda x: float((x - a).abs().max())
    err_b, err_c, err_d = err(b), err(c), err(d)
    msg = (f"{what}: max|logit - torch reference|: decode path (flag off) {err_b:.5f}, "
           f"split paged prefill (key_splits=3) {err_c:.5f}, packed prefill {err_d:.5f}")
    print("ERRORS " + msg)
    assert err_c <= 2.0 * max(err_b, err_d), msg


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8_e4m3"])
def test_engine_chunked_prefill(kv_dtype, monkeypatch):
    calls = _spy(monkeypatch)
    off = _engine(kv_dtype, False)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "1")
    a, _ = _chunked(off)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "0")
    b, kv_b = _chunked(off)
    d = _packed(off, PROMPT)
    _chunked(_engine(kv_dtype, True, paged_prefill_key_splits=1))
    assert calls["n"] == 0, "key_splits=1 must never run the split entry point"
    c, kv_c = _chunked(_engine(kv_dtype, True, paged_prefill_key_splits=3))
    assert calls["n"] > 0, "key_splits=3 must run the split entry point"
    # layer 0's K/V does not depend on attention
    assert torch.equal(kv_b[0], kv_c[0]) and torch.equal(kv_b[1], kv_c[1])
    _criterion(a, b, c, d, f"chunked prefill, {kv_dtype} KV cache")


def _tail_logits(eng, monkeypatch):
    """Prefill a 150-token prompt, then a second one sharing its first 128
    tokens: the logits the second one's tail prefill returned."""
    got = []
    real = eng._prefill_tails

    def spy(*a, **kw):
        r = real(*a, **kw)
        got.append(r[0].float().cpu())
        return r

    monkeypatch.setattr(eng, "_prefill_tails", spy)
    greedy = SamplingParams(temperature=0.0, max_tokens=2)
    eng.generate([GenRequest(prompt_ids=PROMPT, n=1, sampling=greedy)])
    assert not got
    eng.generate([GenRequest(prompt_ids=HIT_PROMPT, n=1, sampling=greedy)])
    assert len(got) == 1, "the second prompt must hit the prefix cache"
    return got[0]


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8_e4m3"])
def test_engine_prefix_cache_tail(kv_dtype, monkeypatch):
    calls = _spy(monkeypatch)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "1")
    a = _tail_logits(_engine(kv_dtype, False), monkeypatch)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "0")
    off = _engine(kv_dtype, False)
    b = _tail_logits(off, monkeypatch)
    d = _packed(off, HIT_PROMPT)
    _tail_logits(_engine(kv_dtype, True, paged_prefill_key_splits=1), monkeypatch)
    assert calls["n"] == 0
    c = _tail_logits(_engine(kv_dtype, True, paged_prefill_key_splits=3), monkeypatch)
    assert calls["n"] > 0
    _criterion(a, b, c, d, f"prefix-cache tail, {kv_dtype} KV cache")
