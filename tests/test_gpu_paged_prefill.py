"""The paged (append / extend) MFMA prefill-attention kernel on the GPU: against
the float64 oracle of ``paged_prefill_cases`` within the packed prefill
kernel's own bound, with a guarded output buffer, under a permuted physical
block placement, and inside the engine (``paged_prefill_attention``) against
the path it replaces.

``test_paged_prefill.py`` proves on the CPU, with the same cases, that the
bound rejects a lost diagonal / prefix / boundary key, a visible future key,
a wrong head map, a wrong table row and an ignored q stride.

Run on an MI355X box: python -m pytest tests/test_gpu_paged_prefill.py -m gpu -q
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

DEV = "cuda:0"
PARAMS, IDS = pc.all_params()

_dev = {}


def on_dev(case):
    """Device copies of a case's tensors and its metadata, made once."""
    key = case["name"]
    if key not in _dev:
        d = {k: v.to(DEV) for k, v in case.items() if isinstance(v, torch.Tensor)}
        T, H = case["q"].shape[:2]
        d["q"] = d["fused"][:, : H * pc.D].view(T, H, pc.D)
        assert T == 1 or d["q"].stride(0) == d["fused"].shape[1]
        d["meta"] = ops.build_paged_prefill(case["lens"], case["starts"], case["block_lists"],
                                            DEV, case["BS"])
        _dev[key] = d
    return _dev[key]


def run(case, **kw):
    d = on_dev(case)
    meta = d["meta"] if not kw else ops.build_paged_prefill(
        case["lens"], case["starts"], case["block_lists"], DEV, case["BS"], **kw)
    return ops.attn_prefill_paged(d["q"], d["kc"], d["vc"], meta, case["scale"],
                                  d.get("ks"), d.get("vs"))


def accept(case, out, what="attn_prefill_paged"):
    e, a = pc.case_oracle(case, round_kv_bf16=True)
    ratio, idx = pc.check(out, e, a, pc.C_MFMA)
    msg = ko.describe(what, case["name"], ratio, idx, ("token", "head", "dim"),
                      pc.where(case)(idx))
    print("RATIO " + msg)
    assert ratio <= 1.0, msg


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8", PARAMS, ids=IDS)
def test_kernel_vs_oracle(seqs, H, KVH, BS, fp8):
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    accept(case, run(case))


@pytest.mark.parametrize("tpg", [1, 3, 8])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_kernel_any_tile_packing(fp8, tpg):
    """The host may pack 1..8 q-tiles per workgroup; each packing is held to
    the oracle (the default one is what ``test_kernel_vs_oracle`` runs)."""
    case = pc.make_case(pc.MULTI, 8, 2, 16, fp8)
    accept(case, run(case, tiles_per_group=tpg), f"attn_prefill_paged tiles_per_group={tpg}")


@pytest.mark.parametrize("seqs,H,KVH,BS,fp8", [
    ([(100, 33)], 8, 2, 16, False), (pc.MULTI, 8, 2, 16, True), (pc.MULTI, 4, 4, 16, False),
], ids=["100+33-bf16", "multi-fp8", "multi-mha"])
def test_guarded_output(seqs, H, KVH, BS, fp8):
    """``out`` is the middle of a sentinel-filled buffer: the sentinels around
    it survive and every row inside is written."""
    case = pc.make_case(seqs, H, KVH, BS, fp8)
    d = on_dev(case)
    T = case["q"].shape[0]
    pad, sentinel = 40, 12352.0            # exact in bf16, far from any output
    big = torch.full((T + 2 * pad, H, pc.D), sentinel, dtype=torch.bfloat16, device=DEV)
    out = big[pad: pad + T]
    assert out.is_contiguous()
    none = torch.empty(0, dtype=torch.float32, device=DEV)
    m = d["meta"]
    ops._C.attn_prefill_paged(out, d["q"], d["kc"], d["vc"], m.block_tables, m.cu_q, m.q_start,
                              m.grp_seq, m.grp_qpos0, case["scale"],
                              d["ks"] if fp8 else none, d["vs"] if fp8 else none)
    torch.cuda.synchronize()
    assert (big[:pad] == sentinel).all() and (big[pad + T:] == sentinel).all(), \
        "the kernel wrote outside its output rows"
    unwritten = (out == sentinel).any(dim=-1).nonzero().tolist()
    assert not unwritten, f"(row, head) never written: {unwritten[:8]}"
    accept(case, out)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_block_placement_independent(fp8):
    case = pc.make_case(pc.MULTI, 8, 2, 16, fp8)
    other = pc.permuted(case)
    assert not torch.equal(case["bt"], other["bt"])
    assert torch.equal(run(case), run(other))


def test_binding_rejects_bad_arguments():
    case = pc.make_case([(16, 31)], 8, 2, 16, False)
    d = on_dev(case)
    m = d["meta"]
    none = torch.empty(0, dtype=torch.float32, device=DEV)
    out = torch.empty(case["q"].shape, dtype=torch.bfloat16, device=DEV)

    def call(out=out, q=d["q"], kc=d["kc"], vc=d["vc"], bt=m.block_tables, cu=m.cu_q,
             ks=none, vs=none):
        ops._C.attn_prefill_paged(out, q, kc, vc, bt, cu, m.q_start, m.grp_seq, m.grp_qpos0,
                                  case["scale"], ks, vs)

    call()
    with pytest.raises(RuntimeError):
        call(out=out.float())
    with pytest.raises(RuntimeError):
        call(out=torch.empty(31, 16, 128, dtype=torch.bfloat16, device=DEV)[:, ::2])
    with pytest.raises(RuntimeError):
        call(q=d["q"][:, :, :64])
    with pytest.raises(RuntimeError):
        call(cu=m.cu_q.long())
    with pytest.raises(RuntimeError):
        call(bt=m.block_tables.repeat(2, 1))     # one table row per sequence
    scales = torch.ones(d["kc"].shape[:3], dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        call(ks=scales, vs=scales)             # scales with a bf16 cache
    with pytest.raises(RuntimeError):
        call(kc=d["kc"].to(torch.float8_e4m3fn), vc=d["vc"].to(torch.float8_e4m3fn))
    torch.cuda.synchronize()


# --- engine ---------------------------------------------------------------------

PROMPT = [(i * 37) % 1900 + 1 for i in range(150)]
CHUNK = 48


def _engine(kv_dtype, on, **kw):
    return LLMEngine(EngineConfig(
        model="mid-llama", max_kv_blocks=256, use_hip_graphs=False, device=DEV, seed=0,
        kv_cache_dtype=kv_dtype, paged_prefill_attention=on, prefix_cache_min_tokens=64, **kw))


def _spy(monkeypatch):
    calls = {"n": 0}
    real = ops.attn_prefill_paged

    def spy(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "attn_prefill_paged", spy)
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
    err = lambda x: float((x - a).abs().max())
    err_b, err_c, err_d = err(b), err(c), err(d)
    msg = (f"{what}: max|logit - torch reference|: decode path (flag off) {err_b:.5f}, "
           f"paged prefill kernel (flag on) {err_c:.5f}, packed prefill {err_d:.5f}")
    print("ERRORS " + msg)
    assert err_c <= 2.0 * max(err_b, err_d), msg


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8_e4m3"])
def test_engine_chunked_prefill(kv_dtype, monkeypatch):
    """(a) torch reference, (b) flag off, (c) flag on, (d) packed prefill of
    the whole prompt: err_c <= 2 * max(err_b, err_d). (d) has the kernel's
    bf16-probability numerics, (b) is the path it replaces; the factor 2
    allows for a different tiling drawing another sample of the same
    roundings."""
    calls = _spy(monkeypatch)
    off = _engine(kv_dtype, False)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "1")
    a, _ = _chunked(off)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "0")
    b, kv_b = _chunked(off)
    d = _packed(off, PROMPT)
    assert calls["n"] == 0, "flag off must never call attn_prefill_paged"
    c, kv_c = _chunked(_engine(kv_dtype, True))
    assert calls["n"] > 0, "flag on must run the paged prefill kernel"
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


HIT_PROMPT = PROMPT[:128] + [(i * 53) % 1900 + 7 for i in range(22)]


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8_e4m3"])
def test_engine_prefix_cache_tail(kv_dtype, monkeypatch):
    calls = _spy(monkeypatch)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "1")
    a = _tail_logits(_engine(kv_dtype, False), monkeypatch)
    monkeypatch.setenv("KLLMS_AMD_FORCE_TORCH_OPS", "0")
    off = _engine(kv_dtype, False)
    b = _tail_logits(off, monkeypatch)
    d = _packed(off, HIT_PROMPT)
    assert calls["n"] == 0
    c = _tail_logits(_engine(kv_dtype, True), monkeypatch)
    assert calls["n"] > 0
    _criterion(a, b, c, d, f"prefix-cache tail, {kv_dtype} KV cache")
