"""Opt-in fp8 (e4m3) Mixtral expert weights, CPU side: the config/env plumbing,
the torch reference of the batched weight-only GEMM against the float64 oracle
of ``fp8_expert_oracles`` (and the mutants that must break its bounds), the
quantised engine, dense against grouped path, and TP-degree invariance over
gloo.
"""

import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

import fp8_expert_oracles as eo
from kllms_amd import ops
from kllms_amd.ops import torch_ref

PORT = 29861
# (E, M, N, K)
SHAPES = [(1, 1, 64, 64), (4, 7, 80, 1088), (3, 33, 96, 1088)]


def _cfg(**kw):
    from kllms_amd.engine.config import EngineConfig

    base = dict(model="tiny-mixtral", max_kv_blocks=64, use_hip_graphs=False, device="cpu", seed=0)
    base.update(kw)
    return EngineConfig(**base)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("KLLMS_EXPERT_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)


# --- config -----------------------------------------------------------------------

class TestConfig:
    def test_default_and_validation(self):
        assert _cfg().expert_weight_dtype == "bf16"
        assert _cfg(expert_weight_dtype="fp8_e4m3").expert_weight_dtype == "fp8_e4m3"
        with pytest.raises(ValueError):
            _cfg(expert_weight_dtype="int8")

    def test_default_leaves_experts_alone(self):
        from kllms_amd.engine.engine import LLMEngine

        eng = LLMEngine(_cfg())
        assert eng.expert_weight_dtype == "bf16"
        for layer in eng.model.layers:
            assert layer.mlp.w_gate_up is not None and layer.mlp.w_down is not None
            assert not hasattr(layer.mlp, "w_gate_up_q")

    def test_env_overrides_both_ways(self, monkeypatch):
        from kllms_amd.engine.engine import LLMEngine

        monkeypatch.setenv("KLLMS_EXPERT_WEIGHT_DTYPE", "fp8_e4m3")
        eng = LLMEngine(_cfg())
        assert eng.expert_weight_dtype == "fp8_e4m3"
        assert all(layer.mlp.w_gate_up is None for layer in eng.model.layers)
        monkeypatch.setenv("KLLMS_EXPERT_WEIGHT_DTYPE", "bf16")
        eng = LLMEngine(_cfg(expert_weight_dtype="fp8_e4m3"))
        assert eng.expert_weight_dtype == "bf16"
        assert all(layer.mlp.w_gate_up is not None for layer in eng.model.layers)

    def test_env_rejects_bad_value(self, monkeypatch):
        from kllms_amd.engine.engine import LLMEngine

        monkeypatch.setenv("KLLMS_EXPERT_WEIGHT_DTYPE", "fp8")
        with pytest.raises(ValueError, match="KLLMS_EXPERT_WEIGHT_DTYPE"):
            LLMEngine(_cfg())

    def test_model_without_experts_raises(self):
        from kllms_amd.engine.engine import LLMEngine

        with pytest.raises(ValueError, match="experts"):
            LLMEngine(_cfg(model="tiny-llama", expert_weight_dtype="fp8_e4m3"))

    def test_weight_dtype_alone_points_to_the_expert_field(self):
        from kllms_amd.engine.engine import LLMEngine

        with pytest.raises(ValueError, match="Mixtral.*expert_weight_dtype"):
            LLMEngine(_cfg(weight_dtype="fp8_e4m3"))

    def test_both_fields_quantise_attention_too(self):
        from kllms_amd.engine.engine import LLMEngine

        eng = LLMEngine(_cfg(weight_dtype="fp8_e4m3", expert_weight_dtype="fp8_e4m3"))
        ref = LLMEngine(_cfg())
        for layer, rl in zip(eng.model.layers, ref.model.layers):
            for mod, rm in ((layer.self_attn.qkv_proj, rl.self_attn.qkv_proj),
                            (layer.self_attn.o_proj, rl.self_attn.o_proj)):
                assert mod.weight is None
                q, s = ops.quantize_fp8_rows(rm.weight.data)
                assert torch.equal(mod.weight_q.view(torch.uint8), q.view(torch.uint8))
                assert torch.equal(mod.weight_scale, s)
            assert layer.mlp.w_gate_up is None and layer.mlp.w_down is None
            assert torch.equal(layer.mlp.gate.weight, rl.mlp.gate.weight)

    def test_experts_only_leaves_attention_bf16(self):
        from kllms_amd.engine.engine import LLMEngine

        eng = LLMEngine(_cfg(expert_weight_dtype="fp8_e4m3"))
        for layer in eng.model.layers:
            assert layer.self_attn.qkv_proj.weight is not None
            assert layer.self_attn.o_proj.weight is not None
            assert layer.mlp.w_gate_up is None


# --- torch reference vs the float64 oracle ----------------------------------------

@pytest.mark.parametrize("per_expert", [False, True], ids=["shared", "per-expert"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
class TestTorchRefBatched:
    def test_within_kernel_bound(self, shape, per_expert):
        case = eo.batched_case(*shape, per_expert)
        for fn in (ops.linear_fp8w_batched, torch_ref.linear_fp8w_batched):
            out = fn(case["x"], case["q"], case["scale"])
            assert out.dtype == torch.bfloat16 and out.shape == case["e"].shape
            ratio, idx = eo.check(out, case["e"], case["mag"], eo.c_kernel(case["K"]))
            print(f"torch_ref.linear_fp8w_batched [{case['name']}]: worst error/bound "
                  f"{ratio:.3f} at {idx}")
            assert ratio <= 1.0, (case["name"], ratio, idx)

    def test_mutants_exceed_bound(self, shape, per_expert):
        case = eo.batched_case(*shape, per_expert)
        muts = eo.mutants(case)
        assert len(muts) == (2 if case["E"] == 1 else 4 + int(per_expert))
        for name, fn in muts.items():
            bad = fn(case).float().bfloat16()
            ratio, _ = eo.check(bad, case["e"], case["mag"], eo.c_kernel(case["K"]))
            print(f"mutant '{name}' [{case['name']}]: error/bound {ratio:.1f}")
            assert ratio > 1.0, f"bound has no teeth against '{name}' on {case['name']}: {ratio}"

    def test_gateup_bound_and_its_mutants(self, shape, per_expert):
        """The same cases read as a fused [gate; up] product: silu(g) * u from
        the reference's bf16 halves stays within the gate_up bound, every
        mutant (and the swapped gate/up scales) exceeds it."""
        case = eo.batched_case(*shape, per_expert)
        e, mag = eo.gateup_from(case["e"], case["mag"])
        c = eo.c_kernel(case["K"])
        out = torch_ref.linear_fp8w_batched(case["x"].float(), case["q"], case["scale"])
        IN = out.shape[-1] // 2
        got = (torch.nn.functional.silu(out[..., :IN]) * out[..., IN:]).bfloat16()
        ratio, idx = eo.check(got, e, mag, c)
        print(f"gate_up via torch_ref [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
        assert ratio <= 1.0, (case["name"], ratio, idx)
        muts = dict(eo.mutants(case))
        muts["gate and up scales swapped"] = eo.gateup_scales_swapped
        for name, fn in muts.items():
            bad = eo.gateup_from(fn(case), case["mag"])[0].float().bfloat16()
            ratio, _ = eo.check(bad, e, mag, c)
            print(f"gate_up mutant '{name}' [{case['name']}]: error/bound {ratio:.1f}")
            assert ratio > 1.0, f"gate_up bound has no teeth against '{name}' on {case['name']}"


@pytest.mark.parametrize("K", [64, 1088])
def test_grouped_cases_have_teeth(K):
    """The grouped-kernel cases of the GPU tests: the swapped-scales mutant
    exceeds the gate_up bound, and a down output with the scales of the
    previous expert exceeds the down bound."""
    gu = eo.grouped_gateup_case(K)
    ratio, _ = eo.check(gu["e_scales_swapped"].float().bfloat16(), gu["e"], gu["mag"], eo.c_kernel(K))
    assert ratio > 1.0
    dn = eo.grouped_down_case(K)
    bad = torch.zeros_like(dn["e"])
    for i in range(4):
        lo, hi = eo.GROUPED_PAD_OFFSETS[i], eo.GROUPED_PAD_OFFSETS[i + 1]
        if hi > lo:
            bad[lo:hi] = eo.fo.oracle(dn["act"][lo:hi], dn["q"][i], dn["scale"][i],
                                      scale_used=dn["scale"][i - 1])[0]
    ratio, _ = eo.check(bad.float().bfloat16(), dn["e"], dn["mag"], eo.c_kernel(K))
    assert ratio > 1.0


# --- engine -----------------------------------------------------------------------

def test_engine_quantised():
    from kllms_amd.engine.engine import GenRequest, LLMEngine
    from kllms_amd.engine.sampling import SamplingParams

    ref = LLMEngine(_cfg())
    eng = LLMEngine(_cfg(expert_weight_dtype="fp8_e4m3"))
    a = eng.arch
    E, I, H = a.num_experts, a.intermediate_size, a.hidden_size
    elem = ref.model.embed_tokens.weight.element_size()
    for li, (layer, rl) in enumerate(zip(eng.model.layers, ref.model.layers)):
        m, r = layer.mlp, rl.mlp
        assert m.w_gate_up is None and m.w_down is None, li
        names = dict(m.named_parameters())
        assert "w_gate_up" not in names and "w_down" not in names, li
        for name, out_ch in (("w_gate_up", 2 * I), ("w_down", H)):
            full = getattr(r, name).data
            q, s = getattr(m, name + "_q"), getattr(m, name + "_scale")
            assert q.dtype == torch.float8_e4m3fn and q.shape == full.shape, (li, name)
            assert s.dtype == torch.float32 and s.shape == (E, out_ch), (li, name)
            for e in range(E):
                wq, ws = ops.quantize_fp8_rows(full[e])
                assert torch.equal(q[e].view(torch.uint8), wq.view(torch.uint8)), (li, name, e)
                assert torch.equal(s[e], ws), (li, name, e)
            held = q.numel() * q.element_size() + s.numel() * 4
            # half the bf16 bytes (the CPU engine holds fp32: a quarter) + 4 B per channel
            assert held <= full.numel() * elem * (1.0 / elem) + 4 * E * out_ch, (li, name)
        assert torch.equal(m.gate.weight, r.gate.weight)
        assert m.gate.weight.dtype == r.gate.weight.dtype
        assert layer.self_attn.qkv_proj.weight is not None
    assert torch.equal(eng.model.embed_tokens.weight, ref.model.embed_tokens.weight)
    assert torch.equal(eng.model.lm_head.weight, ref.model.lm_head.weight)

    out = eng.generate([GenRequest(prompt_ids=list(range(1, 40)), n=3,
                                   sampling=SamplingParams(temperature=1.0, max_tokens=8, seed=2))])[0]
    assert len(out.streams) == 3
    for s in out.streams:
        assert len(s.token_ids) > 0
        assert all(np.isfinite(lp) for lp in s.logprobs)


def test_quantised_dense_path_matches_grouped():
    """As ``test_mixtral.test_dense_path_matches_grouped`` (same weights, input
    and tolerance), on the quantised module."""
    from kllms_amd.engine.config import MODEL_PRESETS
    from kllms_amd.models.mixtral import MixtralMoE
    from kllms_amd.parallel.tp import ParallelContext

    cfg = MODEL_PRESETS["tiny-mixtral"]
    moe = MixtralMoE(cfg, ParallelContext(), dtype=torch.float32)
    torch.manual_seed(3)
    moe.gate.weight.copy_(torch.randn_like(moe.gate.weight) * 0.2)
    moe.w_gate_up.copy_(torch.randn_like(moe.w_gate_up) * 0.1)
    moe.w_down.copy_(torch.randn_like(moe.w_down) * 0.1)
    moe.quantize_fp8_()
    assert moe.quantized and moe.w_gate_up is None
    x = torch.randn(11, cfg.hidden_size)
    probs = torch.softmax(moe.gate(x).float(), dim=-1)
    topw, topi = torch.topk(probs, moe.k, dim=-1)
    topw = topw / topw.sum(dim=-1, keepdim=True)
    dense = moe._forward_dense(x, topw, topi)
    grouped = moe._forward_grouped(x, topw, topi)
    assert torch.isfinite(dense).all()
    assert torch.allclose(dense, grouped, atol=1e-4), (dense - grouped).abs().max()
    moe.quantize_fp8_()     # a second call is a no-op
    assert torch.equal(moe._forward_dense(x, topw, topi), dense)


# --- TP invariance (gloo, world size 2) ---------------------------------------------

def _prefill_logits(eng, ids):
    from kllms_amd.models.llama import ForwardBatch

    seq = eng.kv.alloc_sequence(len(ids))
    batch = ForwardBatch(
        mode="prefill",
        positions=torch.arange(len(ids)),
        slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq)),
        kv_caches=eng.kv.layer_caches(),
        cu_seqlens=torch.tensor([0, len(ids)], dtype=torch.int32),
    )
    logits = eng.model.forward_prefill(torch.tensor(ids), batch)
    eng.kv.free_sequence(seq)
    return logits


def _expert_tensors(eng):
    out = {}
    for i, layer in enumerate(eng.model.layers):
        for name in ("w_gate_up", "w_down"):
            q = getattr(layer.mlp, name + "_q")
            s = getattr(layer.mlp, name + "_scale")
            out[f"layers.{i}.{name}"] = (q.view(torch.uint8).numpy().tobytes(), tuple(q.shape),
                                         s.numpy().tobytes(), tuple(s.shape))
    return out


def _tp_worker(rank: int, world_size: int, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(PORT)
    os.environ.pop("KLLMS_WEIGHT_DTYPE", None)
    os.environ.pop("KLLMS_EXPERT_WEIGHT_DTYPE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from kllms_amd.engine.engine import LLMEngine
        from kllms_amd.parallel.tp import ParallelContext

        eng = LLMEngine(_cfg(tp_size=world_size, max_kv_blocks=128, expert_weight_dtype="fp8_e4m3"),
                        parallel_ctx=ParallelContext(world_size=world_size, rank=rank))
        logits = _prefill_logits(eng, list(range(1, 41)))   # 40 rows > 8 * E: grouped path
        q.put((rank, _expert_tensors(eng), logits.detach().numpy().tobytes(), tuple(logits.shape)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_tp2_expert_quantisation_is_tp_invariant():
    from kllms_amd.engine.engine import LLMEngine

    ctx = mp.get_context("spawn")
    qu = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, qu)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, tensors, buf, shape = qu.get(timeout=240)
        results[rank] = (tensors, np.frombuffer(buf, dtype=np.float32).reshape(shape))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    eng = LLMEngine(_cfg(max_kv_blocks=128, expert_weight_dtype="fp8_e4m3"))
    I = eng.arch.intermediate_size
    for i, layer in enumerate(eng.model.layers):
        for name in ("w_gate_up", "w_down"):
            full_q = getattr(layer.mlp, name + "_q").view(torch.uint8)
            full_s = getattr(layer.mlp, name + "_scale")
            for rank in range(2):
                qb, qshape, sb, sshape = results[rank][0][f"layers.{i}.{name}"]
                got_q = torch.frombuffer(bytearray(qb), dtype=torch.uint8).reshape(qshape)
                got_s = torch.frombuffer(bytearray(sb), dtype=torch.float32).reshape(sshape)
                if name == "w_gate_up":     # per-part ([gate; up]) row slices
                    sz = I // 2
                    rows = torch.cat([torch.arange(rank * sz, (rank + 1) * sz),
                                      I + torch.arange(rank * sz, (rank + 1) * sz)])
                    want_q, want_s = full_q[:, rows], full_s[:, rows]
                else:                       # column slice, scales of the whole row
                    kk = I // 2
                    want_q, want_s = full_q[:, :, rank * kk:(rank + 1) * kk], full_s
                assert torch.equal(got_q, want_q), f"layer {i} {name} rank {rank}: q differs from TP=1 slice"
                assert torch.equal(got_s, want_s), f"layer {i} {name} rank {rank}: scale differs from TP=1"

    np.testing.assert_allclose(results[0][1], results[1][1], rtol=1e-4, atol=1e-4)
    logits_tp1 = _prefill_logits(eng, list(range(1, 41)))
    np.testing.assert_allclose(results[0][1], logits_tp1.detach().numpy(), rtol=2e-3, atol=2e-3)
