"""Opt-in fp8 (e4m3) weights, CPU side: the quantiser, the torch reference of
the weight-only GEMM against a float64 oracle with a derived bound (and
mutants that must break it), the config/env plumbing, the quantised engine,
and TP-degree invariance over gloo.
"""

import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

import fp8w_oracles as fo
from kllms_amd import ops
from kllms_amd.ops import torch_ref

PORT = 29853
SHAPES = [(1, 64, 64), (33, 96, 1088), (120, 160, 2048)]


# --- quantiser ------------------------------------------------------------------

class TestQuantizer:
    def _w(self):
        g = torch.Generator().manual_seed(1)
        w = (torch.randn(12, 96, generator=g) * 0.02).bfloat16()
        w[3] = 0
        w[5, 17] = 800.0
        w[7, 2] = -1.5
        return w

    def test_scale_formula_and_zero_row(self):
        w = self._w()
        q, scale = ops.quantize_fp8_rows(w)
        assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape and q.is_contiguous()
        assert scale.dtype == torch.float32 and scale.shape == (12,)
        want = w.float().abs().amax(1) / 448.0
        want[3] = 1.0
        assert torch.equal(scale, want)
        assert scale[3].item() == 1.0
        assert torch.equal(q[3].float(), torch.zeros(96))

    def test_no_nan_bytes_and_rne(self):
        w = self._w()
        q, scale = ops.quantize_fp8_rows(w)
        raw = q.view(torch.uint8)
        assert not ((raw & 0x7F) == 0x7F).any(), "NaN encodings produced"
        # every code is the nearest e4m3 value to w / scale: no other finite
        # code is strictly closer
        t = (w.float() / scale.unsqueeze(1)).double()
        codes = fo.all_finite_bytes().view(torch.float8_e4m3fn).float().double()
        best = (t.unsqueeze(-1) - codes).abs().amin(-1)
        assert torch.equal((t - q.float().double()).abs(), best)
        # a value that would round past 448 is clamped, not turned into NaN
        q2, _ = ops.quantize_fp8_rows(torch.tensor([[1.0, -1.0, 0.999]]), amax=torch.tensor([0.9]))
        assert q2.float().tolist() == [[448.0, -448.0, 448.0]]

    def test_outlier_round_trip(self):
        w = self._w()
        q, scale = ops.quantize_fp8_rows(w)
        deq = q.float() * scale.unsqueeze(1)
        for n in range(12):
            k = int(w[n].float().abs().argmax())
            ref = w[n, k].float().item()
            assert abs(deq[n, k].item() - ref) <= 2.0 ** -4 * abs(ref), (n, k)
        assert abs(deq[5, 17].item() - 800.0) <= 2.0 ** -4 * 800.0

    def test_amax_override(self):
        w = self._w()
        amax = w.float().abs().amax(1) * 2
        _, scale = ops.quantize_fp8_rows(w, amax)
        want = amax / 448.0
        want[3] = 1.0
        assert torch.equal(scale, want)


# --- torch reference vs the float64 oracle ----------------------------------------

@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
class TestTorchRef:
    def test_within_kernel_bound(self, shape, bias):
        case = fo.gemm_case(*shape, bias=bias)
        out = ops.linear_fp8w(case["x"], case["q"], case["scale"], case["bias"])
        assert out.dtype == case["x"].dtype
        ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_kernel(case["K"]))
        print(f"torch_ref.linear_fp8w [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
        assert ratio <= 1.0, (case["name"], ratio, idx)

    def test_mutants_exceed_bound(self, shape, bias):
        case = fo.gemm_case(*shape, bias=bias)
        for name, fn in fo.MUTANTS.items():
            bad = fn(case).float().bfloat16()
            ratio, _ = fo.check(bad, case["e"], case["mag"], fo.c_kernel(case["K"]))
            print(f"mutant '{name}' [{case['name']}]: error/bound {ratio:.1f}")
            assert ratio > 1.0, f"bound has no teeth against '{name}' on {case['name']}: {ratio}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16])
def test_torch_ref_any_float_dtype(dtype):
    case = fo.gemm_case(7, 64, 128, bias=True)
    x = case["x"].to(dtype)
    out = torch_ref.linear_fp8w(x, case["q"], case["scale"], case["bias"].to(dtype))
    assert out.dtype == dtype
    e, mag = fo.oracle(x, case["q"], case["scale"], case["bias"].to(dtype))
    tol = {torch.float64: 1e-12, torch.float32: 1e-5, torch.float16: 2e-3}[dtype]
    assert ((out.double() - e).abs() <= tol * (mag + 1.0)).all()


# --- config -----------------------------------------------------------------------

def _cfg(**kw):
    from kllms_amd.engine.config import EngineConfig

    base = dict(model="tiny-llama", max_kv_blocks=64, use_hip_graphs=False, device="cpu", seed=0)
    base.update(kw)
    return EngineConfig(**base)


def _projections(eng):
    for i, layer in enumerate(eng.model.layers):
        for name, mod in (("qkv", layer.self_attn.qkv_proj), ("o", layer.self_attn.o_proj),
                          ("gate_up", layer.mlp.gate_up_proj), ("down", layer.mlp.down_proj)):
            yield f"layers.{i}.{name}", mod


class TestConfig:
    def test_field_accepted_and_validated(self):
        assert _cfg().weight_dtype == "bf16"
        assert _cfg(weight_dtype="fp8_e4m3").weight_dtype == "fp8_e4m3"
        with pytest.raises(ValueError):
            _cfg(weight_dtype="int8")

    def test_env_overrides(self, monkeypatch):
        from kllms_amd.engine.engine import LLMEngine

        monkeypatch.setenv("KLLMS_WEIGHT_DTYPE", "fp8_e4m3")
        eng = LLMEngine(_cfg())
        assert eng.weight_dtype == "fp8_e4m3"
        assert all(m.weight is None for _, m in _projections(eng))
        monkeypatch.setenv("KLLMS_WEIGHT_DTYPE", "bf16")
        eng = LLMEngine(_cfg(weight_dtype="fp8_e4m3"))
        assert eng.weight_dtype == "bf16"
        assert all(m.weight is not None for _, m in _projections(eng))

    def test_env_rejects_bad_value(self, monkeypatch):
        from kllms_amd.engine.engine import LLMEngine

        monkeypatch.setenv("KLLMS_WEIGHT_DTYPE", "fp8")
        with pytest.raises(ValueError, match="KLLMS_WEIGHT_DTYPE"):
            LLMEngine(_cfg())

    def test_mixtral_raises(self):
        from kllms_amd.engine.engine import LLMEngine

        with pytest.raises(ValueError, match="Mixtral"):
            LLMEngine(_cfg(model="tiny-mixtral", weight_dtype="fp8_e4m3"))

    def test_default_unchanged(self, monkeypatch):
        from kllms_amd.engine.engine import LLMEngine

        monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
        eng = LLMEngine(_cfg())
        for _, m in _projections(eng):
            assert m.weight is not None and not hasattr(m, "weight_q")


# --- engine -----------------------------------------------------------------------

@pytest.mark.parametrize("model", ["tiny-llama", "tiny-qwen"])
def test_engine_quantised(model, monkeypatch):
    from kllms_amd.engine.engine import GenRequest, LLMEngine
    from kllms_amd.engine.sampling import SamplingParams

    monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
    ref = LLMEngine(_cfg(model=model))
    eng = LLMEngine(_cfg(model=model, weight_dtype="fp8_e4m3"))
    elem = ref.model.embed_tokens.weight.element_size()
    n_proj = 0
    for (name, m), (_, r) in zip(_projections(eng), _projections(ref)):
        n_proj += 1
        assert m.weight is None, name
        assert "weight" not in dict(m.named_parameters()), name
        assert m.weight_q.dtype == torch.float8_e4m3fn and m.weight_q.shape == r.weight.shape, name
        assert m.weight_scale.dtype == torch.float32, name
        assert m.weight_scale.shape == (r.weight.shape[0],), name
        # the quantised weights ARE the quantiser's output on the bf16-engine's weights
        q, s = ops.quantize_fp8_rows(r.weight.data)
        assert torch.equal(m.weight_q.view(torch.uint8), q.view(torch.uint8)), name
        assert torch.equal(m.weight_scale, s), name
        N = r.weight.shape[0]
        held = m.weight_q.numel() * m.weight_q.element_size() + m.weight_scale.numel() * 4
        assert held <= r.weight.numel() * elem * (1.0 / elem) + 4 * N, name
        if getattr(r, "bias", None) is not None:
            assert torch.equal(m.bias, r.bias), name
    assert n_proj == 4 * eng.arch.num_layers
    # embed_tokens / lm_head untouched
    assert torch.equal(eng.model.embed_tokens.weight, ref.model.embed_tokens.weight)
    assert torch.equal(eng.model.lm_head.weight, ref.model.lm_head.weight)
    assert eng.model.lm_head.weight.dtype == ref.model.lm_head.weight.dtype
    if eng.arch.attention_qkv_bias:
        assert eng.model.layers[0].self_attn.qkv_proj.bias is not None

    out = eng.generate([GenRequest(prompt_ids=list(range(1, 40)), n=3,
                                   sampling=SamplingParams(temperature=1.0, max_tokens=8, seed=2))])[0]
    assert len(out.streams) == 3
    for s in out.streams:
        assert len(s.token_ids) > 0
        assert all(np.isfinite(lp) for lp in s.logprobs)


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


def _tp_fp8w_worker(rank: int, world_size: int, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(PORT)
    os.environ.pop("KLLMS_WEIGHT_DTYPE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from kllms_amd.engine.engine import LLMEngine
        from kllms_amd.parallel.tp import ParallelContext

        eng = LLMEngine(_cfg(model="tiny-llama-kv4", tp_size=world_size, max_kv_blocks=128,
                             weight_dtype="fp8_e4m3"),
                        parallel_ctx=ParallelContext(world_size=world_size, rank=rank))
        weights = {name: (m.weight_q.view(torch.uint8).numpy().tobytes(), tuple(m.weight_q.shape),
                          m.weight_scale.numpy().tobytes())
                   for name, m in _projections(eng)}
        logits = _prefill_logits(eng, list(range(1, 33)))
        q.put((rank, weights, logits.detach().numpy().tobytes(), tuple(logits.shape)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_tp2_quantisation_is_tp_invariant(monkeypatch):
    from kllms_amd.engine.engine import LLMEngine
    from kllms_amd.parallel.tp import ColumnParallelLinear

    monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
    ctx = mp.get_context("spawn")
    qu = ctx.Queue()
    procs = [ctx.Process(target=_tp_fp8w_worker, args=(r, 2, qu)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, weights, buf, shape = qu.get(timeout=240)
        results[rank] = (weights, np.frombuffer(buf, dtype=np.float32).reshape(shape))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    eng = LLMEngine(_cfg(model="tiny-llama-kv4", max_kv_blocks=128, weight_dtype="fp8_e4m3"))
    for name, m in _projections(eng):
        full_q = m.weight_q.view(torch.uint8)
        full_s = m.weight_scale
        for rank in range(2):
            qb, qshape, sb = results[rank][0][name]
            got_q = torch.frombuffer(bytearray(qb), dtype=torch.uint8).reshape(qshape)
            got_s = torch.frombuffer(bytearray(sb), dtype=torch.float32)
            if isinstance(m, ColumnParallelLinear):
                rows = []
                off = 0
                for part in m.partition_sizes:
                    sz = part // 2
                    rows.extend(range(off + rank * sz, off + (rank + 1) * sz))
                    off += part
                rows = torch.tensor(rows)
                want_q, want_s = full_q[rows], full_s[rows]
            else:
                kk = full_q.shape[1] // 2
                want_q, want_s = full_q[:, rank * kk:(rank + 1) * kk], full_s
            assert torch.equal(got_q, want_q), f"{name} rank {rank}: weight_q differs from TP=1 slice"
            assert torch.equal(got_s, want_s), f"{name} rank {rank}: weight_scale differs from TP=1"

    np.testing.assert_allclose(results[0][1], results[1][1], rtol=1e-4, atol=1e-4)
    logits_tp1 = _prefill_logits(eng, list(range(1, 33)))
    np.testing.assert_allclose(results[0][1], logits_tp1.detach().numpy(), rtol=2e-3, atol=2e-3)
