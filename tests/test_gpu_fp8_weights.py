"""Weight-only fp8 (e4m3) GEMM on the GPU: the HIP kernel, the large-M
dequant path and the quantised engine.

Run on an MI355X box: python -m pytest tests/test_gpu_fp8_weights.py -m gpu -q

Kernel outputs are held to the float64 oracle of ``fp8w_oracles`` under its
derived bounds (kernel path c = K * 2^-23, large-M path c = 2^-9 + K * 2^-23);
each test prints its worst error/bound ratio before asserting.
"""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import fp8w_oracles as fo
from kllms_amd import ops

DEV = "cuda:0"

# (M, N, K): a single k-step; 17 k-steps (odd, so every K split is uneven);
# two row tiles; four row tiles with a 2-way split; the largest M over 32
# column tiles and two row blocks
EDGE_SHAPES = [(1, 64, 64), (7, 80, 1088), (33, 96, 1088), (120, 160, 2048), (256, 4096, 512)]


def _dev(case):
    buf = case["buf"].to(DEV)
    K = case["K"]
    x = buf[:, :K]
    b = case["bias"].to(DEV) if case["bias"] is not None else None
    return x, case["q"].to(DEV), case["scale"].to(DEV), b


def _canon_zero(t):
    """bf16 bits with -0 mapped to +0."""
    return (t + 0.0).view(torch.int16)


class TestExactConversion:
    def _operands(self):
        N, K = 96, 128
        codes = fo.all_finite_bytes()
        idx = (torch.arange(N).unsqueeze(1) * 131 + torch.arange(K).unsqueeze(0) * 7) % 254
        raw = codes[idx]                                       # [N, K] uint8, asymmetric
        assert len(set(raw.reshape(-1).tolist())) == 254
        q = raw.view(torch.float8_e4m3fn)
        scale = (0.0137 * (1.0 + 0.173 * torch.arange(N).float())).float()
        return q, scale

    def test_identity_all_finite_bytes(self):
        """x = I (128 x 128): out[k, n] must be bf16(fp32(q[n, k]) * scale[n])
        bit for bit, for all 254 finite e4m3 bytes (subnormals, +-448, zeros).

        The sign of a ZERO output is excepted: the definition's sum over k
        holds the exact zeros 0 * q[n, k'] of both signs, whose IEEE sum is
        +0 whatever the byte's sign, so 0x80 legitimately comes out as +0.
        Both sides are compared with -0 canonicalised to +0."""
        q, scale = self._operands()
        x = torch.eye(128, dtype=torch.bfloat16, device=DEV)
        out = ops.linear_fp8w(x, q.to(DEV), scale.to(DEV))
        want = (q.float() * scale.unsqueeze(1)).t().contiguous().bfloat16()
        got = out.cpu()
        assert got.shape == (128, 96)
        bad = _canon_zero(got) != _canon_zero(want)
        print(f"exact conversion: {int(bad.sum())} of {bad.numel()} elements differ")
        assert not bad.any(), f"first mismatch at (k, n) = {tuple(bad.nonzero()[0].tolist())}"
        # and a zero byte gives a zero, never a tiny value
        assert (got[want == 0] == 0).all()

    def test_dequant_all_finite_bytes(self):
        from kllms_amd import _C

        q, scale = self._operands()
        w = torch.full((96 * 128 + 64,), 7.0, dtype=torch.bfloat16, device=DEV)
        _C.dequant_fp8w(w, q.to(DEV), scale.to(DEV))
        want = (q.float() * scale.unsqueeze(1)).bfloat16()
        got = w.cpu()
        assert torch.equal(got[: 96 * 128].view(torch.int16), want.reshape(-1).view(torch.int16))
        assert (got[96 * 128:] == 7.0).all(), "dequant wrote past N*K"


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_within_bound(shape, bias):
    case = fo.gemm_case(*shape, bias=bias)
    x, q, scale, b = _dev(case)
    assert ops._fp8w_kernel_takes(x, q.shape[0], q.shape[1])
    out = ops.linear_fp8w(x, q, scale, b)
    ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_kernel(case["K"]))
    print(f"linear_fp8w kernel [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (case["name"], ratio, idx)


@pytest.mark.parametrize("shape", [(65, 32768, 64), (65, 16384, 1088)],
                         ids=lambda s: "x".join(map(str, s)))
def test_kernel_128_row_blocks(shape):
    """M > 64 runs 128-row blocks only when the grid fills the card (256
    column tiles here; 128 tiles x a 2-way K split), 64-row blocks otherwise,
    as in every M > 64 case above: these two shapes reach the 128-row kernel,
    without and with split-K."""
    case = fo.gemm_case(*shape, bias=True)
    x, q, scale, b = _dev(case)
    out = ops.linear_fp8w(x, q, scale, b)
    ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_kernel(case["K"]))
    print(f"linear_fp8w kernel [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (case["name"], ratio, idx)


def test_kernel_row_strided_x():
    case = fo.gemm_case(33, 96, 1088, bias=True, wide=True)
    x, q, scale, b = _dev(case)
    assert not x.is_contiguous() and x.stride(0) == 1088 + 24
    assert ops._fp8w_kernel_takes(x, 96, 1088)
    out = ops.linear_fp8w(x, q, scale, b)
    ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_kernel(1088))
    print(f"linear_fp8w kernel [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (ratio, idx)


def test_nothing_written_outside():
    from kllms_amd import _C

    case = fo.gemm_case(33, 96, 1088, bias=False)
    x, q, scale, _ = _dev(case)
    buf = torch.full((64, 96), -777.0, dtype=torch.bfloat16, device=DEV)
    _C.linear_fp8w(buf[:33], x, q, scale, torch.empty(0, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()
    assert (buf[33:] == -777.0).all(), "rows >= M were written"
    ratio, idx = fo.check(buf[:33], case["e"], case["mag"], fo.c_kernel(1088))
    assert ratio <= 1.0, (ratio, idx)


@pytest.mark.parametrize("shape", [(120, 160, 2048), (7, 80, 1088)],
                         ids=lambda s: "x".join(map(str, s)))
def test_deterministic(shape):
    case = fo.gemm_case(*shape, bias=True)
    x, q, scale, b = _dev(case)
    a = ops.linear_fp8w(x, q, scale, b)
    c = ops.linear_fp8w(x, q, scale, b)
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


@pytest.mark.parametrize("M", [257, 300])
def test_large_m_path(M):
    case = fo.gemm_case(M, 160, 1088, bias=True)
    x, q, scale, b = _dev(case)
    assert not ops._fp8w_kernel_takes(x, 160, 1088)
    scratch = torch.empty(160 * 1088 + 128, dtype=torch.bfloat16, device=DEV)
    out = ops.linear_fp8w(x, q, scale, b, scratch=scratch)
    ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_large_m(1088))
    print(f"linear_fp8w large-M [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (ratio, idx)
    # no scratch given: same result
    out2 = ops.linear_fp8w(x, q, scale, b)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


def test_unsupported_k_takes_fallback():
    """K = 80 is a multiple of 16 but not of 64: the kernel must refuse it
    and ops must route it through the dequant path, within that path's bound."""
    from kllms_amd import _C

    case = fo.gemm_case(33, 96, 80, bias=True)
    x, q, scale, b = _dev(case)
    assert not ops._fp8w_kernel_takes(x, 96, 80)
    with pytest.raises(RuntimeError, match="K % 64"):
        _C.linear_fp8w(torch.empty(33, 96, dtype=torch.bfloat16, device=DEV), x, q, scale, b)
    out = ops.linear_fp8w(x, q, scale, b)
    ratio, idx = fo.check(out, case["e"], case["mag"], fo.c_large_m(80))
    print(f"linear_fp8w fallback [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (ratio, idx)


# --- engine -----------------------------------------------------------------------

def _engine(model, graphs):
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    return LLMEngine(EngineConfig(model=model, max_kv_blocks=512, use_hip_graphs=graphs, seed=3,
                                  weight_dtype="fp8_e4m3"))


def _forced_torch(fn):
    os.environ["KLLMS_AMD_FORCE_TORCH_OPS"] = "1"
    try:
        return fn()
    finally:
        del os.environ["KLLMS_AMD_FORCE_TORCH_OPS"]


def _close(a, ref, what):
    diff = (a - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: max|d| {diff:.4f}, max|ref| {scale:.3f}")
    assert diff < 0.05 * max(scale, 1.0), f"{what} diverge: {diff} vs scale {scale}"


@pytest.mark.parametrize("model", ["mid-llama", "mid-qwen"])
class TestEngineFp8Weights:
    def test_prefill_logits_match_forced_torch(self, model, monkeypatch):
        from kllms_amd.models.llama import ForwardBatch

        monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
        eng = _engine(model, graphs=False)
        layer = eng.model.layers[0]
        assert layer.self_attn.qkv_proj.weight is None
        assert layer.mlp.down_proj.weight_q.dtype == torch.float8_e4m3fn
        assert layer.mlp.down_proj.fp8_scratch is layer.self_attn.qkv_proj.fp8_scratch
        assert eng.model.lm_head.weight.dtype == torch.bfloat16

        for T in (150, 300):   # kernel path (M <= 256) and large-M path
            ids = torch.randint(0, 2000, (T,), device=DEV)

            def run_prefill():
                seq = eng.kv.alloc_sequence(T)
                batch = ForwardBatch(
                    mode="prefill",
                    positions=torch.arange(T, device=DEV),
                    slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
                    kv_caches=eng.kv.layer_caches(),
                    cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device=DEV),
                )
                logits = eng.model.forward_prefill(ids, batch)
                eng.kv.free_sequence(seq)
                return logits

            _close(run_prefill(), _forced_torch(run_prefill), f"{model} prefill logits T={T}")

    def test_decode_step_graph_and_eager_match_forced_torch(self, model, monkeypatch):
        from kllms_amd.models.llama import ForwardBatch

        monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
        eng = _engine(model, graphs=True)
        B, L = 4, 40
        bs = eng.kv.block_size
        seqs = [eng.kv.alloc_sequence(L + 1) for _ in range(B)]
        g = torch.Generator().manual_seed(5)
        prompt = torch.randint(0, 2000, (B * L,), generator=g).to(DEV)
        slots = [s.blocks[p // bs] * bs + p % bs for s in seqs for p in range(L)]
        pre = ForwardBatch(
            mode="prefill",
            positions=torch.arange(L, device=DEV).repeat(B),
            slot_mapping=torch.tensor(slots, device=DEV),
            kv_caches=eng.kv.layer_caches(),
            cu_seqlens=torch.tensor([i * L for i in range(B + 1)], dtype=torch.int32, device=DEV),
        )
        eng.model.forward_prefill(prompt, pre)

        ids = torch.randint(0, 2000, (B,), generator=g).to(DEV)
        batch = ForwardBatch(
            mode="decode",
            positions=torch.full((B,), L, dtype=torch.long, device=DEV),
            slot_mapping=torch.tensor([s.blocks[L // bs] * bs + L % bs for s in seqs], device=DEV),
            kv_caches=eng.kv.layer_caches(),
            block_tables=torch.tensor([s.blocks for s in seqs], dtype=torch.int32, device=DEV),
            context_lens=torch.full((B,), L + 1, dtype=torch.int32, device=DEV),
        )
        # under inference_mode, as generate() runs it (capture touches the
        # default generator's state, an inference tensor once generate() ran)
        with torch.inference_mode():
            ref = _forced_torch(lambda: eng.model.forward_decode(ids, batch))
            eager = eng.model.forward_decode(ids, batch)
            graph = eng._graph_runner.run(ids, batch)
            replay = eng._graph_runner.run(ids, batch).clone()
        assert eng._graph_runner._enabled, "hipGraph capture of the fp8 GEMM failed"
        _close(eager, ref, f"{model} eager decode logits")
        _close(graph, ref, f"{model} graph decode logits")
        assert torch.equal(graph, replay)
        for s in seqs:
            eng.kv.free_sequence(s)

    def test_generate_with_graphs(self, model, monkeypatch):
        from kllms_amd.engine.engine import GenRequest
        from kllms_amd.engine.sampling import SamplingParams

        monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)
        eng = _engine(model, graphs=True)
        out = eng.generate([
            GenRequest(prompt_ids=list(range(1, 80)), n=4,
                       sampling=SamplingParams(temperature=1.0, max_tokens=24, seed=5))
        ])[0]
        assert eng._graph_runner._enabled
        assert len(out.streams) == 4
        for s in out.streams:
            assert len(s.token_ids) > 0
            assert all(np.isfinite(lp) for lp in s.logprobs)


def test_gpu_engine_needs_bf16():
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    with pytest.raises(ValueError, match="bfloat16"):
        LLMEngine(EngineConfig(model="mid-llama", max_kv_blocks=64, use_hip_graphs=False,
                               dtype="float16", weight_dtype="fp8_e4m3"))
