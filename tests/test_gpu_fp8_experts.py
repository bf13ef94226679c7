"""fp8 (e4m3) Mixtral expert weights on the GPU: the batched weight-only GEMM,
the fp8 instantiations of the grouped MoE kernels, the quantised module and the
quantised engine.

Run on an MI355X box: python -m pytest tests/test_gpu_fp8_experts.py -m gpu -q

Kernel outputs are held to the float64 oracles of ``fp8_expert_oracles`` under
their derived bounds; each test prints its worst error/bound ratio before
asserting.
"""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import fp8_expert_oracles as eo
import fp8w_oracles as fo
from kllms_amd import ops

DEV = "cuda:0"

# (E, M, N, K, per-expert x): a single k-step; N < 128, so an expert's clamped
# rows and dropped columns sit next to the neighbouring expert; two row tiles,
# odd E, 17 uneven k-stages; M = 8 * E; the 128-row block path
BATCHED_CASES = [(1, 1, 64, 64, False), (4, 7, 80, 1088, False), (3, 33, 96, 1088, True),
                 (8, 64, 256, 2048, True), (2, 65, 128, 512, True)]


def _dev(case):
    buf = case["buf"].to(DEV)
    x = buf[:, :case["M"], :case["K"]] if buf.dim() == 3 else buf
    return x, case["q"].to(DEV), case["scale"].to(DEV)


def _report(what, case, out, c):
    ratio, idx = eo.check(out, case["e"], case["mag"], c)
    print(f"{what} [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (case["name"], ratio, idx)


# --- the batched kernel -------------------------------------------------------------

@pytest.mark.parametrize("shape", BATCHED_CASES, ids=lambda s: "x".join(map(str, map(int, s))))
def test_batched_kernel_within_bound(shape):
    case = eo.batched_case(*shape)
    x, q, scale = _dev(case)
    assert ops._fp8w_batched_kernel_takes(x, *q.shape)
    out = ops.linear_fp8w_batched(x, q, scale)
    assert out.shape == case["e"].shape and out.dtype == torch.bfloat16
    _report("linear_fp8w_batched kernel", case, out, eo.c_kernel(case["K"]))


def test_batched_kernel_128_row_blocks():
    """M > 64 runs 128-row blocks only when the grid fills the card, 64-row
    blocks otherwise (as (2, 65, 128, 512) above does on a card with more than
    two CUs): 2 experts x 128 column tiles reach the 128-row batched kernel."""
    case = eo.batched_case(2, 65, 16384, 64, True)
    x, q, scale = _dev(case)
    out = ops.linear_fp8w_batched(x, q, scale)
    _report("linear_fp8w_batched kernel", case, out, eo.c_kernel(64))


@pytest.mark.parametrize("shape", [(7, 80, 1088), (120, 160, 2048)],
                         ids=lambda s: "x".join(map(str, s)))
def test_one_expert_is_linear_fp8w_bit_for_bit(shape):
    case = fo.gemm_case(*shape, bias=False)
    x, q, scale = case["x"].to(DEV), case["q"].to(DEV), case["scale"].to(DEV)
    want = ops.linear_fp8w(x, q, scale)
    for xb in (x, x.unsqueeze(0)):
        got = ops.linear_fp8w_batched(xb, q.unsqueeze(0), scale.unsqueeze(0))
        assert got.shape == (1,) + tuple(want.shape)
        assert torch.equal(got[0].view(torch.int16), want.view(torch.int16))


def test_batched_kernel_strided_x():
    case = eo.batched_case(3, 33, 96, 1088, True, wide=True)
    x, q, scale = _dev(case)
    assert not x.is_contiguous()
    assert x.stride(1) == 1088 + 24 and x.stride(0) == (33 + 3) * (1088 + 24)
    assert ops._fp8w_batched_kernel_takes(x, *q.shape)
    out = ops.linear_fp8w_batched(x, q, scale)
    _report("linear_fp8w_batched kernel", case, out, eo.c_kernel(1088))


@pytest.mark.parametrize("shape", [(4, 7, 80, 1088, False), (3, 33, 96, 1088, True)],
                         ids=lambda s: "x".join(map(str, map(int, s))))
def test_batched_nothing_written_outside(shape):
    from kllms_amd import _C

    case = eo.batched_case(*shape)
    x, q, scale = _dev(case)
    E, M, N = case["E"], case["M"], case["N"]
    guard = 4096
    buf = torch.full((guard + E * M * N + guard,), -777.0, dtype=torch.bfloat16, device=DEV)
    out = buf[guard:guard + E * M * N].view(E, M, N)
    _C.linear_fp8w_batched(out, x, q, scale)
    torch.cuda.synchronize()
    assert (buf[:guard] == -777.0).all(), "elements before out were written"
    assert (buf[guard + E * M * N:] == -777.0).all(), "elements after out were written"
    _report("linear_fp8w_batched in a guarded buffer", case, out, eo.c_kernel(case["K"]))


@pytest.mark.parametrize("shape", [(4, 7, 80, 1088, False), (8, 64, 256, 2048, True)],
                         ids=lambda s: "x".join(map(str, map(int, s))))
def test_batched_deterministic(shape):
    """Both shapes take split-K on a card with >= 64 CUs (few column tiles)."""
    case = eo.batched_case(*shape)
    x, q, scale = _dev(case)
    a = ops.linear_fp8w_batched(x, q, scale)
    b = ops.linear_fp8w_batched(x, q, scale)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("shape", [(3, 7, 96, 1000), (2, 257, 96, 1088)],
                         ids=lambda s: "x".join(map(str, s)))
def test_batched_fallback(shape):
    """K % 64 != 0 and M > 256 dequantise and run torch.bmm: the large-M bound."""
    for per_expert in (False, True):
        case = eo.batched_case(*shape, per_expert)
        x, q, scale = _dev(case)
        assert not ops._fp8w_batched_kernel_takes(x, *q.shape)
        out = ops.linear_fp8w_batched(x, q, scale)
        _report("linear_fp8w_batched fallback", case, out, eo.c_large_m(case["K"]))


def test_batched_binding_refuses_what_the_kernel_does_not_take():
    from kllms_amd import _C

    case = eo.batched_case(3, 7, 96, 1000, True)
    x, q, scale = _dev(case)
    with pytest.raises(RuntimeError, match="K % 64"):
        _C.linear_fp8w_batched(torch.empty(3, 7, 96, dtype=torch.bfloat16, device=DEV), x, q, scale)


# --- fp8 grouped kernels, op level --------------------------------------------------

@pytest.mark.parametrize("IN", [64, 1088])
def test_fp8_moe_down_within_bound(IN):
    case = eo.grouped_down_case(IN)
    S, H = case["e"].shape
    y = torch.zeros(S, H, dtype=torch.bfloat16, device=DEV)
    pad = torch.tensor(eo.GROUPED_PAD_OFFSETS, dtype=torch.int32, device=DEV)
    ops.moe_down(y, case["act"].to(DEV), case["q"].to(DEV), pad, scale=case["scale"].to(DEV))
    _report("fp8 moe_down", case, y, eo.c_kernel(IN))


@pytest.mark.parametrize("K", [64, 1088])
def test_fp8_moe_gateup_within_bound(K):
    case = eo.grouped_gateup_case(K)
    S, IN = case["e"].shape
    act = torch.full((S, IN), 3.0, dtype=torch.bfloat16, device=DEV)
    pad = torch.tensor(eo.GROUPED_PAD_OFFSETS, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(K, dtype=torch.bfloat16, device=DEV)
    ops.moe_gateup(act, case["x"].to(DEV), case["q"].to(DEV), case["sorted_ids"].to(DEV), pad,
                   zeros, scale=case["scale"].to(DEV))
    _report("fp8 moe_gateup", case, act, eo.c_kernel(K))
    assert (act[case["sorted_ids"].to(DEV) < 0] == 0).all(), "pad rows are not zero"


# --- quantised module ---------------------------------------------------------------

class TestQuantisedMoE:
    """``TestMoEGroupedGEMM`` of test_gpu_kernels.py on the quantised module:
    the same input distributions and thresholds."""

    def _moe(self, E=8, I=512, H=512, k=2, seed=0):
        from kllms_amd.engine.config import ModelArchConfig
        from kllms_amd.models.mixtral import MixtralMoE
        from kllms_amd.parallel.tp import ParallelContext

        cfg = ModelArchConfig(arch="mixtral", vocab_size=512, hidden_size=H,
                              intermediate_size=I, num_layers=1, num_heads=4,
                              num_kv_heads=2, num_experts=E, num_experts_per_tok=k)
        torch.manual_seed(seed)
        moe = MixtralMoE(cfg, ParallelContext(), torch.bfloat16).to(DEV)
        with torch.no_grad():
            moe.gate.weight.normal_(0, 0.5)
            moe.w_gate_up.normal_(0, 0.05)
            moe.w_down.normal_(0, 0.05)
        moe.quantize_fp8_()
        assert moe.w_gate_up is None and moe.w_down_q.dtype == torch.float8_e4m3fn
        return moe

    def _compare(self, got, want, what):
        assert torch.isfinite(got.float()).all()
        diff = (got.float() - want.float()).abs()
        scale = want.float().abs().mean().clamp_min(1e-3)
        print(f"{what}: mean rel {(diff.mean() / scale).item():.4f}, max abs {diff.max().item():.4f}")
        assert (diff.mean() / scale).item() < 0.05, (diff.max().item(), scale.item())
        assert diff.max().item() < 0.25

    @pytest.mark.parametrize("T", [129, 300])
    def test_grouped_hip_matches_torch_loop(self, T):
        moe = self._moe()
        torch.manual_seed(T)
        x = (torch.randn(T, 512) * 0.5).bfloat16().to(DEV)
        probs = torch.softmax(moe.gate(x).float(), -1)
        topw, topi = torch.topk(probs, moe.k, -1)
        topw = topw / topw.sum(-1, keepdim=True)
        got = moe._forward_grouped_hip(x, topw, topi)
        want = moe._forward_grouped(x, topw, topi)
        self._compare(got, want, f"quantised grouped T={T}")

    def test_empty_and_skewed_experts(self):
        moe = self._moe(E=4)
        T = 257
        torch.manual_seed(3)
        x = (torch.randn(T, 512) * 0.5).bfloat16().to(DEV)
        topi = torch.zeros(T, 2, dtype=torch.long, device=DEV)
        topi[:, 1] = 1
        topi[::17, 0] = 3        # expert 2 gets nothing
        topw = torch.full((T, 2), 0.5, device=DEV)
        got = moe._forward_grouped_hip(x, topw, topi)
        want = moe._forward_grouped(x, topw, topi)
        self._compare(got, want, "quantised grouped, empty and skewed experts")

    def test_dense_matches_torch_loop(self):
        moe = self._moe()
        T = 64
        torch.manual_seed(T)
        x = (torch.randn(T, 512) * 0.5).bfloat16().to(DEV)
        probs = torch.softmax(moe.gate(x).float(), -1)
        topw, topi = torch.topk(probs, moe.k, -1)
        topw = topw / topw.sum(-1, keepdim=True)
        self._compare(moe._forward_dense(x, topw, topi), moe._forward_grouped(x, topw, topi),
                      "quantised dense T=64")


# --- engine -----------------------------------------------------------------------

def _engine(graphs, **kw):
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    return LLMEngine(EngineConfig(model="mid-mixtral", max_kv_blocks=512, use_hip_graphs=graphs,
                                  seed=3, expert_weight_dtype="fp8_e4m3", **kw))


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


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("KLLMS_EXPERT_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KLLMS_WEIGHT_DTYPE", raising=False)


def _decode_check(eng, what):
    from kllms_amd.models.llama import ForwardBatch

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
    with torch.inference_mode():
        ref = _forced_torch(lambda: eng.model.forward_decode(ids, batch))
        eager = eng.model.forward_decode(ids, batch)
        graph = eng._graph_runner.run(ids, batch)
        replay = eng._graph_runner.run(ids, batch).clone()
    assert eng._graph_runner._enabled, "hipGraph capture of the batched fp8 GEMM failed"
    _close(eager, ref, f"{what} eager decode logits")
    _close(graph, ref, f"{what} graph decode logits")
    assert torch.equal(graph, replay)
    for s in seqs:
        eng.kv.free_sequence(s)


class TestEngineFp8Experts:
    def test_prefill_logits_match_forced_torch(self):
        from kllms_amd.models.llama import ForwardBatch

        eng = _engine(graphs=False)
        mlp = eng.model.layers[0].mlp
        assert mlp.w_gate_up is None and mlp.w_down_q.dtype == torch.float8_e4m3fn
        assert eng.model.layers[0].self_attn.qkv_proj.weight is not None
        assert eng.model.lm_head.weight.dtype == torch.bfloat16
        T = 150                      # > 8 * E = 32: grouped path
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

        _close(run_prefill(), _forced_torch(run_prefill), f"mid-mixtral prefill logits T={T}")

    def test_decode_step_graph_and_eager_match_forced_torch(self):
        _decode_check(_engine(graphs=True), "mid-mixtral fp8 experts")

    def test_decode_step_with_attention_quantised_too(self):
        eng = _engine(graphs=True, weight_dtype="fp8_e4m3")
        assert eng.model.layers[0].self_attn.qkv_proj.weight is None
        assert eng.model.layers[0].mlp.w_gate_up is None
        _decode_check(eng, "mid-mixtral fp8 experts + fp8 attention")

    def test_generate_with_graphs(self):
        from kllms_amd.engine.engine import GenRequest
        from kllms_amd.engine.sampling import SamplingParams

        eng = _engine(graphs=True)
        out = eng.generate([
            GenRequest(prompt_ids=list(range(1, 80)), n=4,
                       sampling=SamplingParams(temperature=1.0, max_tokens=24, seed=5))
        ])[0]
        assert eng._graph_runner._enabled
        assert len(out.streams) == 4
        for s in out.streams:
            assert len(s.token_ids) > 0
            assert all(np.isfinite(lp) for lp in s.logprobs)

    def test_grouped_prefill_and_dense_decode_agree(self):
        """A 199-token prompt (grouped prefill), greedy n = 2: the two streams
        decode through the dense path and must be identical."""
        from kllms_amd.engine.engine import GenRequest
        from kllms_amd.engine.sampling import SamplingParams

        eng = _engine(graphs=False, default_max_new_tokens=4)
        out = eng.generate([GenRequest(prompt_ids=list(range(1, 200)), n=2,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=4))])[0]
        assert out.streams[0].token_ids == out.streams[1].token_ids
        assert len(out.streams[0].token_ids) == 4


def test_gpu_engine_needs_bf16():
    from kllms_amd.engine.config import EngineConfig
    from kllms_amd.engine.engine import LLMEngine

    with pytest.raises(ValueError, match="bfloat16"):
        LLMEngine(EngineConfig(model="mid-mixtral", max_kv_blocks=64, use_hip_graphs=False,
                               dtype="float16", expert_weight_dtype="fp8_e4m3"))
