"""HIP/CDNA4 kernel numerics tests vs the plain-PyTorch fp32 references.

Run on an MI355X box: python -m pytest tests -m gpu -x -q
Every test asserts the HIP kernel (kllms_amd._C) against ops/torch_ref.py on
identical random data (§5.4 rule 25: random, not zero-filled; rule 16:
asymmetric operands so transposes are caught).
"""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops
from kllms_amd.ops import torch_ref

DEV = "cuda:0"


def assert_close_bf16(actual, expected, rtol=2e-2, atol=2e-2, msg=""):
    a = actual.float()
    e = expected.float()
    diff = (a - e).abs()
    denom = e.abs().clamp_min(1.0)
    rel = (diff / denom).max().item()
    assert diff.max().item() < atol or rel < rtol, (
        f"{msg}: max abs {diff.max().item():.4e}, max rel {rel:.4e}"
    )


class TestMFMALayout:
    def test_selftest_asymmetric(self):
        from kllms_amd import _C

        torch.manual_seed(0)
        A = (torch.randn(32, 16) * 0.5).bfloat16().to(DEV)
        B = (torch.randn(16, 32) * 0.5).bfloat16().to(DEV)
        D = _C.mfma_selftest(A, B)
        ref = A.float() @ B.float()
        assert_close_bf16(D, ref.to(DEV), rtol=5e-2, atol=5e-2, msg="mfma fragment map")


class TestElementwise:
    def test_rmsnorm(self):
        torch.manual_seed(1)
        x = torch.randn(100, 4096, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(4096, dtype=torch.bfloat16, device=DEV)
        out = ops.rmsnorm(x, w, 1e-5)
        ref = torch_ref.rmsnorm(x, w, 1e-5)
        assert_close_bf16(out, ref, msg="rmsnorm")

    def test_fused_add_rmsnorm(self):
        torch.manual_seed(2)
        x = torch.randn(64, 4096, dtype=torch.bfloat16, device=DEV)
        r = torch.randn(64, 4096, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(4096, dtype=torch.bfloat16, device=DEV)
        r_hip = r.clone()
        out, res = ops.fused_add_rmsnorm(x, r_hip, w, 1e-5)
        ref_out, ref_res = torch_ref.fused_add_rmsnorm(x, r.clone(), w, 1e-5)
        assert_close_bf16(res, ref_res, msg="fused residual")
        assert_close_bf16(out, ref_out, msg="fused rmsnorm")

    def test_silu_mul(self):
        torch.manual_seed(3)
        g = torch.randn(1000, 1024, dtype=torch.bfloat16, device=DEV)
        u = torch.randn(1000, 1024, dtype=torch.bfloat16, device=DEV)
        assert_close_bf16(ops.silu_mul(g, u), torch_ref.silu_mul(g, u), msg="silu_mul")

    def test_rope(self):
        torch.manual_seed(4)
        T, H, KVH, D = 33, 4, 2, 128
        cs = torch_ref.build_cos_sin_cache(D, 512, 10000.0, DEV)
        pos = torch.randint(0, 512, (T,), device=DEV)
        q = torch.randn(T, H, D, dtype=torch.bfloat16, device=DEV)
        k = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV)
        q_ref, k_ref = q.clone(), k.clone()
        ops.rope_inplace(q, k, pos, cs)
        torch_ref.rope_inplace(q_ref, k_ref, pos, cs)
        assert_close_bf16(q, q_ref, msg="rope q")
        assert_close_bf16(k, k_ref, msg="rope k")

    def test_store_kv(self):
        torch.manual_seed(5)
        T, KVH, D, NB, BS = 50, 2, 128, 16, 16
        k = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV)
        v = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV)
        kc = torch.zeros(NB, KVH, BS, D, dtype=torch.bfloat16, device=DEV)
        vc = torch.zeros_like(kc)
        kc2, vc2 = kc.clone(), vc.clone()
        slots = torch.randperm(NB * BS, device=DEV)[:T]
        ops.store_kv(k, v, kc, vc, slots)
        torch_ref.store_kv(k, v, kc2, vc2, slots)
        assert torch.equal(kc, kc2)
        assert torch.equal(vc, vc2)


class TestAttention:
    @pytest.mark.parametrize("seqlens", [[128], [64, 200, 32], [1, 333]])
    def test_prefill_varlen(self, seqlens):
        torch.manual_seed(6)
        H, KVH, D = 4, 2, 128
        T = sum(seqlens)
        cu = torch.tensor([0] + list(np.cumsum(seqlens)), dtype=torch.int32, device=DEV)
        q = torch.randn(T, H, D, dtype=torch.bfloat16, device=DEV) * 0.5
        k = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV) * 0.5
        v = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV) * 0.5
        scale = D ** -0.5
        out = ops.attn_prefill_varlen(q, k, v, cu, scale)
        ref = torch_ref.attn_prefill_varlen(q, k, v, cu.cpu(), scale)
        assert_close_bf16(out, ref, rtol=3e-2, atol=3e-2, msg=f"prefill {seqlens}")

    @pytest.mark.parametrize("gqa", [1, 2, 4, 8])
    def test_decode_paged(self, gqa):
        torch.manual_seed(7)
        KVH = 2
        H = KVH * gqa
        D, BS, NB, B = 128, 16, 64, 5
        ctx = [7, 16, 33, 257, 401]
        kc = torch.randn(NB, KVH, BS, D, dtype=torch.bfloat16, device=DEV) * 0.5
        vc = torch.randn(NB, KVH, BS, D, dtype=torch.bfloat16, device=DEV) * 0.5
        max_blocks = max((c + BS - 1) // BS for c in ctx)
        # disjoint random block tables
        perm = torch.randperm(NB).tolist()
        bt = torch.zeros(B, max_blocks, dtype=torch.int32, device=DEV)
        it = iter(perm * 4)
        for b in range(B):
            for j in range((ctx[b] + BS - 1) // BS):
                bt[b, j] = next(it)
        lens = torch.tensor(ctx, dtype=torch.int32, device=DEV)
        q = torch.randn(B, H, D, dtype=torch.bfloat16, device=DEV) * 0.5
        scale = D ** -0.5
        out = ops.attn_decode_paged(q, kc, vc, bt, lens, scale)
        ref = torch_ref.attn_decode_paged(q, kc, vc, bt, lens, scale)
        assert_close_bf16(out, ref, rtol=3e-2, atol=3e-2, msg=f"decode gqa={gqa}")


class TestSampling:
    def _tensors(self, B, V, temp=1.0, top_p=1.0, top_k=0):
        torch.manual_seed(8)
        logits = torch.randn(B, V, device=DEV) * 3
        t = torch.full((B,), temp, device=DEV)
        tp = torch.full((B,), top_p, device=DEV)
        tk = torch.full((B,), top_k, dtype=torch.int32, device=DEV)
        seeds = torch.arange(B, dtype=torch.int64, device=DEV) + 11
        steps = torch.zeros(B, dtype=torch.int64, device=DEV)
        return logits, t, tp, tk, seeds, steps

    def test_greedy_matches_ref(self):
        logits, t, tp, tk, seeds, steps = self._tensors(8, 50000, temp=0.0)
        toks, lps = ops.sample(logits, t, tp, tk, seeds, steps)
        assert torch.equal(toks.cpu(), logits.argmax(-1).cpu())
        ref_lp = torch.log_softmax(logits.float(), -1)[torch.arange(8), toks]
        assert torch.allclose(lps.cpu(), ref_lp.cpu(), atol=1e-3)

    def test_deterministic(self):
        logits, t, tp, tk, seeds, steps = self._tensors(4, 50000)
        t1, _ = ops.sample(logits, t, tp, tk, seeds, steps)
        t2, _ = ops.sample(logits, t, tp, tk, seeds, steps)
        assert torch.equal(t1, t2)
        t3, _ = ops.sample(logits, t, tp, tk, seeds + 1, steps)
        assert not torch.equal(t1, t3)

    def test_mask_respected(self):
        B, V = 4, 1024
        logits, t, tp, tk, seeds, steps = self._tensors(B, V)
        W = (V + 31) // 32
        mask = torch.zeros(B, W, dtype=torch.int32, device=DEV)
        allowed = [5, 99, 700]
        for a in allowed:
            mask[:, a // 32] |= 1 << (a % 32)
        toks, _ = ops.sample(logits, t, tp, tk, seeds, steps, mask)
        assert all(int(x) in allowed for x in toks.cpu())

    def test_top_k_confines(self):
        # EXACT top-k (refined histogram cut): the drawn token must be a
        # member of the true top-k, no bin-boundary slack
        B, V = 16, 8192
        logits, t, tp, tk, seeds, steps = self._tensors(B, V, top_k=5)
        toks, _ = ops.sample(logits, t, tp, tk, seeds, steps)
        for b in range(B):
            topk = set(logits[b].topk(5).indices.cpu().tolist())
            assert int(toks[b]) in topk

    def test_top_k_exact_with_crowded_boundary(self):
        # many near-identical logits straddling the k-th value: the refinement
        # sweeps must separate them (the coarse 0.078-wide bin cannot)
        B, V, K = 8, 8192, 7
        g = torch.Generator(device="cpu").manual_seed(5)
        base = torch.randn(B, V, generator=g) * 0.01  # everything within ~1 bin
        logits = base.to(DEV)
        t = torch.full((B,), 0.9, device=DEV)
        tp = torch.ones(B, device=DEV)
        tk = torch.full((B,), K, dtype=torch.int32, device=DEV)
        seeds = torch.arange(B, dtype=torch.int64, device=DEV) + 3
        for s in range(6):
            steps = torch.full((B,), s, dtype=torch.int64, device=DEV)
            toks, _ = ops.sample(logits, t, tp, tk, seeds, steps)
            for b in range(B):
                topk = set(logits[b].topk(K).indices.cpu().tolist())
                assert int(toks[b]) in topk, (b, s, int(toks[b]))

    def test_top_p_exact_nucleus(self):
        # nucleus membership: drawn token must be inside the smallest
        # prefix (by descending prob) whose mass reaches top_p
        B, V, P = 8, 8192, 0.7
        g = torch.Generator(device="cpu").manual_seed(9)
        logits = (torch.randn(B, V, generator=g) * 2.0).to(DEV)
        t = torch.ones(B, device=DEV)
        tp = torch.full((B,), P, device=DEV)
        tk = torch.zeros(B, dtype=torch.int32, device=DEV)
        seeds = torch.arange(B, dtype=torch.int64, device=DEV) + 17
        probs = torch.softmax(logits.float(), dim=-1)
        sp, si = probs.sort(dim=-1, descending=True)
        cum = sp.cumsum(-1)
        for s in range(6):
            steps = torch.full((B,), s, dtype=torch.int64, device=DEV)
            toks, _ = ops.sample(logits, t, tp, tk, seeds, steps)
            for b in range(B):
                ncut = int((cum[b] < P).sum().item()) + 1  # smallest prefix >= P
                nucleus = set(si[b, :ncut].cpu().tolist())
                assert int(toks[b]) in nucleus, (b, s, int(toks[b]), ncut)

    def test_distribution_tracks_softmax(self):
        # one peaked row sampled across many steps: empirical freq of the top
        # token ~ its softmax prob
        V = 1000
        logits = torch.zeros(1, V, device=DEV)
        logits[0, 7] = 2.5
        t = torch.ones(1, device=DEV)
        tp = torch.ones(1, device=DEV)
        tk = torch.zeros(1, dtype=torch.int32, device=DEV)
        seeds = torch.tensor([3], device=DEV)
        hits = 0
        N = 400
        for s in range(N):
            steps = torch.tensor([s], device=DEV)
            tok, _ = ops.sample(logits, t, tp, tk, seeds, steps)
            hits += int(tok.item() == 7)
        p_true = torch.softmax(logits[0], -1)[7].item()
        assert abs(hits / N - p_true) < 0.05


class TestEngineGPU:
    def test_teacher_forced_logits_match_torch_ref(self):
        """Prefill logits: HIP kernels vs forced-torch path on the same GPU
        weights (the kernel-vs-oracle engine-level check)."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import LLMEngine
        from kllms_amd.models.llama import ForwardBatch

        eng = LLMEngine(EngineConfig(model="mid-llama", max_kv_blocks=256, use_hip_graphs=False, seed=3))
        ids = torch.randint(0, 2000, (150,), device=DEV)

        def run_prefill():
            seq = eng.kv.alloc_sequence(150)
            batch = ForwardBatch(
                mode="prefill",
                positions=torch.arange(150, device=DEV),
                slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
                kv_caches=eng.kv.layer_caches(),
                cu_seqlens=torch.tensor([0, 150], dtype=torch.int32, device=DEV),
            )
            logits = eng.model.forward_prefill(ids, batch)
            eng.kv.free_sequence(seq)
            return logits

        hip_logits = run_prefill()
        os.environ["KLLMS_AMD_FORCE_TORCH_OPS"] = "1"
        try:
            ref_logits = run_prefill()
        finally:
            del os.environ["KLLMS_AMD_FORCE_TORCH_OPS"]
        diff = (hip_logits - ref_logits).abs().max().item()
        scale = ref_logits.abs().max().item()
        assert diff < 0.05 * max(scale, 1.0), f"prefill logits diverge: {diff} vs scale {scale}"

    def test_generate_end_to_end(self):
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(model="mid-llama", max_kv_blocks=512, use_hip_graphs=False, seed=4))
        out = eng.generate([
            GenRequest(prompt_ids=list(range(1, 80)), n=4,
                       sampling=SamplingParams(temperature=1.0, max_tokens=24, seed=5))
        ])[0]
        assert len(out.streams) == 4
        for s in out.streams:
            assert len(s.token_ids) > 0
            assert all(np.isfinite(lp) for lp in s.logprobs)

    def test_long_context_decode(self):
        """Multi-chunk split-K decode at ctx > 1000 must stay numerically
        sound end to end (positions, block tables, chunk reduce)."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(model="mid-llama", max_kv_blocks=2048, use_hip_graphs=False,
                                     max_seq_len=2048, seed=11))
        prompt = list(range(1, 1500))
        out = eng.generate([GenRequest(prompt_ids=prompt, n=2,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=8))])[0]
        toks = out.streams[0].token_ids
        assert toks == out.streams[1].token_ids  # greedy streams agree
        assert all(np.isfinite(lp) for lp in out.streams[0].logprobs)

        # teacher-forced check: big prefill over prompt + decoded prefix
        import torch as _t
        from kllms_amd.models.llama import ForwardBatch

        full = prompt + toks[:-1]
        seq = eng.kv.alloc_sequence(len(full))
        batch = ForwardBatch(
            mode="prefill",
            positions=_t.arange(len(full), device=DEV),
            slot_mapping=_t.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
            kv_caches=eng.kv.layer_caches(),
            cu_seqlens=_t.tensor([0, len(full)], dtype=_t.int32, device=DEV),
        )
        logits = eng.model.forward_prefill(_t.tensor(full, device=DEV), batch)
        eng.kv.free_sequence(seq)
        assert int(logits[0].argmax()) == toks[-1], "decode diverged from prefill at long context"

    def test_chunked_prefill_matches_packed_gpu(self):
        """Chunked prefill (decode-path slices over the paged cache) must
        reproduce the packed varlen prefill's next-token logits on the HIP
        kernel path (per-row context lengths in attn_decode, store_kv)."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import LLMEngine
        from kllms_amd.models.llama import ForwardBatch

        eng = LLMEngine(EngineConfig(
            model="mid-llama", max_kv_blocks=512, use_hip_graphs=False,
            max_seq_len=1024, seed=3,
        ))
        ids = [(i * 17) % 200 + 1 for i in range(101)]  # not a chunk multiple

        seq_a = eng.kv.alloc_sequence(len(ids))
        batch = ForwardBatch(
            mode="prefill",
            positions=torch.arange(len(ids), device=DEV),
            slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq_a), device=DEV),
            kv_caches=eng.kv.layer_caches(),
            cu_seqlens=torch.tensor([0, len(ids)], dtype=torch.int32, device=DEV),
        )
        logits_a = eng.model.forward_prefill(torch.tensor(ids, device=DEV), batch)

        seq_b = eng.kv.alloc_sequence(len(ids))
        logits_b = None
        for a in range(0, len(ids), 32):
            e = min(a + 32, len(ids))
            r = eng.prefill_chunk(seq_b, ids, a, e, want_logits=(e == len(ids)))
            if r is not None:
                logits_b = r
        la, lb = logits_a[0].float(), logits_b[0].float()
        scale = la.abs().max().item()
        diff = (la - lb).abs().max().item()
        eng.kv.free_sequence(seq_a)
        eng.kv.free_sequence(seq_b)
        assert diff < 0.05 * max(scale, 1.0), f"chunked vs packed logits: {diff} (scale {scale})"

    def test_mixtral_generate_gpu(self):
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(model="mid-mixtral", max_kv_blocks=256, use_hip_graphs=False, seed=9))
        out = eng.generate([
            GenRequest(prompt_ids=list(range(1, 60)), n=3,
                       sampling=SamplingParams(temperature=1.0, max_tokens=16, seed=2))
        ])[0]
        assert len(out.streams) == 3
        for s in out.streams:
            assert len(s.token_ids) > 0
            assert all(np.isfinite(lp) for lp in s.logprobs)

    def test_hipgraph_decode_matches_eager(self):
        """Graph-replayed decode step vs eager forward on IDENTICAL inputs.
        (Token-exact comparison is wrong by design: rocBLAS may pick different
        GEMM algorithms under capture, so logits are compared to tolerance.)"""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams
        from kllms_amd.models.llama import ForwardBatch

        eng = LLMEngine(EngineConfig(
            model="mid-llama", max_kv_blocks=512, use_hip_graphs=True,
            hip_graph_batch_sizes=[1, 2, 4, 8], max_seq_len=1024, seed=6,
        ))
        # run a generation to exercise capture + replay end to end
        out = eng.generate([GenRequest(prompt_ids=list(range(1, 50)), n=3,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=16))])[0]
        assert eng._graph_runner is not None and eng._graph_runner._enabled, \
            "hipGraph capture fell back to eager"
        assert all(len(s.token_ids) > 0 for s in out.streams)

        # teacher-forced: one decode step, graph vs eager, same inputs
        seq = eng.kv.alloc_sequence(40)
        pre = ForwardBatch(
            mode="prefill",
            positions=torch.arange(40, device=DEV),
            slot_mapping=torch.tensor(eng.kv.prefill_slot_mapping(seq), device=DEV),
            kv_caches=eng.kv.layer_caches(),
            cu_seqlens=torch.tensor([0, 40], dtype=torch.int32, device=DEV),
        )
        eng.model.forward_prefill(torch.arange(1, 41, device=DEV), pre)
        slot = eng.kv.append_slot(seq)
        mk_batch = lambda: ForwardBatch(
            mode="decode",
            positions=torch.tensor([40], device=DEV),
            slot_mapping=torch.tensor([slot], device=DEV),
            kv_caches=eng.kv.layer_caches(),
            block_tables=torch.tensor([seq.blocks + [0] * (4 - len(seq.blocks))], dtype=torch.int32, device=DEV)[:, :len(seq.blocks)],
            context_lens=torch.tensor([41], dtype=torch.int32, device=DEV),
        )
        ids = torch.tensor([123], device=DEV)
        graph_logits = eng._graph_runner.run(ids, mk_batch()).clone()
        eager_logits = eng.model.forward_decode(ids, mk_batch())
        diff = (graph_logits - eager_logits).abs().max().item()
        scale = eager_logits.abs().max().item()
        eng.kv.free_sequence(seq)
        assert diff < 0.05 * max(scale, 1.0), f"graph vs eager logits: {diff} (scale {scale})"

    def test_failed_capture_repairs_rng_state(self):
        """A capture that fails mid-flight must fall back to eager AND leave
        the default Philox generator usable — a capture that dies between
        capture_begin and capture_end otherwise raises 'Offset increment
        outside graph capture encountered unexpectedly' on the next RNG op.

        The injected failure is a pure-Python exception raised while the
        stream is capturing (a device-level violation like synchronize()
        inside capture sticky-errors the whole HIP context on ROCm and would
        poison every later test in the process, so it is NOT used here)."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(
            model="mid-llama", max_kv_blocks=256, use_hip_graphs=True,
            hip_graph_batch_sizes=[1, 2, 4], max_seq_len=512, seed=11,
        ))
        orig = eng.model.forward_hidden

        def poisoned(ids, batch):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("injected capture failure")
            return orig(ids, batch)

        eng.model.forward_hidden = poisoned
        try:
            out = eng.generate([GenRequest(
                prompt_ids=list(range(1, 20)), n=2,
                sampling=SamplingParams(temperature=0.8, max_tokens=4, seed=3))])[0]
        finally:
            eng.model.forward_hidden = orig
        assert eng._graph_runner is not None and not eng._graph_runner._enabled, \
            "poisoned capture unexpectedly succeeded"
        assert all(len(s.token_ids) > 0 for s in out.streams)  # eager fallback served
        t = torch.randn(64, device=DEV)  # generator must serve RNG again
        assert torch.isfinite(t).all()

    def test_no_garbage_collection_while_capturing(self):
        """The cyclic collector is off while the decode step is captured (a
        dead engine's hipGraphs and GPU memory must not be released inside a
        capture; see DecodeGraphRunner._capture) and back on afterwards. The
        test only reads the collector's state from inside an ordinary capture."""
        import gc

        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        assert gc.isenabled()
        eng = LLMEngine(EngineConfig(
            model="mid-llama", max_kv_blocks=256, use_hip_graphs=True,
            hip_graph_batch_sizes=[1, 2, 4], max_seq_len=512, seed=12,
        ))
        orig = eng.model.forward_hidden
        seen = []

        def watched(ids, batch):
            if torch.cuda.is_current_stream_capturing():
                seen.append(gc.isenabled())
            return orig(ids, batch)

        eng.model.forward_hidden = watched
        try:
            eng.generate([GenRequest(
                prompt_ids=list(range(1, 20)), n=2,
                sampling=SamplingParams(temperature=0.0, max_tokens=4))])
        finally:
            eng.model.forward_hidden = orig
        assert seen and not any(seen), "the collector was enabled during capture"
        assert gc.isenabled(), "the collector was left disabled"
        assert eng._graph_runner._enabled


class TestFp8KVCacheGPU:
    def test_store_and_decode_fp8(self):
        torch.manual_seed(17)
        KVH, D, BS, NB, B = 2, 128, 16, 64, 5
        H = KVH * 4
        ctx = [7, 33, 257, 120, 300]
        kc = torch.zeros(NB, KVH, BS, D, dtype=torch.float8_e4m3fn, device=DEV)
        vc = torch.zeros_like(kc)
        # fill via the store kernel (quantization on device)
        T = NB * BS
        k = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV) * 0.3
        v = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=DEV) * 0.3
        # outlier row: would saturate e4m3's +-448 under a static scale; the
        # per-row scale must absorb it
        k[3, 1, 7] = 800.0
        slots = torch.arange(T, device=DEV)
        ks = torch.ones(NB, KVH, BS, device=DEV)
        vs = torch.ones_like(ks)
        ops.store_kv(k, v, kc, vc, slots, ks, vs)
        # quantized store matches the torch reference (dequantized compare:
        # HIP's and torch's fp8 RNE can differ on exact ties, so bitwise
        # equality is the wrong assertion)
        ref_kc = torch.zeros_like(kc)
        ref_vc = torch.zeros_like(vc)
        ref_ks = torch.ones_like(ks)
        ref_vs = torch.ones_like(vs)
        torch_ref.store_kv(k, v, ref_kc, ref_vc, slots, ref_ks, ref_vs)
        assert torch.allclose(ks, ref_ks, rtol=1e-6), "per-row K scales diverge"
        assert torch.allclose(vs, ref_vs, rtol=1e-6), "per-row V scales diverge"
        deq = kc.float() * ks.unsqueeze(-1)
        ref_deq = ref_kc.float() * ref_ks.unsqueeze(-1)
        # one RNE tie at the top of the code range costs ulp(448)*s
        thresh = (ks.max().item() * 32) + 1e-6
        diff = (deq - ref_deq).abs()
        assert diff.max().item() <= thresh, f"fp8 store quantization diverges: {diff.max().item()}"
        mismatch_frac = (kc.view(torch.uint8) != ref_kc.view(torch.uint8)).float().mean().item()
        assert mismatch_frac < 0.01, f"too many fp8 rounding mismatches: {mismatch_frac}"
        # the outlier survives per-row quantization with e4m3 relative precision
        got = deq[slots[3] // BS, 1, slots[3] % BS, 7]
        assert abs(got.item() - 800.0) <= 800.0 * 0.0625, f"outlier lost: {got.item()}"

        max_blocks = max((c + BS - 1) // BS for c in ctx)
        perm = torch.randperm(NB).tolist()
        bt = torch.zeros(B, max_blocks, dtype=torch.int32, device=DEV)
        it = iter(perm * 4)
        for b in range(B):
            for j in range((ctx[b] + BS - 1) // BS):
                bt[b, j] = next(it)
        lens = torch.tensor(ctx, dtype=torch.int32, device=DEV)
        q = torch.randn(B, H, D, dtype=torch.bfloat16, device=DEV) * 0.5
        scale = D ** -0.5
        out = ops.attn_decode_paged(q, kc, vc, bt, lens, scale, ks, vs)
        ref = torch_ref.attn_decode_paged(q, kc, vc, bt, lens, scale, ref_ks, ref_vs)
        assert_close_bf16(out, ref, rtol=4e-2, atol=4e-2, msg="fp8 decode")
        # and the whole fp8 path tracks a full-precision oracle: per-row
        # scales keep the quantization error at e4m3's relative precision
        # even with the injected outlier in the context
        kc_bf = torch.zeros(NB, KVH, BS, D, dtype=torch.bfloat16, device=DEV)
        vc_bf = torch.zeros_like(kc_bf)
        torch_ref.store_kv(k, v, kc_bf, vc_bf, slots)
        oracle = torch_ref.attn_decode_paged(q, kc_bf, vc_bf, bt, lens, scale)
        assert_close_bf16(out, oracle, rtol=8e-2, atol=8e-2, msg="fp8 vs bf16 oracle")

    def test_engine_fp8_cache_generates(self):
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        # hipGraph capture over fp8 caches exercised too (decode graph holds
        # fp8 cache pointers; replay must hit the fp8-templated kernels)
        eng = LLMEngine(EngineConfig(model="mid-llama", max_kv_blocks=512, use_hip_graphs=True,
                                     hip_graph_batch_sizes=[1, 2, 4], max_seq_len=512,
                                     seed=3, kv_cache_dtype="fp8_e4m3"))
        out = eng.generate([GenRequest(prompt_ids=list(range(1, 80)), n=2,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=12))])[0]
        assert eng._graph_runner is not None and eng._graph_runner._enabled
        assert out.streams[0].token_ids == out.streams[1].token_ids
        assert all(np.isfinite(lp) for lp in out.streams[0].logprobs)


class TestOneShotAllreduce:
    def test_allreduce_matches_fp32_sum(self):
        """One-shot all-reduce (single-GPU peer simulation): all N buffers end
        holding the fp32-accumulated sum of the inputs (round-2 groundwork
        for the xGMI one-shot path)."""
        from kllms_amd import ops as kops

        torch.manual_seed(5)
        for n_peers in (2, 4, 8):
            for numel in (8, 4096, 5 * 4096, 120 * 4096):
                bufs = [torch.randn(numel, dtype=torch.bfloat16, device=DEV) for _ in range(n_peers)]
                want = torch.stack([b.float() for b in bufs]).sum(0).to(torch.bfloat16)
                kops._hip_or_raise().one_shot_allreduce(bufs)
                for r, b in enumerate(bufs):
                    assert torch.equal(b, want), f"peers={n_peers} numel={numel} rank-buf {r}"

    def test_allreduce_rejects_mismatch(self):
        from kllms_amd import ops as kops

        a = torch.randn(64, dtype=torch.bfloat16, device=DEV)
        b = torch.randn(128, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError):
            kops._hip_or_raise().one_shot_allreduce([a, b])


class TestMoEGroupedGEMM:
    """Grouped MoE MFMA kernels (ops/hip/moe.hip) vs the per-expert torch
    loop on identical routing — VERDICT r1 item 5."""

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
        return moe

    @pytest.mark.parametrize("T", [129, 300, 1024])
    def test_grouped_hip_matches_torch_loop(self, T):
        moe = self._moe()
        torch.manual_seed(T)
        x = (torch.randn(T, 512) * 0.5).bfloat16().to(DEV)
        logits = moe.gate(x).float()
        probs = torch.softmax(logits, -1)
        topw, topi = torch.topk(probs, moe.k, -1)
        topw = topw / topw.sum(-1, keepdim=True)
        got = moe._forward_grouped_hip(x, topw, topi)
        want = moe._forward_grouped(x, topw, topi)
        diff = (got.float() - want.float()).abs()
        scale = want.float().abs().mean().clamp_min(1e-3)
        assert (diff.mean() / scale).item() < 0.05, (diff.max().item(), scale.item())
        assert diff.max().item() < 0.25

    def test_empty_and_skewed_experts(self):
        # routing forced so some experts get zero tokens and one gets most
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
        assert torch.isfinite(got.float()).all()
        diff = (got.float() - want.float()).abs()
        assert diff.max().item() < 0.25

    def test_mixtral_engine_grouped_prefill_matches_dense(self):
        """End-to-end: a long prompt (grouped path) and the same prompt split
        token-by-token through decode (dense path) give matching logits."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(model="mid-mixtral", max_kv_blocks=512,
                                     use_hip_graphs=False, device=DEV, seed=0,
                                     default_max_new_tokens=4))
        ids = list(range(1, 200))   # 199 tokens > 8*E=32 -> grouped prefill
        out = eng.generate([GenRequest(prompt_ids=ids, n=2,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=4))])[0]
        assert out.streams[0].token_ids == out.streams[1].token_ids
        assert len(out.streams[0].token_ids) == 4


class TestLevenshteinKernel:
    def test_matches_python_dp(self):
        import random
        import string as _string

        from kllms_amd.utils.text import levenshtein_distance

        rng = random.Random(11)
        alpha = _string.ascii_lowercase + _string.digits
        strs = [""] + ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 50)))
                       for _ in range(40)]
        N = len(strs)
        chars = torch.zeros(N, 64, dtype=torch.uint8)
        lens = torch.zeros(N, dtype=torch.int32)
        for i, s in enumerate(strs):
            b = s.encode()
            chars[i, :len(b)] = torch.tensor(list(b), dtype=torch.uint8)
            lens[i] = len(b)
        ii, jj = torch.triu_indices(N, N, offset=1)
        out = ops.levenshtein_pairs(chars.to(DEV), lens.to(DEV),
                                    ii.to(torch.int32).to(DEV), jj.to(torch.int32).to(DEV))
        out = out.cpu().tolist()
        for k in range(len(out)):
            want = levenshtein_distance(strs[int(ii[k])], strs[int(jj[k])])
            assert out[k] == want, (strs[int(ii[k])], strs[int(jj[k])], out[k], want)

    def test_accel_precompute_consistent_with_cpu_path(self):
        from kllms_amd.consensus import similarity as simmod
        from kllms_amd.consensus.accel import precompute_levenshtein_cache
        from kllms_amd.engine.api import LocalEngineClient

        client = LocalEngineClient(model="tiny-llama", max_kv_blocks=128,
                                   use_hip_graphs=False, device=DEV)
        _ = client.engine
        contents = [{"city": "Paris", "note": "short text A"},
                    {"city": "paris!", "note": "short text B"},
                    {"city": "Berlin", "note": "short text A"}]
        n = precompute_levenshtein_cache(contents, client=client)
        assert n > 0
        # cached values equal the CPU formula
        got = simmod.string_similarity("Paris", "paris!", "embeddings", None)
        want = simmod.levenshtein_similarity("Paris", "paris!")
        assert got == pytest.approx(want, abs=1e-9)


class TestPrefixCacheGPU:
    def test_shared_prefix_parity_on_gpu(self):
        """Prefix-cache hits must be output-invisible with the HIP kernels:
        the cached-head + decode-mode-tail path must reproduce the uncached
        packed-prefill greedy decode exactly."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        shared = list(range(2, 300))   # 298 tokens >= prefix_cache_min_tokens=128
        mk = lambda cache: LLMEngine(EngineConfig(
            model="mid-llama", max_kv_blocks=1024, use_hip_graphs=True,
            device=DEV, seed=0, default_max_new_tokens=12,
            enable_prefix_caching=cache))
        greedy = SamplingParams(temperature=0.0, max_tokens=12)

        eng_c = mk(True)
        eng_c.generate([GenRequest(prompt_ids=shared + [333], n=1, sampling=greedy)])
        out_hit = eng_c.generate([GenRequest(prompt_ids=shared + [444, 445], n=2, sampling=greedy)])[0]
        assert eng_c.prefix_cache.hits >= 1
        assert eng_c.prefix_cache.tokens_saved >= 128

        eng_u = mk(False)
        eng_u.generate([GenRequest(prompt_ids=shared + [333], n=1, sampling=greedy)])
        out_ref = eng_u.generate([GenRequest(prompt_ids=shared + [444, 445], n=2, sampling=greedy)])[0]

        for a, b in zip(out_hit.streams, out_ref.streams):
            assert a.token_ids == b.token_ids


class TestRealVocabGPU:
    def test_hf_vocab_engine_constrained_on_gpu(self, tmp_path):
        """Engine over an HF-layout model dir (trained ByteLevel-BPE
        tokenizer.json, synthetic safetensors) on the HIP path: greedy
        determinism + constrained parse producing schema-valid JSON with the
        REAL vocab's token masks in the sampling kernel."""
        import json as _json
        import shutil

        from pydantic import BaseModel, Field

        from kllms_amd.engine.api import LocalEngineClient
        from kllms_amd.engine.config import MODEL_PRESETS
        from tests.test_weights_io import _make_hf_llama_checkpoint

        arch = MODEL_PRESETS["mid-llama"].model_copy(update={"vocab_size": 571})
        d = tmp_path / "hfmodel"
        d.mkdir()
        with open(d / "config.json", "w") as f:
            _json.dump({
                "model_type": "llama", "vocab_size": 571, "hidden_size": arch.hidden_size,
                "intermediate_size": arch.intermediate_size, "num_hidden_layers": arch.num_layers,
                "num_attention_heads": arch.num_heads, "num_key_value_heads": arch.num_kv_heads,
                "rope_theta": arch.rope_theta, "rms_norm_eps": arch.rms_norm_eps,
                "max_position_embeddings": 2048, "tie_word_embeddings": False,
            }, f)
        shutil.copy(os.path.join(os.path.dirname(__file__), "data", "bpe_tokenizer.json"),
                    d / "tokenizer.json")
        _make_hf_llama_checkpoint(d, arch)

        class Rec(BaseModel):
            city: str = Field(max_length=10)
            n: int = Field(ge=0, le=99)

        client = LocalEngineClient(model=str(d), max_kv_blocks=512,
                                   use_hip_graphs=True, device=DEV,
                                   default_max_new_tokens=16, max_seq_len=1024)
        r1 = client.chat_completions_create(
            False, messages=[{"role": "user", "content": "name a city"}],
            n=3, temperature=0.0, max_tokens=10)
        assert r1.choices[0].message.content == r1.choices[1].message.content

        r2 = client.chat_completions_parse(
            False, messages=[{"role": "user", "content": "emit a record"}],
            response_format=Rec, n=4, temperature=0.9, max_tokens=64, seed=1)
        for ch in r2.choices:
            if ch.finish_reason == "stop":
                assert ch.message.parsed is not None
                obj = _json.loads(ch.message.content)
                assert set(obj) == {"city", "n"} and 0 <= obj["n"] <= 99


class TestQwenGPU:
    def test_qwen_bias_engine_generates(self):
        """Qwen2-style fused-QKV bias through the full GPU path (rocBLAS
        GEMM + bias epilogue, HIP attention, hipGraph decode capture)."""
        from kllms_amd.engine.config import EngineConfig
        from kllms_amd.engine.engine import GenRequest, LLMEngine
        from kllms_amd.engine.sampling import SamplingParams

        eng = LLMEngine(EngineConfig(model="mid-qwen", max_kv_blocks=512, use_hip_graphs=True,
                                     hip_graph_batch_sizes=[1, 2, 4], max_seq_len=512, seed=5))
        assert eng.model.layers[0].self_attn.qkv_proj.bias is not None
        assert torch.equal(eng.model.lm_head.weight, eng.model.embed_tokens.weight)
        out = eng.generate([GenRequest(prompt_ids=list(range(1, 60)), n=2,
                                       sampling=SamplingParams(temperature=0.0, max_tokens=10))])[0]
        assert eng._graph_runner is not None and eng._graph_runner._enabled
        assert out.streams[0].token_ids == out.streams[1].token_ids
        # the bias is live: zeroing it changes the greedy continuation path
        with torch.no_grad():
            for layer in eng.model.layers:
                layer.self_attn.qkv_proj.bias.zero_()
        out2 = eng.generate([GenRequest(prompt_ids=list(range(1, 60)), n=1,
                                        sampling=SamplingParams(temperature=0.0, max_tokens=10))])[0]
        assert out2.streams[0].token_ids != out.streams[0].token_ids
