"""Shared fixtures for the shared-prefix (cascade) decode-attention tests:
one paged-KV batch of forked groups, used by the CPU metadata test and the
GPU kernel tests alike (not a test module itself)."""

import random

import torch

KVH, D, BS = 2, 128, 16
NB = 384
JUNK_BLOCKS = 40          # reserved at the top of the pool, never in a table


def group_specs(gqa):
    """(fork_id, shared_blocks, context lengths). A: 528 shared keys (S=2 plus
    a 16-key remainder); B: exactly 256 shared keys; C: 160 shared keys (not
    cascaded); a singleton; at gqa=8 a 9-member group (72 rows, two tiles)."""
    specs = [
        (0, 33, [529, 530, 600, 777, 1025]),
        (1, 16, [257, 300]),
        (2, 10, [170, 200, 290]),
        (3, 0, [401]),
    ]
    if gqa == 8:
        specs.append((4, 17, [273 + 11 * i for i in range(9)]))
    return specs


def build_batch(gqa, seed=0):
    """CPU tensors: q [B, H, D] bf16, bf16 caches [NB, KVH, BS, D], int32
    block tables and context lengths, plus the python block lists / fork ids
    the metadata builder takes. Rows of different groups are interleaved."""
    g = torch.Generator().manual_seed(100 + seed)
    rnd = random.Random(7 + seed)
    H = KVH * gqa
    free = list(range(NB - JUNK_BLOCKS))
    rnd.shuffle(free)
    rows = []  # (fork_id, ctx, blocks)
    for fid, shared_blocks, ctxs in group_specs(gqa):
        shared = [free.pop() for _ in range(shared_blocks)]
        for ctx in ctxs:
            n = (ctx + BS - 1) // BS
            rows.append((fid, ctx, shared + [free.pop() for _ in range(n - shared_blocks)]))
    rnd.shuffle(rows)  # members of a group end up at non-adjacent rows
    B = len(rows)
    max_blocks = max(len(r[2]) for r in rows)
    bt = torch.zeros(B, max_blocks, dtype=torch.int32)
    for i, (_, _, blocks) in enumerate(rows):
        bt[i, : len(blocks)] = torch.tensor(blocks, dtype=torch.int32)
    return {
        "gqa": gqa,
        "q": (torch.randn(B, H, D, generator=g) * 0.5).bfloat16(),
        "kc": (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16(),
        "vc": (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16(),
        "bt": bt,
        "lens": torch.tensor([r[1] for r in rows], dtype=torch.int32),
        "block_lists": [r[2] for r in rows],
        "fork_ids": [r[0] for r in rows],
        "scale": D ** -0.5,
    }


def build_tiles(batch):
    from kllms_amd.engine.shared_prefix import build_shared_prefix_tiles

    return build_shared_prefix_tiles(batch["block_lists"], batch["fork_ids"], BS, batch["gqa"])


def assert_close_bf16(actual, expected, rtol=3e-2, atol=3e-2, msg=""):
    """The project's kernel-level criterion (tests/test_gpu_kernels.py)."""
    a = actual.float()
    e = expected.float()
    diff = (a - e).abs()
    denom = e.abs().clamp_min(1.0)
    rel = (diff / denom).max().item()
    assert diff.max().item() < atol or rel < rtol, (
        f"{msg}: max abs {diff.max().item():.4e}, max rel {rel:.4e}"
    )


def assert_logits_close(actual, ref, msg=""):
    """Engine-level criterion: max|dlogits| < 0.05 * max(|ref|, 1)."""
    a, r = actual.float(), ref.float()
    d = (a - r).abs().max().item()
    bound = 0.05 * max(r.abs().max().item(), 1.0)
    assert d < bound, f"{msg}: max |dlogits| {d:.4e} >= {bound:.4e}"


def decode_step_batches(eng, state):
    """The decode step's ForwardBatch for ``state`` twice — with the state's
    cascade metadata and without — over identical inputs (the prompt lengths
    used leave room in every stream's last block, so no block is allocated)."""
    from kllms_amd.models.llama import ForwardBatch

    bs = eng.kv.block_size
    assert all(s.seq.num_tokens % bs != 0 for s in state.streams)
    slots = (
        state.bt.gather(1, (state.positions // bs).unsqueeze(1).to(torch.int64)).squeeze(1)
        .to(torch.int64) * bs + state.positions % bs
    )

    def mk(shared):
        return ForwardBatch(
            mode="decode", positions=state.positions, slot_mapping=slots,
            kv_caches=eng.kv.layer_caches(), block_tables=state.bt,
            context_lens=state.ctx, shared=shared)

    return mk(state.shared), mk(None)
