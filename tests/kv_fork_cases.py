"""Shared cases for the fork_batch tests (CPU and GPU): a small PagedKVCache
pre-filled with distinct junk per block, parents with tail lengths 0, 1 and 15
forked 1, 2 and 5 ways, and byte-level comparison helpers."""

import torch

from kllms_amd.engine.kvcache import PagedKVCache, SequenceKV

L, NB, KVH, BS, D = 3, 64, 2, 16, 8
# (prompt tokens, children): tails 0, 1 and 15 with counts 1, 2 and 5
PARENTS = [(32, 2), (17, 5), (31, 1), (15, 5), (33, 2)]


def make_cache(fp8, device="cpu", num_blocks=NB, layers=L, kvh=KVH, bs=BS, d=D):
    """Cache whose every block (and every fp8 scale row) holds values no other
    block holds, so a copy from the wrong block or layer shows."""
    dtype = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kv = PagedKVCache(layers, kvh, d, bs, num_blocks, device, dtype=dtype)
    g = torch.Generator().manual_seed(77 + int(fp8))
    for arr in (kv.k_all, kv.v_all):
        raw = torch.randint(0, 120 if fp8 else 0x7F00, arr.shape, generator=g,
                            dtype=torch.int16 if not fp8 else torch.uint8)
        arr.copy_(raw.view(dtype).to(device))
    if fp8:
        for arr in (kv.k_scale_all, kv.v_scale_all):
            arr.copy_((torch.rand(arr.shape, generator=g) + 0.5).to(device))
    return kv


def arrays(kv):
    out = [kv.k_all, kv.v_all]
    if kv.fp8:
        out += [kv.k_scale_all, kv.v_scale_all]
    return out


def as_int(t):
    """Integer view of a cache array for byte-exact comparison."""
    t = t.detach().cpu()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8)
    return t.view(torch.int32)


def snapshot(kv):
    return [as_int(a).clone() for a in arrays(kv)]


def alloc_parents(kv, parents=PARENTS):
    return [kv.alloc_sequence(n) for n, _ in parents]


def expected_after(before, pairs):
    """The cache arrays after copying block src -> dst in every layer."""
    want = [a.clone() for a in before]
    for s, d in pairs:
        for a, b in zip(want, before):
            a[:, d] = b[:, s]
    return want


def clone_seq(seq):
    return SequenceKV(blocks=list(seq.blocks), num_tokens=seq.num_tokens)
