"""The batched KV block copy on the device (kv_copy.hip) against the cache
built on the CPU: 1, 7 and 600 pairs (the last wraps the kernel's capped
grid), one source feeding five destinations, bf16 and fp8 with scales, the
narrow-lane paths, fork_batch end to end, and one case in the production
regime where a layer of the block array spans more than 2^31 bytes.

Run on an MI355X box: python -m pytest tests/test_gpu_kv_fork_batch.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import kv_fork_cases as fc

DEV = "cuda:0"


def _pairs(n, num_blocks):
    """n (src, dst) pairs: the first five destinations share one source, the
    rest have sources of their own; sources and destinations are disjoint."""
    g = torch.Generator().manual_seed(900 + n)
    perm = torch.randperm(num_blocks, generator=g).tolist()
    dst = perm[:n]
    pool = perm[n:]
    src = [pool[0] if i < 5 else pool[i % len(pool)] for i in range(n)]
    return list(zip(src, dst))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("n", [1, 7, 600])
def test_copy_blocks_matches_cpu(n, fp8):
    nb = 64 if n <= 7 else 1024
    kv = fc.make_cache(fp8, DEV, num_blocks=nb)
    before = fc.snapshot(kv)
    pairs = _pairs(n, nb)
    if n >= 5:
        assert len({s for s, _ in pairs[:5]}) == 1
    # 600 pairs * 3 layers * 2 arrays = 3600 work units > the 2048-workgroup cap
    kv._copy_blocks([s for s, _ in pairs], [d for _, d in pairs])
    torch.cuda.synchronize()
    for a, w in zip(fc.snapshot(kv), fc.expected_after(before, pairs)):
        assert torch.equal(a, w)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_fork_batch_on_device(fp8):
    kv = fc.make_cache(fp8, DEV)
    parents = fc.alloc_parents(kv)
    before = fc.snapshot(kv)
    kids = kv.fork_batch([(p, n) for p, (_, n) in zip(parents, fc.PARENTS)])
    pairs = [(p.blocks[-1], k.blocks[-1]) for p, ks in zip(parents, kids) for k in ks
             if p.num_tokens % fc.BS]
    assert len(pairs) == 13
    for p in parents:                       # as the engine does, after the launch
        kv.free_sequence(p)
    torch.cuda.synchronize()
    for a, w in zip(fc.snapshot(kv), fc.expected_after(before, pairs)):
        assert torch.equal(a, w)


@pytest.mark.parametrize("kvh,bs,d,fp8", [(1, 1, 6, False), (1, 3, 1, True)],
                         ids=["12-byte-blocks", "3-byte-blocks"])
def test_narrow_geometry(kvh, bs, d, fp8):
    """Block sizes that are no multiple of 16 bytes take the 4-byte and the
    1-byte lanes (the fp8 scales here are 12 bytes per block)."""
    kv = fc.make_cache(fp8, DEV, num_blocks=40, kvh=kvh, bs=bs, d=d)
    before = fc.snapshot(kv)
    pairs = _pairs(7, 40)
    kv._copy_blocks([s for s, _ in pairs], [d_ for _, d_ in pairs])
    torch.cuda.synchronize()
    for a, w in zip(fc.snapshot(kv), fc.expected_after(before, pairs)):
        assert torch.equal(a, w)


def test_layer_stride_beyond_2_31_bytes():
    """Production regime: 32 KiB blocks, one layer spanning 2^31 + 2^20 bytes,
    so a 32-bit byte offset wraps. Only the blocks used are filled."""
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip("needs 16 GB of free device memory")
    kvh, bs, d, layers = 8, 16, 128, 2
    blk_bytes = kvh * bs * d * 2
    nb = 2 ** 31 // blk_bytes + 32
    edge = 2 ** 31 // blk_bytes           # first block past the 2^31-byte boundary
    k_all = torch.empty(layers, nb, kvh, bs, d, device=DEV, dtype=torch.bfloat16)
    v_all = torch.empty_like(k_all)
    assert k_all.stride(0) * 2 > 2 ** 31
    # (src, dst): block 0, the last block and both sides of the boundary take
    # part; 5 and 9 are neighbours that must stay as they are
    pairs = [(0, edge - 1), (edge + 1, 1), (edge - 2, nb - 1), (nb - 2, edge), (0, 7)]
    used = sorted({b for p in pairs for b in p} |
                  {2, 6, 8, edge - 3, edge + 2, nb - 3})
    g = torch.Generator().manual_seed(5)
    fill = {}
    for arr, nm in ((k_all, "k"), (v_all, "v")):
        for layer in range(layers):
            for b in used:
                x = torch.randint(0, 0x7F00, (kvh, bs, d), generator=g, dtype=torch.int16)
                fill[nm, layer, b] = x
                arr[layer, b].copy_(x.view(torch.bfloat16))
    src = torch.tensor([s for s, _ in pairs], dtype=torch.int32, device=DEV)
    dst = torch.tensor([d_ for _, d_ in pairs], dtype=torch.int32, device=DEV)
    ops.copy_kv_blocks(k_all, v_all, src, dst)
    torch.cuda.synchronize()
    moved = dict((d_, s) for s, d_ in pairs)
    for arr, nm in ((k_all, "k"), (v_all, "v")):
        for layer in range(layers):
            for b in used:
                want = fill[nm, layer, moved.get(b, b)]
                got = arr[layer, b].cpu().view(torch.int16)
                assert torch.equal(got, want), (nm, layer, b)
