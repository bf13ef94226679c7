"""PagedKVCache.fork_batch on the CPU: the batched fork gives the block tables,
refcounts and cache bytes of the forks done one at a time with the per-layer
``copy_`` it replaces, touches nothing but its destination blocks, rolls back
on exhaustion and leaves copy-on-write in ``append_slot`` working."""

import pytest
import torch

import kv_fork_cases as fc


def legacy_fork(kv, parent):
    """The fork this change replaces: eager per-block ``copy_`` of the tail."""
    child = fc.SequenceKV(blocks=[], num_tokens=parent.num_tokens)
    tail = parent.num_tokens % kv.block_size
    for i, b in enumerate(parent.blocks):
        if i == len(parent.blocks) - 1 and tail != 0:
            dst = kv.allocator.alloc()
            for arr in fc.arrays(kv):
                arr[:, dst].copy_(arr[:, b])
            child.blocks.append(dst)
        else:
            kv.allocator.incref(b)
            child.blocks.append(b)
    return child


@pytest.fixture(params=[False, True], ids=["bf16", "fp8"])
def fp8(request):
    return request.param


def test_fork_batch_matches_one_by_one(fp8):
    kv, ref = fc.make_cache(fp8), fc.make_cache(fp8)
    start_free = kv.allocator.num_free
    parents, ref_parents = fc.alloc_parents(kv), fc.alloc_parents(ref)
    assert [p.blocks for p in parents] == [p.blocks for p in ref_parents]
    before = fc.snapshot(kv)

    got = kv.fork_batch([(p, n) for p, (_, n) in zip(parents, fc.PARENTS)])
    want = [[legacy_fork(ref, p) for _ in range(n)] for p, (_, n) in zip(ref_parents, fc.PARENTS)]

    assert [len(c) for c in got] == [n for _, n in fc.PARENTS]
    pairs = []
    for parent, kids, ref_kids in zip(parents, got, want):
        tail = parent.num_tokens % fc.BS
        for kid, ref_kid in zip(kids, ref_kids):
            assert kid.blocks == ref_kid.blocks and kid.num_tokens == parent.num_tokens
            n_shared = len(parent.blocks) - (1 if tail else 0)
            assert kid.blocks[:n_shared] == parent.blocks[:n_shared]
            if tail:
                assert kid.blocks[-1] not in parent.blocks
                assert kv.allocator.refcount(kid.blocks[-1]) == 1
                pairs.append((parent.blocks[-1], kid.blocks[-1]))
    assert len(pairs) == 5 + 1 + 5 + 2
    assert kv.allocator._refcount == ref.allocator._refcount
    assert kv.allocator.num_free == ref.allocator.num_free

    # private tails equal the parent's bytes (K, V, scales); every block that
    # is not a destination is unchanged; and the whole cache equals the
    # one-by-one reference
    after = fc.snapshot(kv)
    for a, w, r in zip(after, fc.expected_after(before, pairs), fc.snapshot(ref)):
        assert torch.equal(a, w)
        assert torch.equal(a, r)
    dsts = {d for _, d in pairs}
    keep = [b for b in range(fc.NB) if b not in dsts]
    for a, b in zip(after, before):
        assert torch.equal(a[:, keep], b[:, keep])

    for kids in got:
        for kid in kids:
            kv.free_sequence(kid)
    for p in parents:
        kv.free_sequence(p)
    assert kv.allocator.num_free == start_free
    assert not any(kv.allocator._refcount)


def test_fork_is_a_batch_of_one(fp8):
    kv = fc.make_cache(fp8)
    parent = kv.alloc_sequence(21)
    before = fc.snapshot(kv)
    kid = kv.fork(parent)
    assert kid.blocks[0] == parent.blocks[0] and kid.blocks[1] != parent.blocks[1]
    assert kv.allocator.refcount(parent.blocks[0]) == 2
    want = fc.expected_after(before, [(parent.blocks[1], kid.blocks[1])])
    for a, w in zip(fc.snapshot(kv), want):
        assert torch.equal(a, w)


def test_exhaustion_mid_batch_rolls_back(fp8):
    kv = fc.make_cache(fp8)
    parents = fc.alloc_parents(kv)
    # leave 6 free blocks: the batch needs 13 tail blocks and fails on the 7th
    hold = [kv.allocator.alloc() for _ in range(kv.allocator.num_free - 6)]
    free_before = kv.allocator.num_free
    refs_before = list(kv.allocator._refcount)
    before = fc.snapshot(kv)
    with pytest.raises(RuntimeError, match="out of blocks"):
        kv.fork_batch([(p, n) for p, (_, n) in zip(parents, fc.PARENTS)])
    assert kv.allocator.num_free == free_before == 6
    assert kv.allocator._refcount == refs_before
    for a, b in zip(fc.snapshot(kv), before):
        assert torch.equal(a, b)
    assert hold


def test_append_slot_detaches_shared_tail(fp8):
    kv = fc.make_cache(fp8)
    parent = kv.alloc_sequence(20)
    shared = fc.clone_seq(parent)          # a second owner of the same blocks
    for b in shared.blocks:
        kv.allocator.incref(b)
    before = fc.snapshot(kv)
    slot = kv.append_slot(shared)
    new = shared.blocks[1]
    assert new != parent.blocks[1] and shared.num_tokens == 21
    assert slot == new * fc.BS + 4
    assert kv.allocator.refcount(parent.blocks[1]) == 1 and kv.allocator.refcount(new) == 1
    want = fc.expected_after(before, [(parent.blocks[1], new)])
    for a, w in zip(fc.snapshot(kv), want):
        assert torch.equal(a, w)


def test_copy_rejects_source_that_is_a_destination():
    kv = fc.make_cache(False)
    with pytest.raises(AssertionError):
        kv._copy_blocks([1, 2], [2, 3])
    with pytest.raises(AssertionError):
        kv._copy_blocks([1, 2], [5, 5])
    with pytest.raises(AssertionError):
        kv._copy_blocks([1], [fc.NB])
