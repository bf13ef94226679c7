"""Shared-prefix cascade metadata: the pure-Python tile builder and the torch
reference that consumes it (CPU)."""

import pytest
import torch

from kllms_amd.engine.shared_prefix import build_shared_prefix_tiles
from kllms_amd.ops import torch_ref

import shared_prefix_cases as cases

BS = 16


def lists(shared, privates, base=1000):
    """Block lists with a common head of ``shared`` blocks and per-member
    private tails (disjoint ids)."""
    head = list(range(shared))
    out, nxt = [], base
    for p in privates:
        out.append(head + list(range(nxt, nxt + p)))
        nxt += p
    return out


def test_five_siblings_33_blocks():
    t = build_shared_prefix_tiles(lists(33, [1, 1, 5, 16, 32]), [7] * 5, BS, gqa=4)
    assert t.skip == [2] * 5
    assert t.n_tiles == 1 and t.tile_nmembers == [5] and t.tile_chunks == [2]
    assert t.tile_rows[0][:5] == [0, 1, 2, 3, 4] and len(t.tile_rows[0]) == 64
    assert all(r == -1 for r in t.tile_rows[0][5:])
    assert t.rows_cascaded == 5


def test_single_member_group_not_cascaded():
    t = build_shared_prefix_tiles(lists(33, [1]) + lists(40, [2], base=5000), [0, 1], BS, gqa=4)
    assert t.skip == [0, 0] and t.n_tiles == 0 and t.rows_cascaded == 0


def test_160_shared_keys_not_cascaded():
    t = build_shared_prefix_tiles(lists(10, [1, 3, 9]), [0] * 3, BS, gqa=4)
    assert t.skip == [0, 0, 0] and t.n_tiles == 0


def test_exactly_256_shared_keys():
    t = build_shared_prefix_tiles(lists(16, [1, 3]), [0, 0], BS, gqa=4)
    assert t.skip == [1, 1] and t.tile_chunks == [1] and t.tile_nmembers == [2]


def test_min_shared_chunks_threshold():
    t = build_shared_prefix_tiles(lists(33, [1, 1]), [0, 0], BS, gqa=4, min_shared_chunks=3)
    assert t.skip == [0, 0] and t.n_tiles == 0


def test_non_adjacent_members():
    a = lists(33, [1, 2, 3])
    b = lists(16, [1, 1], base=7000)
    b = [[x + 3000 for x in l] for l in b]
    block_lists = [a[0], b[0], a[1], [9000 + i for i in range(20)], b[1], a[2]]
    t = build_shared_prefix_tiles(block_lists, [5, 9, 5, None, 9, 5], BS, gqa=2)
    assert t.skip == [2, 1, 2, 0, 1, 2]
    assert t.n_tiles == 2
    assert t.tile_rows[0][:3] == [0, 2, 5] and t.tile_nmembers[0] == 3 and t.tile_chunks[0] == 2
    assert t.tile_rows[1][:2] == [1, 4] and t.tile_nmembers[1] == 2 and t.tile_chunks[1] == 1


def test_nine_members_gqa8_two_tiles():
    t = build_shared_prefix_tiles(lists(17, [2] * 9), [3] * 9, BS, gqa=8)
    assert t.n_tiles == 2
    assert t.tile_nmembers == [8, 1] and t.tile_chunks == [1, 1]
    assert t.tile_rows[0][:8] == list(range(8)) and t.tile_rows[1][0] == 8
    assert t.skip == [1] * 9


def test_lists_diverging_before_the_prompt_end():
    """The shared length follows the block lists: a member whose list departs
    at block 20 bounds the group to 20 shared blocks (320 keys, S=1), however
    long the common prompt was."""
    ls = lists(33, [1, 1, 1])
    ls[1] = ls[1][:20] + [8000 + i for i in range(14)]
    t = build_shared_prefix_tiles(ls, [0, 0, 0], BS, gqa=4)
    assert t.tile_chunks == [1] and t.skip == [1, 1, 1]


def test_context_lens_bound_the_shared_chunks():
    t = build_shared_prefix_tiles(lists(33, [1, 1]), [0, 0], BS, gqa=4, context_lens=[300, 600])
    assert t.skip == [1, 1]


def test_bad_arguments():
    with pytest.raises(ValueError):
        build_shared_prefix_tiles([[1]], [0, 1], BS, gqa=4)
    with pytest.raises(ValueError):
        build_shared_prefix_tiles([[1]], [0], BS, gqa=128)


@pytest.mark.parametrize("gqa", [1, 2, 4, 8])
def test_reference_with_metadata_matches_plain_reference(gqa):
    b = cases.build_batch(gqa)
    tiles = cases.build_tiles(b)
    by_fork = {}
    for row, fid in enumerate(b["fork_ids"]):
        by_fork.setdefault(fid, []).append(row)
    want = {0: 2, 1: 1, 2: 0, 3: 0, 4: 1}
    for fid, rows in by_fork.items():
        assert [tiles.skip[r] for r in rows] == [want[fid]] * len(rows)
    assert tiles.n_tiles == (4 if gqa == 8 else 2)
    shared = tiles.to_tensors("cpu")
    ref = torch_ref.attn_decode_paged(b["q"], b["kc"], b["vc"], b["bt"], b["lens"], b["scale"])
    out = torch_ref.attn_decode_paged_shared(
        b["q"], b["kc"], b["vc"], b["bt"], b["lens"], b["scale"], shared=shared)
    cases.assert_close_bf16(out, ref, msg=f"cascade reference gqa={gqa}")


def test_reference_really_reads_the_metadata():
    """Wrong metadata must give wrong numbers: skipping a chunk that no tile
    supplies drops those keys from the softmax."""
    b = cases.build_batch(4)
    tiles = cases.build_tiles(b)
    row = b["fork_ids"].index(3)          # the singleton, 401 keys
    tiles.skip[row] = 1
    shared = tiles.to_tensors("cpu")
    ref = torch_ref.attn_decode_paged(b["q"], b["kc"], b["vc"], b["bt"], b["lens"], b["scale"])
    out = torch_ref.attn_decode_paged_shared(
        b["q"], b["kc"], b["vc"], b["bt"], b["lens"], b["scale"], shared=shared)
    assert (out[row].float() - ref[row].float()).abs().max().item() > 1e-2
