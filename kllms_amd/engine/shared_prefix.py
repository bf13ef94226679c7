"""Host metadata for shared-prefix (cascade) decode attention.

The streams forked from one prompt share that prompt's KV blocks. The
cascade kernel (ops/hip/attn_decode_shared.hip) reads a group's shared K/V
once and multiplies it against all of the group's query rows; the per-stream
kernel then only covers each stream's private suffix. This module turns the
decode batch's block lists into the four small tables the kernel takes.

Pure Python over lists — no torch, no device — so it is testable anywhere
and, being a deterministic function of the streams, comes out identical on
every tensor-parallel rank.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

TILE_SLOTS = 64  # width of a tile_rows row (kernel contract)


@dataclass
class SharedPrefixTiles:
    """skip[b]: leading 256-key chunks of row b that the cascade kernel owns
    (0 = row not cascaded). One tile = up to ``max_rows // gqa`` rows of one
    group: tile_rows[t] holds their batch rows (-1 padded to 64),
    tile_nmembers[t] how many, tile_chunks[t] the group's shared chunks."""

    skip: List[int]
    tile_rows: List[List[int]] = field(default_factory=list)
    tile_nmembers: List[int] = field(default_factory=list)
    tile_chunks: List[int] = field(default_factory=list)

    @property
    def n_tiles(self) -> int:
        return len(self.tile_nmembers)

    @property
    def rows_cascaded(self) -> int:
        return sum(1 for s in self.skip if s > 0)

    def to_tensors(self, device):
        """The ops-level view (ops.SharedPrefix, int32 tensors on ``device``)."""
        import torch

        from ..ops import SharedPrefix

        def t(x, shape):
            return torch.tensor(x, dtype=torch.int32).reshape(shape).to(device)

        n = self.n_tiles
        return SharedPrefix(
            skip_chunks=t(self.skip, (len(self.skip),)),
            tile_rows=t(self.tile_rows, (n, TILE_SLOTS)),
            tile_nmembers=t(self.tile_nmembers, (n,)),
            tile_chunks=t(self.tile_chunks, (n,)),
        )


def _common_prefix_len(lists: Sequence[Sequence[int]]) -> int:
    n = min(len(l) for l in lists)
    first = lists[0]
    for i in range(n):
        b = first[i]
        for l in lists[1:]:
            if l[i] != b:
                return i
    return n


def build_shared_prefix_tiles(
    block_lists: Sequence[Sequence[int]],
    fork_ids: Sequence[Optional[int]],
    block_size: int,
    gqa: int,
    chunk_keys: int = 256,
    min_shared_chunks: int = 1,
    max_rows: int = 64,
    context_lens: Optional[Sequence[int]] = None,
) -> SharedPrefixTiles:
    """Group rows by ``fork_id`` and tile every group worth cascading.

    - A group is the set of rows with equal ``fork_id`` (``None`` or a
      negative id: a row on its own). Members need not be adjacent rows.
    - Its shared blocks are the longest common prefix of the members' block
      LISTS — read from the lists, never assumed from a prompt length.
    - ``S = shared_blocks * block_size // chunk_keys`` whole chunks; with
      ``context_lens`` given, never more than the shortest member holds.
    - Fewer than 2 members or ``S < min_shared_chunks``: not cascaded
      (skip 0, no tile).
    - Groups of more than ``max_rows // gqa`` members are split into tiles.
    """
    B = len(block_lists)
    if len(fork_ids) != B:
        raise ValueError(f"{len(fork_ids)} fork ids for {B} rows")
    if gqa <= 0 or max_rows // gqa <= 0 or max_rows > TILE_SLOTS:
        raise ValueError(f"gqa={gqa} does not fit a {max_rows}-row tile")
    per_tile = max_rows // gqa
    groups: dict = {}
    for row, fid in enumerate(fork_ids):
        if fid is None or fid < 0:
            continue
        groups.setdefault(fid, []).append(row)

    out = SharedPrefixTiles(skip=[0] * B)
    for rows in groups.values():  # insertion order = first appearance
        if len(rows) < 2:
            continue
        shared_blocks = _common_prefix_len([block_lists[r] for r in rows])
        S = shared_blocks * block_size // chunk_keys
        if context_lens is not None:
            S = min(S, min(int(context_lens[r]) for r in rows) // chunk_keys)
        if S < max(1, min_shared_chunks):
            continue
        for r in rows:
            out.skip[r] = S
        for i in range(0, len(rows), per_tile):
            members = rows[i : i + per_tile]
            out.tile_rows.append(members + [-1] * (TILE_SLOTS - len(members)))
            out.tile_nmembers.append(len(members))
            out.tile_chunks.append(S)
    return out
