"""hipGraph capture of the decode step.

The decode inner loop is launch-bound (dozens of small kernels x 32+ layers
per token); capturing it as a hipGraph (torch.cuda.CUDAGraph on ROCm IS
hipGraph) replays the whole step as one graph launch. Paged-KV pointer
indirection is handled the standard way: all graph inputs (token ids,
positions, slot mapping, block tables, context lens) live in fixed
pre-allocated buffers that the engine writes into before replay; the KV cache
tensors themselves are allocated once and never move.

Batch sizes are bucketed (config.hip_graph_batch_sizes); a decode batch of
size B runs the smallest captured bucket >= B with tail padding. Padded lanes
replay against a scratch KV block (slot 0 writes are masked by pointing
padded slots at a dedicated scratch block) and their outputs are discarded.

With shared-prefix attention on, every bucket also owns static cascade
metadata (skip_chunks[bs] and tile tables for bs // 2 tiles) and is captured
with the cascade launch in it. A step's metadata is copied in and the rest
zeroed; all-zero metadata replays as the plain per-stream path (the cascade
blocks return at once, no chunk is skipped).
"""

from __future__ import annotations

import gc
from typing import Dict, List, Optional

import torch

from ..models.llama import ForwardBatch


class DecodeGraphRunner:
    def __init__(self, engine, batch_sizes: List[int]):
        self.engine = engine
        self.batch_sizes = sorted(batch_sizes)
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.buffers: Dict[int, dict] = {}
        self.max_blocks_per_seq = (engine.config.max_seq_len + engine.config.kv_block_size - 1) // engine.config.kv_block_size
        # one scratch block for padded lanes' KV writes
        self._scratch_block = engine.kv.allocator.alloc()
        self._enabled = True

    def _capture(self, bs: int) -> None:
        eng = self.engine
        dev = eng.device
        mb = self.max_blocks_per_seq
        buf = {
            "ids": torch.zeros(bs, dtype=torch.long, device=dev),
            "positions": torch.zeros(bs, dtype=torch.long, device=dev),
            "slots": torch.full((bs,), self._scratch_block * eng.config.kv_block_size, dtype=torch.long, device=dev),
            "block_tables": torch.full((bs, mb), self._scratch_block, dtype=torch.int32, device=dev),
            "context_lens": torch.ones(bs, dtype=torch.int32, device=dev),
        }
        shared = None
        if eng.shared_prefix_attention:
            from ..ops import SharedPrefix

            nt = bs // 2   # a tile has >= 2 members except a large group's last
            shared = SharedPrefix(
                skip_chunks=torch.zeros(bs, dtype=torch.int32, device=dev),
                tile_rows=torch.full((nt, 64), -1, dtype=torch.int32, device=dev),
                tile_nmembers=torch.zeros(nt, dtype=torch.int32, device=dev),
                tile_chunks=torch.zeros(nt, dtype=torch.int32, device=dev),
            )
            buf["shared"] = shared
            buf["shared_src"] = None   # metadata object the buffers hold now
        batch = ForwardBatch(
            mode="decode",
            positions=buf["positions"],
            slot_mapping=buf["slots"],
            kv_caches=eng.kv.layer_caches(),
            block_tables=buf["block_tables"],
            context_lens=buf["context_lens"],
            shared=shared,
        )
        # warmup on a side stream (required before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                out = eng.model.forward_hidden(buf["ids"], batch)
        torch.cuda.current_stream().wait_stream(s)

        # Capture the LAYERS only; the LM-head GEMM runs eagerly per step —
        # under capture rocBLAS picks a stream-K algorithm (~3x slower, plus a
        # workspace fill) for the [B,H]x[H,V] shape; eager picks the
        # weight-streaming-bound one (measured in scripts/lmhead_probe.py).
        #
        # No cyclic garbage collection while the stream is capturing: an engine
        # and its graph runner refer to each other, so a dead engine's hipGraphs,
        # streams and GPU memory are released only by the collector, and
        # releasing them in the middle of a capture is not allowed (it has
        # aborted the process). torch.cuda.graph no longer collects before it
        # captures, so do it here, then hold the collector off until the end.
        g = torch.cuda.CUDAGraph()
        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                out = eng.model.forward_hidden(buf["ids"], batch)
        finally:
            if gc_was_enabled:
                gc.enable()
        buf["out"] = out
        self.graphs[bs] = g
        self.buffers[bs] = buf

    def _recover_generator_state(self) -> None:
        """Un-stick the default Philox generator after a failed capture.

        hipGraph capture registers the device's default RNG generator at
        capture_begin; only a successful capture_end runs the epilogue that
        clears the generator's 'capturing' flag. A capture that dies between
        the two (e.g. cudaStreamEndCapture on an invalidated capture) leaves
        the flag set, and the next RNG op ANYWHERE in the process then raises
        "Offset increment outside graph capture encountered unexpectedly".
        Swapping in a fresh clone of the state (same seed/offset, flag clear)
        repairs it.
        """
        try:
            idx = self.engine.device.index
            if idx is None:
                idx = torch.cuda.current_device()
            gen = torch.cuda.default_generators[idx]
            gen.graphsafe_set_state(gen.clone_state())
        except Exception:
            pass  # best effort: eager fallback works regardless for non-RNG ops

    def _bucket(self, b: int) -> Optional[int]:
        for bs in self.batch_sizes:
            if bs >= b:
                return bs
        return None

    @staticmethod
    def _load_shared(buf: dict, src, B: int) -> None:
        """Copy a step's cascade metadata into the bucket's static tables and
        zero the rest (padded lanes: skip 0; unused tiles: 0 members). The
        metadata only changes when the decode state is rebuilt, so an
        unchanged source object is not copied again."""
        if buf["shared_src"] is src and buf.get("shared_B") == B:
            return
        dst = buf["shared"]
        dst.skip_chunks.zero_()
        dst.tile_nmembers.zero_()
        dst.tile_chunks.zero_()
        if src is not None:
            n = src.n_tiles
            dst.skip_chunks[:B].copy_(src.skip_chunks)
            dst.tile_rows[:n].copy_(src.tile_rows)
            dst.tile_nmembers[:n].copy_(src.tile_nmembers)
            dst.tile_chunks[:n].copy_(src.tile_chunks)
        buf["shared_src"] = src
        buf["shared_B"] = B

    def run(self, ids: torch.Tensor, batch: ForwardBatch) -> torch.Tensor:
        if not self._enabled:
            return self.engine.model.forward_decode(ids, batch)
        B = ids.shape[0]
        bs = self._bucket(B)
        if bs is None or batch.block_tables.shape[1] > self.max_blocks_per_seq:
            return self.engine.model.forward_decode(ids, batch)
        if bs not in self.graphs:
            try:
                self._capture(bs)
            except Exception as e:  # capture failure: loud, then eager
                import logging

                logging.getLogger("kllms_amd.engine").error(
                    "hipGraph capture failed for batch %d (%s); falling back to eager",
                    bs, e, exc_info=True,
                )
                self._enabled = False
                self._recover_generator_state()
                return self.engine.model.forward_decode(ids, batch)
        buf = self.buffers[bs]
        if batch.shared is not None:
            if "shared" not in buf or batch.shared.n_tiles > buf["shared"].n_tiles:
                # not captured with cascade tables / more tiles than they hold
                return self.engine.model.forward_decode(ids, batch)
        if "shared" in buf:
            self._load_shared(buf, batch.shared, B)
        scratch_slot = self._scratch_block * self.engine.config.kv_block_size
        buf["ids"][:B].copy_(ids)
        buf["ids"][B:].fill_(0)
        buf["positions"][:B].copy_(batch.positions)
        buf["positions"][B:].fill_(0)
        buf["slots"][:B].copy_(batch.slot_mapping)
        buf["slots"][B:].fill_(scratch_slot)
        nb = batch.block_tables.shape[1]
        buf["block_tables"][:B, :nb].copy_(batch.block_tables)
        buf["block_tables"][:B, nb:].fill_(self._scratch_block)
        buf["block_tables"][B:].fill_(self._scratch_block)
        buf["context_lens"][:B].copy_(batch.context_lens)
        buf["context_lens"][B:].fill_(1)
        self.graphs[bs].replay()
        return self.engine.model.compute_logits(buf["out"][:B])
