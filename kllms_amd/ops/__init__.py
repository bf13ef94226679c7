"""Op dispatch: HIP/CDNA4 kernels on GPU, torch reference on CPU.

Policy (BASELINE north star): on a GPU (`tensor.is_cuda`, which on
PyTorch-ROCm means an AMD GPU) the hand-written gfx950 HIP kernels in
``kllms_amd._C`` are the ONLY path — if the extension is missing the op
RAISES instead of silently falling back to eager PyTorch. On CPU the pure
torch reference implementations (torch_ref.py) run, which is what the
GPU-less CI environment uses.

Set ``KLLMS_AMD_FORCE_TORCH_OPS=1`` to force the torch path on GPU (used only
by numerics tests to produce the oracle on-device).
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import torch_ref

_C = None
_C_err: Optional[str] = None
try:
    from kllms_amd import _C  # type: ignore[no-redef]  # built by setup.py build_ext --inplace
except Exception as e:  # pragma: no cover - import-time probe
    _C = None
    _C_err = str(e)


def hip_available() -> bool:
    return _C is not None


def _force_torch() -> bool:
    return os.environ.get("KLLMS_AMD_FORCE_TORCH_OPS", "0") == "1"


def _hip_or_raise():
    if _C is None:
        raise RuntimeError(
            "kllms_amd HIP extension (kllms_amd/_C*.so) is not built but a GPU "
            "tensor was passed. Build it with `python setup.py build_ext --inplace` "
            f"(PYTORCH_ROCM_ARCH=gfx950). Import error: {_C_err}"
        )
    return _C


def _scale_or_empty(scale: Optional[torch.Tensor], device: torch.device) -> torch.Tensor:
    """The binding takes an empty tensor for 'bf16 weights or caches, no scales'."""
    return scale if scale is not None else torch.empty(0, dtype=torch.float32, device=device)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda and not _force_torch():
        out = torch.empty_like(x)
        _hip_or_raise().rmsnorm(out, x, weight, eps)
        return out
    return torch_ref.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    if x.is_cuda and not _force_torch():
        # in-place: residual += x; x_out = rmsnorm(residual)
        out = torch.empty_like(x)
        _hip_or_raise().fused_add_rmsnorm(out, x, residual, weight, eps)
        return out, residual
    return torch_ref.fused_add_rmsnorm(x, residual, weight, eps)


def rope_inplace(q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> None:
    if q.is_cuda and not _force_torch():
        _hip_or_raise().rope_inplace(q, k, positions, cos_sin)
        return
    torch_ref.rope_inplace(q, k, positions, cos_sin)


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if gate.is_cuda and not _force_torch():
        out = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
        _hip_or_raise().silu_mul(out, gate, up)
        return out
    return torch_ref.silu_mul(gate, up)


quantize_fp8_rows = torch_ref.quantize_fp8_rows

# the shapes the HIP weight-only fp8 GEMM takes (linear_fp8w.hip)
FP8W_MAX_M = 256


def _fp8w_kernel_takes(x: torch.Tensor, N: int, K: int) -> bool:
    return (x.dtype == torch.bfloat16 and 1 <= x.shape[0] <= FP8W_MAX_M
            and K % 64 == 0 and N % 16 == 0
            and x.stride(1) == 1 and x.stride(0) >= K and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0)


def linear_fp8w(
    x: torch.Tensor,
    q: torch.Tensor,
    scale: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    scratch: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``(x @ q^T) * scale + bias`` with weight-only fp8: ``q`` e4m3 [N, K],
    ``scale`` fp32 [N] (``quantize_fp8_rows``), ``x`` [..., K].

    On the GPU, bf16 ``x`` with 1 <= M <= 256, K % 64 == 0 and N % 16 == 0 runs
    the HIP kernel (exact e4m3 x bf16 products, fp32 accumulation, scale and
    bias on the fp32 sum). Anything else -- packed prefill above 256 rows, or
    a shape the kernel does not take -- dequantises the weight with a second
    HIP kernel into ``scratch`` (a reusable bf16 buffer of at least N*K
    elements; allocated per call when None) and runs the library GEMM on it.
    """
    if x.is_cuda and not _force_torch():
        C = _hip_or_raise()
        N, K = q.shape
        x2 = x if x.dim() == 2 else x.reshape(-1, K)
        if x2.dtype != torch.bfloat16:
            raise ValueError(f"linear_fp8w on GPU needs bf16 activations, got {x2.dtype}")
        none = torch.empty(0, dtype=torch.bfloat16, device=x.device)
        if _fp8w_kernel_takes(x2, N, K):
            out = torch.empty((x2.shape[0], N), dtype=torch.bfloat16, device=x.device)
            C.linear_fp8w(out, x2, q, scale, bias if bias is not None else none)
        else:
            if scratch is None or scratch.numel() < N * K:
                scratch = torch.empty(N * K, dtype=torch.bfloat16, device=x.device)
            C.dequant_fp8w(scratch, q, scale)
            out = torch.nn.functional.linear(x2, scratch[: N * K].view(N, K), bias)
        return out if x.dim() == 2 else out.view(*x.shape[:-1], N)
    return torch_ref.linear_fp8w(x, q, scale, bias)


def _fp8w_batched_kernel_takes(x: torch.Tensor, E: int, N: int, K: int) -> bool:
    rows = x if x.dim() == 2 else x[0]
    return (_fp8w_kernel_takes(rows, N, K) and 1 <= E <= 1024
            and (x.dim() == 2 or x.stride(0) % 8 == 0))


def linear_fp8w_batched(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``out[e] = (x_e @ q[e]^T) * scale[e]`` for the E experts of a MoE layer:
    ``q`` e4m3 [E, N, K], ``scale`` fp32 [E, N]; ``x`` is [M, K] (one
    activation shared by all experts) or [E, M, K] (one per expert). Returns
    [E, M, N] in the dtype of ``x``.

    On the GPU, bf16 ``x`` with 1 <= M <= 256, K % 64 == 0 and N % 16 == 0 runs
    ONE batched launch of the ``linear_fp8w`` kernel (expert index in the
    grid); at E = 1 it gives the bits of ``linear_fp8w``. Anything else
    dequantises the experts to bf16 and runs ``torch.bmm``, like the large-M
    branch of ``linear_fp8w``."""
    E, N, K = q.shape
    if x.is_cuda and not _force_torch():
        C = _hip_or_raise()
        if x.dtype != torch.bfloat16:
            raise ValueError(f"linear_fp8w_batched on GPU needs bf16 activations, got {x.dtype}")
        if _fp8w_batched_kernel_takes(x, E, N, K):
            out = torch.empty((E, x.shape[-2], N), dtype=torch.bfloat16, device=x.device)
            C.linear_fp8w_batched(out, x, q, scale)
            return out
        if K % 16 == 0:
            w = torch.empty((E, N, K), dtype=torch.bfloat16, device=x.device)
            C.dequant_fp8w(w, q.view(E * N, K), scale.view(E * N))
        else:       # the dequant kernel converts 16 weights per thread
            w = (q.float() * scale.unsqueeze(-1)).bfloat16()
        xb = x.unsqueeze(0).expand(E, -1, -1) if x.dim() == 2 else x
        return torch.bmm(xb, w.transpose(1, 2))
    return torch_ref.linear_fp8w_batched(x, q, scale)


def store_kv(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> None:
    """k_scale/v_scale: [NB, KVH, BS] fp32 per-row dequant scales, REQUIRED
    when the caches are fp8 (written here: s = amax(|row|)/448), None for bf16."""
    if k.is_cuda and not _force_torch():
        _hip_or_raise().store_kv(
            k, v, k_cache, v_cache, slot_mapping,
            _scale_or_empty(k_scale, k.device), _scale_or_empty(v_scale, k.device))
        return
    torch_ref.store_kv(k, v, k_cache, v_cache, slot_mapping, k_scale, v_scale)


def rope_store_kv(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    positions: torch.Tensor,
    cos_sin: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> None:
    """``rope_inplace(q, k, ...)`` followed by ``store_kv(k, v, ...)`` as ONE
    kernel on the GPU: q and k are rotated in place, the rotated k and the
    untouched v go to the paged caches at ``slot_mapping``. q, k, both caches
    and (fp8) both scale arrays end up with the bits of the two separate ops."""
    if q.is_cuda and not _force_torch():
        _hip_or_raise().rope_store_kv(
            q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping,
            _scale_or_empty(k_scale, q.device), _scale_or_empty(v_scale, q.device))
        return
    torch_ref.rope_inplace(q, k, positions, cos_sin)
    torch_ref.store_kv(k, v, k_cache, v_cache, slot_mapping, k_scale, v_scale)


def copy_kv_blocks(a_all: torch.Tensor, b_all: torch.Tensor,
                   src: torch.Tensor, dst: torch.Tensor) -> None:
    """Copy blocks ``src[i] -> dst[i]`` (int32 [n], on the arrays' device) of
    the two ``[L, NB, ...]`` arrays ``a_all`` and ``b_all`` in every layer: one
    HIP launch on the GPU, torch indexing on the CPU. A source may repeat; the
    caller guarantees that no block is both a source and a destination."""
    if src.numel() == 0:
        return
    if a_all.is_cuda and not _force_torch():
        _hip_or_raise().copy_kv_blocks(a_all, b_all, src, dst)
        return
    s, d = src.long(), dst.long()
    a_all[:, d] = a_all[:, s]
    b_all[:, d] = b_all[:, s]


def _prefill_tiles(cu_seqlens: torch.Tensor, device) -> tuple:
    """Grouped q-tile metadata for the MFMA prefill kernel: 32-row q-tiles of
    each sequence packed 8 per workgroup (the 8 waves share the K/V LDS
    staging); idle wave slots padded with -1. One host round-trip per prefill
    batch (once per generate() call)."""
    NW = 8
    cu = cu_seqlens.cpu().tolist()
    grp_start, grp_len, grp_qpos0 = [], [], []
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        L = e - s
        tiles = list(range(0, L, 32))
        for g0 in range(0, len(tiles), NW):
            grp_start.append(s)
            grp_len.append(L)
            grp = tiles[g0 : g0 + NW]
            grp_qpos0.extend(grp + [-1] * (NW - len(grp)))
    t = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
    return t(grp_start), t(grp_qpos0), t(grp_len)


def attn_prefill_varlen(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens: torch.Tensor, scale: float
) -> torch.Tensor:
    if q.is_cuda and not _force_torch():
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        gs, gq, gl = _prefill_tiles(cu_seqlens, q.device)
        _hip_or_raise().attn_prefill(out, q, k, v, gs, gq, gl, scale)
        return out
    return torch_ref.attn_prefill_varlen(q, k, v, cu_seqlens, scale)


@dataclass
class SharedPrefix:
    """Shared-prefix (cascade) decode-attention metadata, int32 tensors on the
    batch's device (engine.shared_prefix.build_shared_prefix_tiles):
    skip_chunks [B] — leading 256-key chunks of each row that the group kernel
    computes; tile_rows [n_tiles, 64] — member batch rows of each tile;
    tile_nmembers [n_tiles]; tile_chunks [n_tiles] — shared chunks per tile.
    The first member's block table addresses a tile's shared K/V."""

    skip_chunks: torch.Tensor
    tile_rows: torch.Tensor
    tile_nmembers: torch.Tensor
    tile_chunks: torch.Tensor

    @property
    def n_tiles(self) -> int:
        return int(self.tile_nmembers.shape[0])


def attn_decode_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    shared: Optional[SharedPrefix] = None,
) -> torch.Tensor:
    """``shared`` (optional) turns on the shared-prefix cascade: each tile's
    shared K/V chunks are read once for all of its rows, the per-stream
    kernel covers the rest. ``None`` is the per-stream path alone."""
    if q.is_cuda and not _force_torch():
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ks, vs = _scale_or_empty(k_scale, q.device), _scale_or_empty(v_scale, q.device)
        if shared is None:
            _hip_or_raise().attn_decode_paged(
                out, q, k_cache, v_cache, block_tables, context_lens, scale, ks, vs)
        else:
            _hip_or_raise().attn_decode_paged_shared(
                out, q, k_cache, v_cache, block_tables, context_lens, scale, ks, vs,
                shared.skip_chunks, shared.tile_rows, shared.tile_nmembers, shared.tile_chunks)
        return out
    if shared is not None:
        return torch_ref.attn_decode_paged_shared(
            q, k_cache, v_cache, block_tables, context_lens, scale, k_scale, v_scale, shared)
    return torch_ref.attn_decode_paged(q, k_cache, v_cache, block_tables, context_lens, scale,
                                       k_scale, v_scale)


@dataclass
class PagedPrefill:
    """Paged (append / extend) prefill-attention metadata, int32 tensors on the
    batch's device (``build_paged_prefill``): cu_q [n_seq + 1] — packed row
    range of each sequence's new tokens; q_start [n_seq] — keys already in the
    cache; block_tables [n_seq, max_blocks] — ONE table row per sequence;
    grp_seq [G] and grp_qpos0 [G * 8] — per workgroup its sequence and the
    first row (relative to cu_q) of each wave's 32-row q-tile, -1 = idle.

    With key splits (``key_splits`` != 1 chose to split at least one
    sequence; None / 0 / 1 otherwise): grp_krange [G * 2] — the workgroup's
    key range [kbeg, kend), kbeg a multiple of 64; grp_split [G] — its split
    index, -1 for a workgroup of an unsplit sequence (whole range, writes the
    output itself); seq_nsplit [n_seq] — splits of the sequence (1 = unsplit);
    seq_ws_base [n_seq] — its first partial slot, row i / split j of the
    sequence owning slot ``base + i * nsplit + j``; ws_rows — slots in all;
    max_splits — the largest seq_nsplit."""

    cu_q: torch.Tensor
    q_start: torch.Tensor
    block_tables: torch.Tensor
    grp_seq: torch.Tensor
    grp_qpos0: torch.Tensor
    grp_krange: Optional[torch.Tensor] = None
    grp_split: Optional[torch.Tensor] = None
    seq_nsplit: Optional[torch.Tensor] = None
    seq_ws_base: Optional[torch.Tensor] = None
    ws_rows: int = 0
    max_splits: int = 1

    @property
    def n_seq(self) -> int:
        return int(self.q_start.shape[0])

    @property
    def n_groups(self) -> int:
        return int(self.grp_seq.shape[0])

    @property
    def has_splits(self) -> bool:
        return self.grp_split is not None


PAGED_PREFILL_WAVES = 8     # q-tile slots per workgroup (attn_prefill_paged.hip)
PAGED_PREFILL_QBLK = 32
PAGED_PREFILL_KVBLK = 64    # keys per round: the unit key ranges are cut in
PAGED_PREFILL_MAX_SPLITS = 64
# partial workspace budget: (128 + 2) fp32 per (slot, q-head); splits are
# reduced rather than exceed it
PAGED_PREFILL_WS_BYTES = 256 << 20
PAGED_PREFILL_WS_CELL_BYTES = (128 + 2) * 4
# the budget is checked against this many q-heads when the caller names none
PAGED_PREFILL_WS_HEADS = 128
# auto (key_splits=0) tunables, from the "Paged prefill attention: key splits"
# table of profiles/README.md: a split keeps at least this many 64-key rounds
# (64 rows after 1024 keys, 17 rounds: 8 splits of 2-3 rounds took 21.9 us, 4
# splits 23.9 us, 16 splits of 1-2 rounds 36.3 us — below 2 rounds the fixed
# cost of a workgroup, its Q fragments, first unoverlapped gather, partial
# write and merge, outweighs the shorter loop), and a batch that is split
# packs all of a sequence's q-tiles (up to 8) into one workgroup, so each key
# range is read once per head (the packing every forced count was timed with).
PAGED_PREFILL_AUTO_MIN_ROUNDS = 2
PAGED_PREFILL_AUTO_TILES = 8


def _device_cu_count(device) -> Optional[int]:
    """Compute units of ``device`` from its properties; None off the GPU."""
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        return None
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _auto_key_splits(q_lens, q_starts, tiles_per_group, default_tpg, num_q_heads, num_cus):
    """(per-sequence split counts, tiles per group) of auto mode, or None to
    keep the unsplit plan."""
    NW, QB, KB = PAGED_PREFILL_WAVES, PAGED_PREFILL_QBLK, PAGED_PREFILL_KVBLK
    if num_cus is None:
        return None
    tiles = [(L + QB - 1) // QB for L in q_lens]
    groups = sum((t + default_tpg - 1) // default_tpg for t in tiles)
    if groups * num_q_heads >= num_cus:
        return None
    tpg = PAGED_PREFILL_AUTO_TILES if tiles_per_group is None else tiles_per_group
    packed = sum((t + tpg - 1) // tpg for t in tiles)
    k = min(num_cus // (packed * num_q_heads), PAGED_PREFILL_MAX_SPLITS)
    per_seq = []
    for L, s0 in zip(q_lens, q_starts):
        rounds = (s0 + L + KB - 1) // KB
        per_seq.append(max(1, min(k, rounds // PAGED_PREFILL_AUTO_MIN_ROUNDS)))
    if max(per_seq) < 2:
        return None
    return per_seq, tpg


def build_paged_prefill(q_lens, q_starts, block_lists, device, block_size: int,
                        tiles_per_group: Optional[int] = None, key_splits: int = 1,
                        num_q_heads: Optional[int] = None,
                        num_cus: Optional[int] = None) -> PagedPrefill:
    """Build ``PagedPrefill`` from Python lists in one host pass: sequence s
    appends ``q_lens[s]`` >= 1 tokens after ``q_starts[s]`` >= 0 cached keys and
    owns the physical blocks ``block_lists[s]`` (of ``block_size`` slots).

    Every 32-row q-tile of every sequence lands in exactly one workgroup slot;
    a workgroup holds tiles of one sequence only and pads with -1.
    ``tiles_per_group`` (1..8) is how many tiles share a workgroup's K/V
    staging; None picks 8 once the batch has 64 tiles and fewer below, so that
    a short append still spreads over enough workgroups. Raises when a
    sequence's ``start + len`` does not fit its blocks.

    ``key_splits``: 1 — every workgroup walks all of its keys (the fields
    above only). k >= 2 — each sequence's ``ceil((start + len) / 64)`` rounds
    are spread as evenly as possible over up to k contiguous key ranges (never
    more ranges than rounds, at most 64); every q-tile group then has one
    workgroup per range, which writes a partial that a reduce kernel merges.
    0 — auto: split only when the unsplit plan has fewer workgroups
    (groups x ``num_q_heads``, required here) than the device has compute
    units (``num_cus``, default: the device's properties; never on the CPU);
    then all of a sequence's q-tiles share a workgroup and the split count
    brings the workgroup count up to the CU count, each split keeping at least
    ``PAGED_PREFILL_AUTO_MIN_ROUNDS`` rounds. Where auto does not split it
    returns exactly the ``key_splits=1`` plan. Split counts are reduced until
    the partial workspace fits ``PAGED_PREFILL_WS_BYTES``."""
    NW, QB, KB = PAGED_PREFILL_WAVES, PAGED_PREFILL_QBLK, PAGED_PREFILL_KVBLK
    if not (len(q_lens) == len(q_starts) == len(block_lists)) or len(q_lens) == 0:
        raise ValueError("build_paged_prefill: need one q_len, q_start and block list per sequence")
    if isinstance(key_splits, bool) or not isinstance(key_splits, int) or key_splits < 0:
        raise ValueError(f"build_paged_prefill: key_splits must be an integer >= 0, got {key_splits!r}")
    if key_splits == 0 and num_q_heads is None:
        raise ValueError("build_paged_prefill: key_splits=0 (auto) needs num_q_heads")
    if num_q_heads is not None and num_q_heads < 1:
        raise ValueError(f"build_paged_prefill: num_q_heads {num_q_heads} out of range")
    n_tiles = 0
    for L, s0, blocks in zip(q_lens, q_starts, block_lists):
        if L < 1 or s0 < 0:
            raise ValueError(f"build_paged_prefill: q_len {L} / q_start {s0} out of range")
        if s0 + L > len(blocks) * block_size:
            raise ValueError(
                f"build_paged_prefill: start {s0} + len {L} exceeds the sequence's "
                f"{len(blocks)} blocks of {block_size}")
        n_tiles += (L + QB - 1) // QB
    if tiles_per_group is not None and not 1 <= tiles_per_group <= NW:
        raise ValueError(f"build_paged_prefill: tiles_per_group must be 1..{NW}")
    default_tpg = min(NW, max(1, n_tiles // 8))
    nsplit = [1] * len(q_lens)
    if key_splits == 0:
        auto = _auto_key_splits(q_lens, q_starts, tiles_per_group, default_tpg, num_q_heads,
                                num_cus if num_cus is not None else _device_cu_count(device))
        if auto is not None:
            nsplit, tiles_per_group = auto
    elif key_splits >= 2:
        nsplit = [min(key_splits, PAGED_PREFILL_MAX_SPLITS, (s0 + L + KB - 1) // KB)
                  for L, s0 in zip(q_lens, q_starts)]
    if tiles_per_group is None:
        tiles_per_group = default_tpg
    # the workspace budget: take a split off the most-split sequences until
    # the partials fit
    cell = PAGED_PREFILL_WS_CELL_BYTES * (num_q_heads or PAGED_PREFILL_WS_HEADS)
    while sum(L * k for L, k in zip(q_lens, nsplit) if k > 1) * cell > PAGED_PREFILL_WS_BYTES:
        top = max(nsplit)
        nsplit = [k - 1 if k == top else k for k in nsplit]
    split = max(nsplit) > 1
    max_nb = max(len(b) for b in block_lists)
    cu = [0]
    table, grp_seq, grp_qpos0, grp_krange, grp_split, ws_base = [], [], [], [], [], []
    ws_rows = 0
    for s, (L, s0, blocks) in enumerate(zip(q_lens, q_starts, block_lists)):
        cu.append(cu[-1] + L)
        table.append(list(blocks) + [0] * (max_nb - len(blocks)))
        k = nsplit[s]
        if k > 1:
            # rounds spread evenly: the first (rounds % k) ranges get one more
            rounds = (s0 + L + KB - 1) // KB
            edges = [(j * (rounds // k) + min(j, rounds % k)) * KB for j in range(k + 1)]
            ranges = [(edges[j], min(edges[j + 1], s0 + L), j) for j in range(k)]
            ws_base.append(ws_rows)
            ws_rows += L * k
        else:
            ranges = [(0, 0x7FFFFFFF, -1)]
            ws_base.append(0)
        tiles = list(range(0, L, QB))
        for g0 in range(0, len(tiles), tiles_per_group):
            grp = tiles[g0: g0 + tiles_per_group]
            for kbeg, kend, j in ranges:
                grp_seq.append(s)
                grp_qpos0.extend(grp + [-1] * (NW - len(grp)))
                grp_krange.extend((kbeg, kend))
                grp_split.append(j)
    t = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
    meta = PagedPrefill(cu_q=t(cu), q_start=t(list(q_starts)), block_tables=t(table),
                        grp_seq=t(grp_seq), grp_qpos0=t(grp_qpos0))
    if split:
        meta.grp_krange, meta.grp_split = t(grp_krange), t(grp_split)
        meta.seq_nsplit, meta.seq_ws_base = t(nsplit), t(ws_base)
        meta.ws_rows, meta.max_splits = ws_rows, max(nsplit)
    return meta


def attn_prefill_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    meta: PagedPrefill,
    scale: float,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Causal attention of newly appended tokens over the paged cache: packed
    row ``cu_q[s] + i`` attends to keys ``0 .. q_start[s] + i`` of sequence s,
    all read from the cache (``store_kv`` has already written the new ones).
    On the GPU this is the MFMA kernel of attn_prefill_paged.hip; elsewhere
    ``torch_ref.attn_prefill_paged``, which is ``attn_decode_paged`` over the
    per-token rows. Metadata with key splits runs the split kernel and its
    reduce over a workspace allocated here (prefill is not graph-captured);
    elsewhere ``torch_ref.attn_prefill_paged_split`` walks the same plan."""
    if q.is_cuda and not _force_torch():
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        ks, vs = _scale_or_empty(k_scale, q.device), _scale_or_empty(v_scale, q.device)
        if meta.has_splits:
            H = q.shape[1]
            part_o = torch.empty((meta.ws_rows, H, 128), dtype=torch.float32, device=q.device)
            part_ml = torch.empty((meta.ws_rows, H, 2), dtype=torch.float32, device=q.device)
            _hip_or_raise().attn_prefill_paged_split(
                out, q, k_cache, v_cache, meta.block_tables, meta.cu_q, meta.q_start,
                meta.grp_seq, meta.grp_qpos0, meta.grp_krange, meta.grp_split,
                meta.seq_nsplit, meta.seq_ws_base, part_o, part_ml, meta.ws_rows,
                meta.max_splits, scale, ks, vs)
            return out
        _hip_or_raise().attn_prefill_paged(
            out, q, k_cache, v_cache, meta.block_tables, meta.cu_q, meta.q_start,
            meta.grp_seq, meta.grp_qpos0, scale, ks, vs)
        return out
    if meta.has_splits:
        return torch_ref.attn_prefill_paged_split(q, k_cache, v_cache, meta, scale,
                                                  k_scale, v_scale)
    return torch_ref.attn_prefill_paged(q, k_cache, v_cache, meta.block_tables, meta.cu_q,
                                        meta.q_start, scale, k_scale, v_scale)


def sample(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    seeds: torch.Tensor,
    steps: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    dbg: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    if logits.is_cuda and not _force_torch():
        B = logits.shape[0]
        tokens = torch.empty(B, dtype=torch.long, device=logits.device)
        logprobs = torch.empty(B, dtype=torch.float32, device=logits.device)
        _hip_or_raise().sample(
            tokens, logprobs, logits, temperatures, top_ps, top_ks, seeds, steps,
            mask if mask is not None else torch.empty(0, dtype=torch.int32, device=logits.device),
            dbg if dbg is not None else torch.empty(0, dtype=torch.float32, device=logits.device),
        )
        return tokens, logprobs
    return torch_ref.sample(logits, temperatures, top_ps, top_ks, seeds, steps, mask)


def fsm_descriptor(tables, device) -> torch.Tensor:
    """[B, 6] int64 descriptor for sample_fsm: per stream the device addresses
    of mask / trans / tok_off / tok_bytes, then S and W; an all-zero row for
    an unconstrained stream (``None``)."""
    rows = [t.descriptor() if t is not None else [0] * 6 for t in tables]
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 6).to(device)


def _fsm_eos(tables) -> int:
    eos = {t.eos_id for t in tables if t is not None}
    if len(eos) > 1:
        raise ValueError(f"sample_fsm: streams disagree on eos_id: {sorted(eos)}")
    return eos.pop() if eos else -1


def sample_fsm(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    seeds: torch.Tensor,
    steps: torch.Tensor,
    fsm_state: torch.Tensor,
    tables,
    tabs: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Constrained sampling with the DFA state on the device.

    ``fsm_state`` ([B] int32) is each stream's DFA state: the kernel gathers
    the stream's mask row from its device table by state, samples exactly as
    ``sample`` does, and advances the state IN PLACE by the chosen token. A
    constrained stream whose state is outside its table is sampled unmasked
    and its state set to -1 for the caller to turn into an error.

    ``tables`` is the per-stream list of constrained.DeviceTables (``None``
    for an unconstrained stream: no mask, state untouched); the caller keeps
    them alive until the launch has run. ``tabs`` is ``fsm_descriptor(tables)``
    when the caller has it cached.
    """
    B = logits.shape[0]
    if len(tables) != B:
        raise ValueError(f"sample_fsm: {len(tables)} tables for {B} rows")
    if logits.is_cuda and not _force_torch():
        if tabs is None:
            tabs = fsm_descriptor(tables, logits.device)
        tokens = torch.empty(B, dtype=torch.long, device=logits.device)
        logprobs = torch.empty(B, dtype=torch.float32, device=logits.device)
        _hip_or_raise().sample_fsm(
            tokens, logprobs, logits, temperatures, top_ps, top_ks, seeds, steps,
            fsm_state, tabs, _fsm_eos(tables),
        )
        return tokens, logprobs
    return torch_ref.sample_fsm(logits, temperatures, top_ps, top_ks, seeds, steps,
                                fsm_state, tables)


def moe_gateup(
    act: torch.Tensor,
    x: torch.Tensor,
    w_gate_up: torch.Tensor,
    sorted_ids: torch.Tensor,
    pad_offsets: torch.Tensor,
    zeros: torch.Tensor,
    scale: Optional[torch.Tensor] = None,
) -> None:
    """Grouped MoE gate/up GEMM + fused silu*mul into `act` (sorted-by-expert
    row space). GPU-only (Mixtral prefill hot path); the CPU path keeps the
    per-expert torch loop in models/mixtral.py. With ``scale`` (fp32
    [E, 2*IN]) ``w_gate_up`` is e4m3 and the fp8 instantiation runs."""
    _hip_or_raise().moe_gateup(act, x, w_gate_up, _scale_or_empty(scale, x.device),
                               sorted_ids, pad_offsets, zeros)


def moe_down(
    y: torch.Tensor,
    act: torch.Tensor,
    w_down: torch.Tensor,
    pad_offsets: torch.Tensor,
    scale: Optional[torch.Tensor] = None,
) -> None:
    """Grouped MoE down GEMM in sorted-row space (see moe_gateup); ``scale``
    (fp32 [E, H]) goes with e4m3 ``w_down``."""
    _hip_or_raise().moe_down(y, act, w_down, _scale_or_empty(scale, act.device), pad_offsets)


def levenshtein_pairs(
    chars: torch.Tensor,
    lens: torch.Tensor,
    pair_i: torch.Tensor,
    pair_j: torch.Tensor,
) -> torch.Tensor:
    """Batched Myers bit-parallel edit distance over packed [N, 64] uint8
    normalized strings; returns int32 distances per (i, j) pair. GPU-only —
    the CPU consensus path keeps the pure-python DP (utils/text.py)."""
    return _hip_or_raise().levenshtein_pairs(chars, lens, pair_i, pair_j)
