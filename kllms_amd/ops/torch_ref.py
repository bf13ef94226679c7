"""Pure-PyTorch reference implementations of every engine op.

These are the numerics oracles for the HIP/CDNA4 kernels (tests compare the
kernels against these in fp32) and the CPU execution path for GPU-less test
environments. On a GPU box the dispatch layer (ops/__init__.py) routes to the
HIP kernels and refuses to fall back silently.

Conventions:
- q/k/v activations: [tokens, heads, head_dim]
- paged KV cache: [num_blocks, kv_heads, block_size, head_dim]
- cos/sin cache: [max_pos, head_dim] with cos in [:, :D/2], sin in [:, D/2:]
- logits: [batch, vocab]
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch


# --- normalization ------------------------------------------------------------

def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    norm = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (norm * weight.float()).to(x.dtype)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual' = x + residual; y = rmsnorm(residual')."""
    new_residual = (x.float() + residual.float()).to(x.dtype)
    return rmsnorm(new_residual, weight, eps), new_residual


# --- rotary embedding ---------------------------------------------------------

def build_cos_sin_cache(head_dim: int, max_pos: int, theta: float, device,
                        dtype=torch.float32, rope_scaling=None) -> torch.Tensor:
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64, device=device) / half))
    if rope_scaling:
        rt = rope_scaling.get("rope_type") or rope_scaling.get("type")
        if rt == "llama3":
            # Llama-3.1 frequency-banded NTK scaling: low-frequency bands
            # (wavelength > old context) are divided by `factor`; high-
            # frequency bands are untouched; the band between interpolates.
            import math as _math

            factor = float(rope_scaling.get("factor", 8.0))
            lo_f = float(rope_scaling.get("low_freq_factor", 1.0))
            hi_f = float(rope_scaling.get("high_freq_factor", 4.0))
            old_ctx = float(rope_scaling.get("original_max_position_embeddings", 8192))
            wavelen = 2 * _math.pi / inv_freq
            lo_wl = old_ctx / lo_f
            hi_wl = old_ctx / hi_f
            smooth = ((old_ctx / wavelen - lo_f) / (hi_f - lo_f)).clamp(0.0, 1.0)
            scaled = (1 - smooth) * inv_freq / factor + smooth * inv_freq
            inv_freq = torch.where(wavelen > lo_wl, inv_freq / factor,
                                   torch.where(wavelen < hi_wl, inv_freq, scaled))
        elif rt == "linear":
            inv_freq = inv_freq / float(rope_scaling.get("factor", 1.0))
        # unknown types: serve unscaled rather than failing (documented)
    t = torch.arange(max_pos, dtype=torch.float64, device=device)
    freqs = torch.outer(t, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).to(dtype)


def rope_inplace(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor
) -> None:
    """Llama-style (rotate-half over contiguous halves) rotary embedding,
    applied in place to q [T, H, D] and k [T, KVH, D]."""
    D = q.shape[-1]
    half = D // 2
    cs = cos_sin[positions]  # [T, D]
    cos = cs[:, :half].unsqueeze(1).float()  # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1).float()
    for t in (q, k):
        tf = t.float()
        x1 = tf[..., :half]
        x2 = tf[..., half:]
        t[..., :half] = (x1 * cos - x2 * sin).to(t.dtype)
        t[..., half:] = (x2 * cos + x1 * sin).to(t.dtype)


# --- activations --------------------------------------------------------------

def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate.dtype)


# --- fp8 (e4m3) weights -------------------------------------------------------

FP8_E4M3_MAX = 448.0


def quantize_fp8_rows(w: torch.Tensor, amax: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-output-channel e4m3 quantisation of a weight ``w`` [N, K]: returns
    ``(q, scale)`` with ``q`` float8_e4m3fn [N, K] (K-contiguous) and ``scale``
    fp32 [N], ``scale[n] = amax(|w[n, :]|) / 448`` (1.0 for an all-zero row) and
    ``q = RNE(w / scale)`` clamped to +-448, so the NaN encodings never appear.
    ``amax`` ([N] fp32) overrides the row maxima: a row-parallel shard passes
    the maximum over ALL ranks' columns so that the quantised model does not
    depend on the TP degree. The one definition for CPU and GPU (runs once at
    load)."""
    wf = w.float()
    if amax is None:
        amax = wf.abs().amax(dim=1)
    amax = amax.float()
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    q = (wf / scale.unsqueeze(1)).clamp_(-FP8_E4M3_MAX, FP8_E4M3_MAX).to(torch.float8_e4m3fn)
    return q.contiguous(), scale.contiguous()


def linear_fp8w(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(x @ q^T) * scale + bias`` for e4m3 ``q`` [N, K] with per-channel fp32
    ``scale`` [N]; any float dtype of ``x`` (fp32 accumulation, fp64 for fp64
    input). The scale multiplies the accumulated sum, never the weights."""
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    y = (x.to(acc) @ q.to(acc).t()) * scale.to(acc)
    if bias is not None:
        y = y + bias.to(acc)
    return y.to(x.dtype)


def linear_fp8w_batched(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``out[e] = (x_e @ q[e]^T) * scale[e]`` for e4m3 ``q`` [E, N, K] with fp32
    ``scale`` [E, N]; ``x`` [M, K] (shared by all experts) or [E, M, K]. fp32
    accumulation (fp64 for fp64 input); the scale multiplies the accumulated
    sum, never the weights."""
    acc = torch.float64 if x.dtype == torch.float64 else torch.float32
    y = torch.matmul(x.to(acc), q.to(acc).transpose(1, 2)) * scale.to(acc).unsqueeze(1)
    return y.to(x.dtype)


# --- paged KV cache -----------------------------------------------------------

def store_kv(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_scale=None,
    v_scale=None,
) -> None:
    """Scatter new K/V ([T, KVH, D]) into the paged caches at flat slots.

    A flat slot s addresses (block = s // block_size, offset = s % block_size).
    fp8 caches with k_scale/v_scale ([NB, KVH, BS] fp32): each (token, head)
    row is quantized with its OWN scale s = max(amax(|row|)/448, 1e-8), the
    scale written alongside — outlier rows no longer saturate e4m3.
    """
    num_blocks, kv_heads, block_size, head_dim = k_cache.shape
    blk = slot_mapping // block_size
    off = slot_mapping % block_size
    if k_scale is not None:
        sk = (k.float().abs().amax(-1) / 448.0).clamp_(min=1e-8)  # [T, KVH]
        sv = (v.float().abs().amax(-1) / 448.0).clamp_(min=1e-8)
        k_scale[blk, :, off] = sk
        v_scale[blk, :, off] = sv
        k_cache[blk, :, off, :] = (k.float() / sk.unsqueeze(-1)).to(k_cache.dtype)
        v_cache[blk, :, off, :] = (v.float() / sv.unsqueeze(-1)).to(v_cache.dtype)
        return
    k_cache[blk, :, off, :] = k.to(k_cache.dtype)
    v_cache[blk, :, off, :] = v.to(v_cache.dtype)


# --- attention ----------------------------------------------------------------

def attn_prefill_varlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    scale: float,
) -> torch.Tensor:
    """Causal varlen attention over packed sequences.

    q: [T, H, D]; k/v: [T, KVH, D] (GQA: H % KVH == 0). Returns [T, H, D].
    """
    T, H, D = q.shape
    KVH = k.shape[1]
    rep = H // KVH
    out = torch.empty_like(q)
    cu = cu_seqlens.tolist()
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        qi = q[s:e].float().permute(1, 0, 2)  # [H, L, D]
        ki = k[s:e].float().repeat_interleave(rep, dim=1).permute(1, 0, 2)
        vi = v[s:e].float().repeat_interleave(rep, dim=1).permute(1, 0, 2)
        o = torch.nn.functional.scaled_dot_product_attention(
            qi, ki, vi, is_causal=True, scale=scale
        )
        out[s:e] = o.permute(1, 0, 2).to(q.dtype)
    return out


def attn_decode_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    k_scale=None,
    v_scale=None,
) -> torch.Tensor:
    """Single-token decode attention against the paged KV cache.

    q: [B, H, D]; caches [num_blocks, KVH, block_size, D];
    block_tables: [B, max_blocks] int32; context_lens: [B] (length INCLUDING
    the token being decoded, whose K/V are already stored). k_scale/v_scale
    ([NB, KVH, BS] fp32, fp8 caches only): per-row dequant multipliers.
    """
    B, H, D = q.shape
    _, KVH, BS, _ = k_cache.shape
    rep = H // KVH
    out = torch.empty_like(q)
    for b in range(B):
        L = int(context_lens[b])
        nblk = (L + BS - 1) // BS
        blocks = block_tables[b, :nblk].long()
        kk = k_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L].float()
        vv = v_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L].float()
        if k_scale is not None:
            kk = kk * k_scale[blocks].permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
            vv = vv * v_scale[blocks].permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
        qb = q[b].float()  # [H, D]
        # per-head GQA mapping without materializing repeats
        for h in range(H):
            g = h // rep
            s = (qb[h] @ kk[g].T) * scale  # [L]
            p = torch.softmax(s, dim=-1)
            out[b, h] = (p @ vv[g]).to(q.dtype)
    return out


def attn_prefill_paged(q, k_cache, v_cache, block_tables, cu_q, q_start, scale,
                       k_scale=None, v_scale=None) -> torch.Tensor:
    """Paged (append) prefill attention, DEFINED as ``attn_decode_paged`` over
    the expanded per-token rows: packed row ``cu_q[s] + i`` gets sequence s's
    table row and ``context_lens = q_start[s] + i + 1``. block_tables is
    [n_seq, max_blocks] (one row per sequence)."""
    cu = [int(c) for c in cu_q]
    starts = [int(c) for c in q_start]
    rows, lens = [], []
    for s in range(len(starts)):
        n = cu[s + 1] - cu[s]
        rows.extend([s] * n)
        lens.extend(range(starts[s] + 1, starts[s] + n + 1))
    dev = block_tables.device
    bt = block_tables[torch.tensor(rows, dtype=torch.long, device=dev)]
    ctx = torch.tensor(lens, dtype=torch.int32, device=dev)
    return attn_decode_paged(q, k_cache, v_cache, bt, ctx, scale, k_scale, v_scale)


def paged_prefill_split_partials(q, k_cache, v_cache, meta, scale, k_scale=None, v_scale=None,
                                 p_bf16=False, kv_bf16=False, empty_init=False):
    """The split plan of ``meta`` (ops.PagedPrefill with key splits) walked
    group by group as the HIP kernel's grid does. Returns ``(out, m, l, o)``:
    out [T, H, D] fp32 holds the rows of direct-epilogue groups (NaN
    elsewhere); m, l [ws_rows, H] and o [ws_rows, H, D] are the partials, NaN
    where no group wrote (``empty_init``: the empty partial instead), so that a
    plan that leaves a slot uncovered shows in the result. ``p_bf16`` rounds
    the probabilities entering P.V to bf16 (the normaliser keeps fp32);
    ``kv_bf16`` rounds dequantised fp8 K/V to bf16, as the kernel's staging."""
    T, H, D = q.shape
    _, KVH, BS, _ = k_cache.shape
    rep = H // KVH
    cu = meta.cu_q.tolist()
    starts = meta.q_start.tolist()
    grp_seq = meta.grp_seq.tolist()
    qpos = meta.grp_qpos0.tolist()
    krange = meta.grp_krange.tolist()
    split = meta.grp_split.tolist()
    nsplit = meta.seq_nsplit.tolist()
    base = meta.seq_ws_base.tolist()
    f32 = dict(dtype=torch.float32, device=q.device)
    out = torch.full((T, H, D), float("nan"), **f32)
    W = meta.ws_rows
    if empty_init:
        pm = torch.full((W, H), float("-inf"), **f32)
        pl, po = torch.zeros((W, H), **f32), torch.zeros((W, H, D), **f32)
    else:
        pm, pl = torch.full((W, H), float("nan"), **f32), torch.full((W, H), float("nan"), **f32)
        po = torch.full((W, H, D), float("nan"), **f32)
    for g, s in enumerate(grp_seq):
        start, n = starts[s], cu[s + 1] - cu[s]
        kbeg, kend = krange[2 * g], krange[2 * g + 1]
        for r0 in qpos[8 * g: 8 * g + 8]:
            if r0 < 0 or r0 >= n:
                continue
            r1 = min(r0 + 32, n)
            k1 = min(kend, start + r1)               # the tile's causal bound
            rows = torch.arange(r0, r1, device=q.device)
            m = torch.full((r1 - r0, H), float("-inf"), **f32)
            l = torch.zeros((r1 - r0, H), **f32)
            o = torch.zeros((r1 - r0, H, D), **f32)
            if k1 > kbeg:
                j0, j1 = kbeg // BS, (k1 + BS - 1) // BS
                blocks = meta.block_tables[s, j0:j1].long()
                lo, hi = kbeg - j0 * BS, k1 - j0 * BS
                nb = j1 - j0
                kk = k_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nb * BS, D)[:, lo:hi].float()
                vv = v_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, nb * BS, D)[:, lo:hi].float()
                if k_scale is not None:
                    kk = kk * k_scale[blocks].permute(1, 0, 2).reshape(KVH, nb * BS)[:, lo:hi, None]
                    vv = vv * v_scale[blocks].permute(1, 0, 2).reshape(KVH, nb * BS)[:, lo:hi, None]
                    if kv_bf16:
                        kk, vv = kk.bfloat16().float(), vv.bfloat16().float()
                kk = kk.repeat_interleave(rep, dim=0)     # [H, keys, D]
                vv = vv.repeat_interleave(rep, dim=0)
                sc = torch.einsum("ihd,hjd->ihj", q[cu[s] + r0: cu[s] + r1].float(), kk) * scale
                keys = torch.arange(kbeg, k1, device=q.device)
                ok = keys[None, :] <= (start + rows)[:, None]          # [rows, keys]
                sc = sc.masked_fill(~ok[:, None, :], float("-inf"))
                m = sc.max(dim=-1).values
                ref = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
                p = torch.exp(sc - ref[..., None])                     # 0 where masked
                l = p.sum(dim=-1)
                if p_bf16:
                    p = p.bfloat16().float()
                o = torch.einsum("ihj,hjd->ihd", p, vv)
            if split[g] < 0:
                den = l[..., None]
                out[cu[s] + r0: cu[s] + r1] = torch.where(den > 0, o / den.clamp_min(1e-38),
                                                          torch.zeros_like(o))
            else:
                slots = base[s] + rows * nsplit[s] + split[g]
                pm[slots], pl[slots], po[slots] = m, l, o
    return out, pm, pl, po


def paged_prefill_split_merge(out, pm, pl, po, meta):
    """Merge of the partials into the rows of split sequences, in fp32 and in
    split order: w_j = exp(m_j - max_j m_j), 0 for an empty partial (l_j = 0 or
    m_j = -inf); out = sum_j w_j o_j / sum_j w_j l_j, zeros when that is 0."""
    cu = meta.cu_q.tolist()
    for s, (k, b) in enumerate(zip(meta.seq_nsplit.tolist(), meta.seq_ws_base.tolist())):
        n = cu[s + 1] - cu[s]
        if k < 2:
            continue
        H, D = po.shape[1:]
        m = pm[b: b + n * k].view(n, k, H)
        l = pl[b: b + n * k].view(n, k, H)
        o = po[b: b + n * k].view(n, k, H, D)
        empty = (l == 0) | (m == float("-inf"))
        m_all = m.masked_fill(empty, float("-inf")).max(dim=1, keepdim=True).values
        w = torch.where(empty, torch.zeros_like(m), torch.exp(m - m_all))
        acc = torch.zeros((n, H, D), dtype=torch.float32, device=po.device)
        den = torch.zeros((n, H), dtype=torch.float32, device=po.device)
        for j in range(k):
            wj = w[:, j]
            acc = acc + torch.where(empty[:, j, :, None], torch.zeros_like(acc),
                                    wj[..., None] * o[:, j])
            den = den + torch.where(empty[:, j], torch.zeros_like(den), wj * l[:, j])
        out[cu[s]: cu[s + 1]] = torch.where(den[..., None] > 0,
                                            acc / den[..., None].clamp_min(1e-38),
                                            torch.zeros_like(acc))
    return out


def attn_prefill_paged_split(q, k_cache, v_cache, meta, scale, k_scale=None, v_scale=None,
                             p_bf16=False, kv_bf16=False) -> torch.Tensor:
    """Paged prefill attention over a key-split plan: per-group partials, then
    the merge, both in fp32. Every group and key range is taken from ``meta``
    exactly as the HIP kernel takes it, so a plan that loses or repeats keys
    gives a wrong (or NaN) result here too."""
    out, pm, pl, po = paged_prefill_split_partials(q, k_cache, v_cache, meta, scale, k_scale,
                                                   v_scale, p_bf16=p_bf16, kv_bf16=kv_bf16)
    return paged_prefill_split_merge(out, pm, pl, po, meta).to(q.dtype)


def _paged_partial(qb, k_cache, v_cache, blocks_row, k0, k1, scale, k_scale, v_scale):
    """Unnormalised softmax partial of one row's heads over keys [k0, k1) read
    through ``blocks_row``: (m [H], l [H], o [H, D]) in fp32."""
    H, D = qb.shape
    _, KVH, BS, _ = k_cache.shape
    rep = H // KVH
    j0, j1 = k0 // BS, (k1 + BS - 1) // BS
    blocks = blocks_row[j0:j1].long()
    lo, hi = k0 - j0 * BS, k1 - j0 * BS
    n = j1 - j0
    kk = k_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, n * BS, D)[:, lo:hi].float()
    vv = v_cache[blocks].permute(1, 0, 2, 3).reshape(KVH, n * BS, D)[:, lo:hi].float()
    if k_scale is not None:
        kk = kk * k_scale[blocks].permute(1, 0, 2).reshape(KVH, n * BS)[:, lo:hi, None]
        vv = vv * v_scale[blocks].permute(1, 0, 2).reshape(KVH, n * BS)[:, lo:hi, None]
    kk = kk.repeat_interleave(rep, dim=0)  # [H, n, D]
    vv = vv.repeat_interleave(rep, dim=0)
    s = torch.einsum("hd,hnd->hn", qb, kk) * scale
    m = s.max(dim=-1).values
    p = torch.exp(s - m[:, None])
    return m, p.sum(dim=-1), torch.einsum("hn,hnd->hd", p, vv)


def attn_decode_paged_shared(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    k_scale=None,
    v_scale=None,
    shared=None,
    chunk_keys: int = 256,
) -> torch.Tensor:
    """Shared-prefix cascade reference, driven by the SAME metadata as the
    HIP path (``shared``: ops.SharedPrefix), so wrong metadata gives wrong
    numbers here too:

    - every tile's chunks ``< tile_chunks[t]`` are computed for each member
      row from the tile's FIRST member's block table only;
    - every row's keys from ``skip_chunks[b] * chunk_keys`` on come from its
      own block table;
    - the partials of a row are merged by log-sum-exp in fp32.
    """
    if shared is None:
        return attn_decode_paged(q, k_cache, v_cache, block_tables, context_lens, scale,
                                 k_scale, v_scale)
    B, H, D = q.shape
    skip = shared.skip_chunks.tolist()
    rows_t = shared.tile_rows.tolist()
    nmem_t = shared.tile_nmembers.tolist()
    chunks_t = shared.tile_chunks.tolist()
    parts = [[] for _ in range(B)]
    for rows, nmem, S in zip(rows_t, nmem_t, chunks_t):
        if nmem <= 0 or S <= 0:
            continue
        first = block_tables[rows[0]]
        for b in rows[:nmem]:
            if 0 <= b < B:
                parts[b].append(_paged_partial(q[b].float(), k_cache, v_cache, first,
                                               0, S * chunk_keys, scale, k_scale, v_scale))
    out = torch.empty_like(q)
    for b in range(B):
        L = int(context_lens[b])
        k0 = skip[b] * chunk_keys
        if k0 < L:
            parts[b].append(_paged_partial(q[b].float(), k_cache, v_cache, block_tables[b],
                                           k0, L, scale, k_scale, v_scale))
        if not parts[b]:
            out[b] = 0
            continue
        m = torch.stack([p[0] for p in parts[b]])          # [P, H]
        M = m.max(dim=0).values
        w = torch.exp(m - M)                                # [P, H]
        l = (torch.stack([p[1] for p in parts[b]]) * w).sum(dim=0)
        o = (torch.stack([p[2] for p in parts[b]]) * w[:, :, None]).sum(dim=0)
        out[b] = (o / l[:, None]).to(q.dtype)
    return out


# --- sampling -----------------------------------------------------------------

def _stream_generator(seed: int, step: int, device) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed((seed * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9) % (2**63))
    return g


def sample(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    seeds: torch.Tensor,
    steps: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused sampling reference.

    - mask: optional [B, ceil(V/32)] uint32 bitmask of ALLOWED tokens
      (constrained decoding); disallowed logits become -inf.
    - temperature == 0 -> greedy.
    - top_k <= 0 means no top-k; top_p >= 1 means no top-p.
    - Returns (token_ids [B], logprobs [B]) where logprob is the
      log-softmax of the MASKED, UNtempered distribution at the chosen token
      (OpenAI-style model logprob).
    """
    B, V = logits.shape
    lf = logits.float().clone()
    if mask is not None:
        bit = torch.arange(V, device=logits.device)
        allowed = (mask[:, bit // 32] >> (bit % 32).to(torch.int64)) & 1
        lf = torch.where(allowed.bool(), lf, torch.full_like(lf, float("-inf")))
    base_logprobs = torch.log_softmax(lf, dim=-1)

    tokens = torch.empty(B, dtype=torch.long, device=logits.device)
    for b in range(B):
        temp = float(temperatures[b])
        row = lf[b]
        if temp == 0.0:
            tokens[b] = torch.argmax(row)
            continue
        scaled = row / temp
        k = int(top_ks[b])
        p = float(top_ps[b])
        probs = torch.softmax(scaled, dim=-1)
        if k > 0 and k < V:
            kth = torch.topk(probs, k).values[-1]
            probs = torch.where(probs >= kth, probs, torch.zeros_like(probs))
        if p < 1.0:
            sorted_probs, sorted_idx = torch.sort(probs, descending=True)
            cumsum = torch.cumsum(sorted_probs, dim=-1)
            # keep the smallest prefix with mass >= top_p (first token always kept)
            cut = (cumsum - sorted_probs) >= p
            sorted_probs = torch.where(cut, torch.zeros_like(sorted_probs), sorted_probs)
            probs = torch.zeros_like(probs).scatter(0, sorted_idx, sorted_probs)
        probs = probs / probs.sum()
        g = _stream_generator(int(seeds[b]), int(steps[b]), logits.device)
        u = torch.rand(V, generator=g).to(logits.device)
        # Gumbel-max over the truncated renormalized distribution
        e = (-torch.log(u.clamp_min(1e-20))).clamp_min(1e-20)  # Exp(1)
        gumbel = -torch.log(e)
        masked_logp = torch.where(probs > 0, torch.log(probs), torch.full_like(probs, float("-inf")))
        tokens[b] = torch.argmax(masked_logp + gumbel)

    logprobs = base_logprobs[torch.arange(B, device=logits.device), tokens]
    return tokens, logprobs


def sample_fsm(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_ps: torch.Tensor,
    top_ks: torch.Tensor,
    seeds: torch.Tensor,
    steps: torch.Tensor,
    fsm_state: torch.Tensor,
    tables,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference for the device-resident constraint sampler.

    Gathers each stream's mask row from its tables by ``fsm_state`` (all-ones
    for an unconstrained ``None`` stream), samples through ``sample`` and
    advances every constrained state in place by walking the chosen token's
    bytes through the byte DFA. A constrained stream whose state is outside
    [0, S) is sampled unmasked and its state becomes -1."""
    B, V = logits.shape
    W = (V + 31) // 32
    states = fsm_state.tolist()
    mask = None
    if any(t is not None for t in tables):
        mask = torch.full((B, W), -1, dtype=torch.int32, device=logits.device)
        for i, t in enumerate(tables):
            if t is not None and 0 <= states[i] < t.S and t.W == W:
                mask[i] = t.mask[states[i]]
    tokens, logprobs = sample(logits, temperatures, top_ps, top_ks, seeds, steps, mask)
    toks = tokens.tolist()
    for i, t in enumerate(tables):
        if t is None:
            continue
        if 0 <= states[i] < t.S and t.W == W:
            fsm_state[i] = t.advance(states[i], toks[i])
        else:
            fsm_state[i] = -1
    return tokens, logprobs
