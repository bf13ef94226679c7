"""Float64 oracles, derived error bounds, defect "mutants" and the shared edge
cases for the HIP kernel tests (not a test module itself; imported like
``shared_prefix_cases``).

Every oracle is written straight from the op's definition in float64 and never
calls ``ops/torch_ref.py``: ``torch_ref`` is itself one of the things
``test_kernel_oracles.py`` checks against these.

Bounds
------
A kernel output ``a`` (bf16) is accepted against the float64 value ``e`` when,
for every element,

    |a - e| <= 2^-7 * |e| + c * M

- ``2^-7 * |e|`` is one bf16 ulp of the oracle (bf16 keeps 8 significant bits,
  so an ulp is at most 2^-7 relative): twice the half-ulp that the final
  round-to-nearest of a correct fp32 result costs, which leaves the other half
  for the fp32 result landing on the far side of a rounding boundary.
- ``M`` is the magnitude that the kernel's internal rounding errors scale
  with, and ``c`` the relative size of those errors:

  * attention: ``M = A = sum_j p_j * |v_j|`` (softmax-weighted mean of |V| per
    output element). A kernel that feeds bf16-rounded probabilities to the MFMA
    (prefill, the cascade group kernel) perturbs each ``p_j`` in the numerator
    by at most 2^-9 relative (half a bf16 ulp), i.e. the numerator by at most
    ``2^-9 * A``; the normaliser may carry the same again, so ``c = 2^-8``
    (``C_MFMA``). The per-stream decode kernel keeps probabilities and the
    accumulation in fp32: ``L * 2^-24`` summation error plus the ``__expf``
    argument/result error (a few 2^-22 for |s - m| < 64) stays far below
    ``c = 2^-12`` (``C_FP32``) for L <= 1025. A call that mixes both kernels
    (cascade on) uses 2^-8.
  * elementwise: ``M = T``, the sum of the absolute values of the terms that
    enter the element (``|x1*c| + |x2*s|`` for rope, ``|e|`` for the single
    product of rmsnorm / silu_mul), and ``c = 2^-18`` (``C_ELEM``): a handful
    of fp32 roundings (2^-24 each), the fp32 mean-square reduction (at most
    ~40 sequential+tree additions per lane at n = 8192) and the fast-exp
    argument error at |gate| = 30 (ulp(43.3) * ln 2 / 2 ~ 2^-19.5) all fit
    with room to spare, while a single wrong bf16 input bit (2^-8) does not.

The constants come from this arithmetic, not from what any kernel produced,
and are not to be widened; ``check`` returns the worst ``error / bound`` ratio
so tests can report the head-room.
"""

import torch

import shared_prefix_cases as sp_cases

C_MFMA = 2.0 ** -8
C_FP32 = 2.0 ** -12
C_ELEM = 2.0 ** -18
ULP = 2.0 ** -7

F64 = torch.float64


def f64(t):
    """Exact widening of bf16 / fp8 / fp32 data to float64."""
    if t.dtype in (torch.float8_e4m3fn, torch.bfloat16):
        return t.float().to(F64)
    return t.to(F64)


def round_bf16(t64):
    """float64 -> (fp32 RNE) -> (bf16 RNE) -> float64, the kernels' own
    two-step rounding of an fp32 value to bf16."""
    return t64.float().bfloat16().float().to(F64)


# --- the bound checker ----------------------------------------------------------

def check(actual, e, mag, c):
    """Worst ``|a - e| / (2^-7 |e| + c * mag)`` and the (unravelled) index of
    that element. A zero bound with a zero error counts as ratio 0 (the
    all-zero rmsnorm row must come out exactly 0), with any error as inf."""
    a = f64(actual.detach().cpu())
    assert a.shape == e.shape, (a.shape, e.shape)
    err = (a - e).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    bound = ULP * e.abs() + c * mag
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    flat = int(ratio.reshape(-1).argmax())
    idx = []
    for s in reversed(e.shape):
        idx.append(flat % s)
        flat //= s
    return float(ratio.max()), tuple(reversed(idx))


def describe(kernel, case, ratio, idx, names, extra=""):
    where = ", ".join(f"{n}={i}" for n, i in zip(names, idx))
    return f"{kernel} [{case}]: worst error/bound {ratio:.3f} at {where}{extra}"


# --- elementwise oracles --------------------------------------------------------

def rmsnorm(x, w, eps):
    """y = x / sqrt(mean(x^2) + eps) * w. Returns (e, T) with T = |e|."""
    xd, wd = f64(x), f64(w)
    e = xd / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps) * wd
    return e, e.abs()


def fused_add_rmsnorm(x, r, w, eps):
    """The kernel's contract: residual' = bf16(fp32(x) + fp32(r)), written
    back, and y = rmsnorm(residual'). Returns (residual' bf16, e, T)."""
    res = (x.float() + r.float()).bfloat16()
    e, t = rmsnorm(res, w, eps)
    return res, e, t


def silu_mul(gate, up):
    """out = gate / (1 + exp(-gate)) * up. Returns (e, T) with T = |e|."""
    g, u = f64(gate), f64(up)
    e = g / (1.0 + torch.exp(-g)) * u
    return e, e.abs()


def rope(x, positions, cos_sin):
    """Rotate-half rotary embedding of x [T, heads, D] with the half-split
    cache layout (cos in [:, :D/2], sin in [:, D/2:]). Returns (e, T)."""
    D = x.shape[-1]
    half = D // 2
    cs = f64(cos_sin)[positions.long()]
    c = cs[:, :half].unsqueeze(1)
    s = cs[:, half:].unsqueeze(1)
    xd = f64(x)
    x1, x2 = xd[..., :half], xd[..., half:]
    e = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    t = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return e, t


def store_kv(k, v, k_cache, v_cache, slots):
    """bf16 scatter: token t's [KVH, D] rows go to (slot // BS, :, slot % BS).
    Returns the expected caches (bit-exact copies of the inputs elsewhere)."""
    BS = k_cache.shape[2]
    kc, vc = k_cache.clone(), v_cache.clone()
    for t, s in enumerate(slots.tolist()):
        kc[s // BS, :, s % BS, :] = k[t]
        vc[s // BS, :, s % BS, :] = v[t]
    return kc, vc


def store_kv_fp8(k, v, k_cache, v_cache, k_scale, v_scale, slots):
    """Per-row e4m3 quantisation: s = max(amax|row| / 448, 1e-8), code =
    fp8(x / s). Returns the expected (k_cache, v_cache, k_scale, v_scale)."""
    BS = k_cache.shape[2]
    kc, vc, ks, vs = k_cache.clone(), v_cache.clone(), k_scale.clone(), v_scale.clone()
    for src, cache, sc in ((k, kc, ks), (v, vc, vs)):
        xd = f64(src)
        s = (xd.abs().amax(-1) / 448.0).clamp_min(1e-8)          # [T, KVH]
        codes = (xd / s.unsqueeze(-1)).float().to(torch.float8_e4m3fn)
        for t, slot in enumerate(slots.tolist()):
            cache[slot // BS, :, slot % BS, :] = codes[t]
            sc[slot // BS, :, slot % BS] = s[t].float()
    return kc, vc, ks, vs


# --- attention oracles ----------------------------------------------------------

def _softmax_pv(s, vv, p_bf16):
    """s [H, L] scores, vv [H, L, D]. Returns (e, A). ``p_bf16`` emulates the
    MFMA kernels: exp(s - m) is rounded to bf16 for the PV product while the
    normaliser sums the unrounded fp32 values."""
    if s.shape[1] == 0:
        z = torch.zeros(vv.shape[0], vv.shape[2], dtype=F64)
        return z, z.clone()
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    if p_bf16:
        p32 = p.float()
        num = p32.bfloat16().float().to(F64)
        p = num / p32.to(F64).sum(-1, keepdim=True)
    else:
        p = p / p.sum(-1, keepdim=True)
    e = torch.einsum("hl,hld->hd", p, vv)
    a = torch.einsum("hl,hld->hd", p, vv.abs())
    return e, a


def attn_decode(q, k_cache, v_cache, block_tables, context_lens, scale,
                k_scale=None, v_scale=None, *, round_kv_bf16=False,
                keep=None, head_map=None, p_bf16=False):
    """Paged single-token decode attention, float64.

    q [B, H, D]; caches [NB, KVH, BS, D] (bf16 or fp8); row b attends to the
    first ``context_lens[b]`` keys reached through ``block_tables[b]``; q-head
    h reads kv-head ``h // (H // KVH)``. ``k_scale``/``v_scale`` [NB, KVH, BS]
    are per-row dequant multipliers. ``round_kv_bf16``: True rounds every
    dequantised K/V value to bf16 first (the cascade group kernel converts
    fp8 * scale to bf16 before its MFMA); a per-row list of key counts rounds
    only each row's leading keys (the ones that kernel covers).

    ``keep(b, L)`` (bool [L] or None) and ``head_map(h)`` exist for the
    mutants. Returns (e, A), both [B, H, D] float64."""
    B, H, D = q.shape
    _, KVH, BS, _ = k_cache.shape
    rep = H // KVH
    hm = head_map or (lambda h: h // rep)
    gidx = torch.tensor([hm(h) for h in range(H)])
    qd = f64(q)
    e_out = torch.zeros(B, H, D, dtype=F64)
    a_out = torch.zeros(B, H, D, dtype=F64)
    for b in range(B):
        L = int(context_lens[b])
        nblk = (L + BS - 1) // BS
        blocks = block_tables[b, :nblk].long()
        kk = f64(k_cache[blocks]).permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L]
        vv = f64(v_cache[blocks]).permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L]
        if k_scale is not None:
            kk = kk * f64(k_scale[blocks]).permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
            vv = vv * f64(v_scale[blocks]).permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
        if round_kv_bf16 is not False:
            n = L if round_kv_bf16 is True else min(L, int(round_kv_bf16[b]))
            kk = torch.cat([round_bf16(kk[:, :n]), kk[:, n:]], dim=1)
            vv = torch.cat([round_bf16(vv[:, :n]), vv[:, n:]], dim=1)
        if keep is not None:
            mask = keep(b, L)
            if mask is not None:
                kk, vv = kk[:, mask], vv[:, mask]
        kh, vh = kk[gidx], vv[gidx]                      # [H, L, D]
        s = torch.einsum("hd,hld->hl", qd[b], kh) * scale
        e_out[b], a_out[b] = _softmax_pv(s, vh, p_bf16)
    return e_out, a_out


def attn_prefill(q, k, v, cu_seqlens, scale, *, keep=None, head_map=None, p_bf16=False):
    """Causal attention over packed sequences, float64. q [T, H, D], k/v
    [T, KVH, D]; token i of a sequence attends to tokens 0..i of the same
    sequence. ``keep(L)`` (bool [L, L] rows x keys, or None) and ``head_map``
    exist for the mutants. Returns (e, A), both [T, H, D] float64."""
    T, H, D = q.shape
    KVH = k.shape[1]
    rep = H // KVH
    hm = head_map or (lambda h: h // rep)
    gidx = torch.tensor([hm(h) for h in range(H)])
    qd, kd, vd = f64(q), f64(k), f64(v)
    e_out = torch.zeros(T, H, D, dtype=F64)
    a_out = torch.zeros(T, H, D, dtype=F64)
    cu = [int(c) for c in cu_seqlens]
    for i in range(len(cu) - 1):
        s0, s1 = cu[i], cu[i + 1]
        L = s1 - s0
        allow = torch.ones(L, L, dtype=torch.bool).tril()
        if keep is not None:
            extra = keep(L)
            if extra is not None:
                allow = allow & extra
        kh = kd[s0:s1][:, gidx].permute(1, 0, 2)          # [H, L, D]
        vh = vd[s0:s1][:, gidx].permute(1, 0, 2)
        s = torch.einsum("lhd,hjd->hlj", qd[s0:s1], kh) * scale
        s = s.masked_fill(~allow, float("-inf"))
        m = s.max(dim=-1, keepdim=True).values
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.exp(s - m)
        den = p.sum(-1, keepdim=True)
        if p_bf16:
            p32 = p.float()
            den = p32.to(F64).sum(-1, keepdim=True)
            p = p32.bfloat16().float().to(F64)
        p = torch.where(den > 0, p / den.clamp_min(1e-300), torch.zeros_like(p))
        e_out[s0:s1] = torch.einsum("hlj,hjd->lhd", p, vh)
        a_out[s0:s1] = torch.einsum("hlj,hjd->lhd", p, vh.abs())
    return e_out, a_out


# --- mutants: the oracle with a classic kernel defect ---------------------------
# Each takes the case dict and returns the mutated float64 output, or None when
# the case holds no key the defect would touch.

def _decode(case, **kw):
    return attn_decode(case["q"], case["kc"], case["vc"], case["bt"], case["lens"],
                       case["scale"], case.get("ks"), case.get("vs"),
                       round_kv_bf16=case.get("round_kv", False), **kw)[0]


def _drop_range(case, lo_of, hi_of, applies):
    lens = case["lens"].tolist()
    if not any(applies(L) for L in lens):
        return None

    def keep(b, L):
        if not applies(L):
            return None
        m = torch.ones(L, dtype=torch.bool)
        m[lo_of(L):hi_of(L)] = False
        return m

    return _decode(case, keep=keep)


def decode_drop_last_key(case):
    """context_lens off by one: every row with more than one key loses its last."""
    return _drop_range(case, lambda L: L - 1, lambda L: L, lambda L: L > 1)


def decode_drop_key_255(case):
    """The last key of the first 256-key split-K chunk is lost."""
    return _drop_range(case, lambda L: 255, lambda L: 256, lambda L: L > 255)


def decode_drop_keys_512_528(case):
    """The 16 keys after two full chunks are lost (the shared remainder that
    the cascade hands back to the per-stream kernel)."""
    return _drop_range(case, lambda L: 512, lambda L: min(L, 528), lambda L: L > 512)


def decode_drop_tail_block(case):
    """The trailing partial KV block is lost."""
    BS = case["kc"].shape[2]
    return _drop_range(case, lambda L: L // BS * BS, lambda L: L,
                       lambda L: L % BS != 0 and L > BS)


def decode_wrong_block(case):
    """One block-table entry of the median-length row points at another
    (valid) block."""
    lens = case["lens"].tolist()
    BS = case["kc"].shape[2]
    order = sorted(range(len(lens)), key=lambda b: lens[b])
    b = order[len(order) // 2]
    nblk = (lens[b] + BS - 1) // BS
    j = nblk // 2
    other = order[-1] if order[-1] != b else order[0]
    bt = case["bt"].clone()
    new = int(case["bt"][other, 0])
    if new == int(bt[b, j]):
        return None
    bt[b, j] = new
    return _decode(dict(case, bt=bt))


def wrong_head_map(case, prefill=False):
    """q-head h reads kv-head ``h % KVH`` instead of ``h // rep``."""
    H = case["q"].shape[1]
    KVH = case["k"].shape[1] if prefill else case["kc"].shape[1]
    rep = H // KVH
    if all(h % KVH == h // rep for h in range(H)):
        return None
    hm = lambda h: h % KVH
    return _prefill(case, head_map=hm) if prefill else _decode(case, head_map=hm)


def _prefill(case, **kw):
    return attn_prefill(case["q"], case["k"], case["v"], case["cu"], case["scale"], **kw)[0]


def _prefill_keep(case, applies, fn):
    if not any(applies(L) for L in case["seqlens"]):
        return None

    def keep(L):
        if not applies(L):
            return None
        m = torch.ones(L, L, dtype=torch.bool)
        fn(m, L)
        return m

    return _prefill(case, keep=keep)


def prefill_drop_diagonal(case):
    """Causal mask off by one: rows >= 1 do not see their own key."""
    def fn(m, L):
        i = torch.arange(1, L)
        m[i, i] = False
    return _prefill_keep(case, lambda L: L > 1, fn)


def prefill_drop_key_256(case):
    """Rows > 256 (the second workgroup of a sequence) lose key 256."""
    def fn(m, L):
        m[257:, 256] = False
    return _prefill_keep(case, lambda L: L > 257, fn)


def prefill_tail_tile_blind(case):
    """The rows of the tail 64-key tile do not see that tile's keys."""
    def fn(m, L):
        t0 = (L - 1) // 64 * 64
        m[t0:, t0:] = False
    return _prefill_keep(case, lambda L: (L - 1) // 64 * 64 > 0, fn)


def misread_contiguous(view):
    """What a kernel that ignored its token-stride argument would read: the
    view's shape laid out densely from the view's first element."""
    strides = []
    n = 1
    for s in reversed(view.shape):
        strides.append(n)
        n *= s
    return torch.as_strided(view, tuple(view.shape), tuple(reversed(strides)),
                            view.storage_offset())


def decode_stride_ignored(case):
    qm = misread_contiguous(case["q"])
    if torch.equal(qm, case["q"]):
        return None
    return _decode(dict(case, q=qm))


def prefill_stride_ignored(case, which):
    m = misread_contiguous(case[which])
    if torch.equal(m, case[which]):
        return None
    return _prefill(dict(case, **{which: m}))


DECODE_MUTANTS = {
    "last key dropped": decode_drop_last_key,
    "key 255 dropped": decode_drop_key_255,
    "keys [512, 528) dropped": decode_drop_keys_512_528,
    "tail partial block dropped": decode_drop_tail_block,
    "one block-table entry replaced": decode_wrong_block,
    "head map h % KVH": wrong_head_map,
    "q token stride ignored": decode_stride_ignored,
}

PREFILL_MUTANTS = {
    "diagonal key dropped": prefill_drop_diagonal,
    "key 256 dropped for rows > 256": prefill_drop_key_256,
    "tail tile blind": prefill_tail_tile_blind,
    "head map h % KVH": lambda c: wrong_head_map(c, prefill=True),
    "q token stride ignored": lambda c: prefill_stride_ignored(c, "q"),
    "k token stride ignored": lambda c: prefill_stride_ignored(c, "k"),
    "v token stride ignored": lambda c: prefill_stride_ignored(c, "v"),
}


# --- shared cases (CPU tensors; the GPU tests move them to the device) ----------

KVH, D = 2, 128
JUNK = 100.0
DECODE_CTX = [1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025]
PREFILL_SEQLENS = [[1], [31], [32], [33], [63], [64], [65], [255], [256], [257], [289],
                   [33, 1, 64, 257]]
PREFILL_HEADS = [(4, 4), (8, 2)]

_cases = {}


def _cached(key, fn):
    if key not in _cases:
        _cases[key] = fn()
    return _cases[key]


def _junk_tail(kc, vc, block, ctx, BS):
    """Slots of a row's last block past its context hold the junk constant."""
    if ctx % BS:
        kc[block, :, ctx % BS:, :] = JUNK
        vc[block, :, ctx % BS:, :] = JUNK


def _quantise_fp8(kc, vc, edit):
    """Quantise bf16 caches with ``torch_ref.store_kv`` (per-row scales) after
    ``edit(k_rows, v_rows)`` changed the [NB * BS, KVH, D] rows in place."""
    from kllms_amd.ops import torch_ref

    NB, KVH_, BS, D_ = kc.shape
    k_rows = kc.permute(0, 2, 1, 3).reshape(NB * BS, KVH_, D_).clone()
    v_rows = vc.permute(0, 2, 1, 3).reshape(NB * BS, KVH_, D_).clone()
    edit(k_rows, v_rows)
    kc8 = torch.zeros(NB, KVH_, BS, D_, dtype=torch.float8_e4m3fn)
    vc8 = torch.zeros_like(kc8)
    ks = torch.ones(NB, KVH_, BS)
    vs = torch.ones(NB, KVH_, BS)
    torch_ref.store_kv(k_rows, v_rows, kc8, vc8, torch.arange(NB * BS), ks, vs)
    return kc8, vc8, ks, vs


def decode_case(gqa, BS=16, fp8=False):
    """Per-stream decode: ctx = DECODE_CTX, disjoint random block tables two
    entries wider than any row needs, q a strided view into a fused
    [B, (H + 2 KVH) D] buffer, every table entry and cache slot past a row's
    context valid and filled with 100.0."""
    def build():
        g = torch.Generator().manual_seed(1000 + 10 * gqa + BS)
        H = KVH * gqa
        B = len(DECODE_CTX)
        need = [(c + BS - 1) // BS for c in DECODE_CTX]
        n_junk = 8
        NB = sum(need) + n_junk
        max_blocks = max(need) + 2
        kc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
        vc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
        perm = torch.randperm(NB - n_junk, generator=g).tolist()
        junk = list(range(NB - n_junk, NB))
        kc[junk] = JUNK
        vc[junk] = JUNK
        bt = torch.tensor([[junk[(b + j) % n_junk] for j in range(max_blocks)]
                           for b in range(B)], dtype=torch.int32)
        it = iter(perm)
        slot_of = {}
        for b in range(B):
            for j in range(need[b]):
                bt[b, j] = next(it)
            _junk_tail(kc, vc, int(bt[b, need[b] - 1]), DECODE_CTX[b], BS)
            slot_of[b] = lambda key, b=b: int(bt[b, key // BS]) * BS + key % BS
        fused = (torch.randn(B, (H + 2 * KVH) * D, generator=g) * 4.0).bfloat16()
        q = fused[:, : H * D].view(B, H, D)
        case = {"name": f"decode gqa={gqa} BS={BS}" + (" fp8" if fp8 else ""),
                "gqa": gqa, "fused": fused, "q": q, "kc": kc, "vc": vc, "bt": bt,
                "lens": torch.tensor(DECODE_CTX, dtype=torch.int32),
                "scale": D ** -0.5, "c": C_FP32}
        if fp8:
            # x4 row inside the ctx=1025 row, 800.0 outlier inside the ctx=513 row
            def edit(k_rows, v_rows):
                k_rows[slot_of[B - 1](700)] *= 4.0
                v_rows[slot_of[B - 1](700)] *= 4.0
                k_rows[slot_of[B - 2](300), 1, 7] = 800.0

            kc8, vc8, ks, vs = _quantise_fp8(kc, vc, edit)
            case.update(kc=kc8, vc=vc8, ks=ks, vs=vs)
        return case

    return _cached(("decode", gqa, BS, fp8), build)


def cascade_case(gqa, fp8=False):
    """The ``shared_prefix_cases`` batch with a peaked q (x8: std 4), junk
    padding (table entries past each row's blocks point at the reserved junk
    blocks, filled with 100.0 like the slots past each context) and the
    metadata of ``build_shared_prefix_tiles``."""
    def build():
        b = sp_cases.build_batch(gqa)
        BS = sp_cases.BS
        kc, vc = b["kc"].clone(), b["vc"].clone()
        junk = list(range(sp_cases.NB - sp_cases.JUNK_BLOCKS, sp_cases.NB))
        kc[junk] = JUNK
        vc[junk] = JUNK
        bt = b["bt"].clone()
        lens = b["lens"].tolist()
        for r, blocks in enumerate(b["block_lists"]):
            for j in range(len(blocks), bt.shape[1]):
                bt[r, j] = junk[(r + j) % len(junk)]
            _junk_tail(kc, vc, blocks[-1], lens[r], BS)
        tiles = sp_cases.build_tiles(b)
        H = KVH * gqa
        B = len(lens)
        fused = torch.zeros(B, (H + 2 * KVH) * D, dtype=torch.bfloat16)
        fused[:, : H * D] = (b["q"].float() * 8.0).bfloat16().reshape(B, H * D)
        g = torch.Generator().manual_seed(7)
        fused[:, H * D:] = (torch.randn(B, 2 * KVH * D, generator=g) * 4.0).bfloat16()
        case = {"name": f"cascade gqa={gqa}" + (" fp8" if fp8 else ""), "gqa": gqa,
                "fused": fused, "q": fused[:, : H * D].view(B, H, D), "kc": kc, "vc": vc,
                "bt": bt, "lens": b["lens"], "scale": b["scale"], "tiles": tiles,
                "c": C_MFMA}
        if fp8:
            # per-row scales of different sizes; K rows are only ever scaled
            # DOWN (a x4 key row would own the softmax and blind the test to
            # every other key)
            def edit(k_rows, v_rows):
                k_rows[::3] *= 0.5
                v_rows[1::5] *= 0.25

            kc8, vc8, ks, vs = _quantise_fp8(kc, vc, edit)
            # the group kernel rounds dequantised K/V to bf16; it covers each
            # row's first skip*256 keys
            case.update(kc=kc8, vc=vc8, ks=ks, vs=vs,
                        round_kv=[s * 256 for s in tiles.skip])
        return case

    return _cached(("cascade", gqa, fp8), build)


def prefill_case(seqlens, H, KVH_):
    """Packed causal prefill; q/k/v are strided views of one fused
    [T, (H + 2 KVH) D] buffer (q std 4, k and v std 0.5)."""
    def build():
        g = torch.Generator().manual_seed(2000 + sum(seqlens) * 7 + H)
        T = sum(seqlens)
        W = (H + 2 * KVH_) * D
        fused = torch.empty(T, W, dtype=torch.bfloat16)
        fused[:, : H * D] = (torch.randn(T, H * D, generator=g) * 4.0).bfloat16()
        fused[:, H * D:] = (torch.randn(T, 2 * KVH_ * D, generator=g) * 0.5).bfloat16()
        cu = [0]
        for L in seqlens:
            cu.append(cu[-1] + L)
        return {"name": f"prefill {seqlens} H={H} KVH={KVH_}", "seqlens": list(seqlens),
                "fused": fused,
                "q": fused[:, : H * D].view(T, H, D),
                "k": fused[:, H * D: (H + KVH_) * D].view(T, KVH_, D),
                "v": fused[:, (H + KVH_) * D:].view(T, KVH_, D),
                "cu": torch.tensor(cu, dtype=torch.int32), "scale": D ** -0.5, "c": C_MFMA}

    return _cached(("prefill", tuple(seqlens), H, KVH_), build)


def decode_oracle(case):
    """(e, A) of a decode / cascade case, computed once."""
    return _cached(("oracle", case["name"]), lambda: attn_decode(
        case["q"], case["kc"], case["vc"], case["bt"], case["lens"], case["scale"],
        case.get("ks"), case.get("vs"), round_kv_bf16=case.get("round_kv", False)))


def prefill_oracle(case):
    return _cached(("oracle", case["name"]), lambda: attn_prefill(
        case["q"], case["k"], case["v"], case["cu"], case["scale"]))


def query_pos(case, t):
    """(sequence, position) of packed token t."""
    cu = case["cu"].tolist()
    for i in range(len(cu) - 1):
        if cu[i] <= t < cu[i + 1]:
            return i, t - cu[i]
    raise IndexError(t)


# elementwise cases

RMSNORM_SHAPES = [(rows, n) for n in (8, 136, 2048, 2056, 8192) for rows in (1, 3)]
ROPE_SHAPES = [(Dh, H, KVH_, T) for Dh in (64, 128) for (H, KVH_) in ((4, 2), (1, 1))
               for T in (1, 33)]
SILU_SHAPES = [(T, I) for I in (8, 1024) for T in (1, 7)]
STORE_SHAPES = [(Dh, BS, T) for Dh in (64, 128) for BS in (16, 32) for T in (1, 50)]
ROPE_MAX_POS = 512
EPS = 1e-5


def rmsnorm_case(rows, n):
    """x, residual r, weight with mean 1; with 3 rows, row 1 is all zeros
    (and r = -x there, so the fused sum is exactly zero too)."""
    def build():
        g = torch.Generator().manual_seed(3000 + n + rows)
        x = torch.randn(rows, n, generator=g).bfloat16()
        r = torch.randn(rows, n, generator=g).bfloat16()
        w = (torch.randn(n, generator=g) * 0.5 + 1.0).bfloat16()
        xz = x.clone()
        if rows > 1:
            xz[1] = 0
            r[1] = -x[1]
        return {"name": f"rows={rows} n={n}", "x": xz, "xr": x, "r": r, "w": w,
                "zero_row": 1 if rows > 1 else None}

    return _cached(("rmsnorm", rows, n), build)


def rope_case(Dh, H, KVH_, T):
    from kllms_amd.ops import torch_ref

    def build():
        g = torch.Generator().manual_seed(4000 + Dh + 10 * H + T)
        W = (H + 2 * KVH_) * Dh
        fused = torch.randn(T, W, generator=g).bfloat16()
        pos = torch.randint(0, ROPE_MAX_POS, (T,), generator=g)
        pos[-1] = ROPE_MAX_POS - 1
        if T > 1:
            pos[0] = 0
        return {"name": f"D={Dh} H={H} KVH={KVH_} T={T}", "fused": fused, "pos": pos,
                "H": H, "KVH": KVH_, "D": Dh,
                "cs": torch_ref.build_cos_sin_cache(Dh, ROPE_MAX_POS, 10000.0, "cpu")}

    return _cached(("rope", Dh, H, KVH_, T), build)


def qkv_views(fused, H, KVH_, Dh):
    T = fused.shape[0]
    return (fused[:, : H * Dh].view(T, H, Dh),
            fused[:, H * Dh: (H + KVH_) * Dh].view(T, KVH_, Dh),
            fused[:, (H + KVH_) * Dh:].view(T, KVH_, Dh))


def silu_case(T, I, fused=True):
    """gate/up as the halves of one [T, 2I] buffer (or two contiguous
    tensors); gate holds +-30 and 0."""
    def build():
        g = torch.Generator().manual_seed(5000 + T + I)
        if fused:
            buf = (torch.randn(T, 2 * I, generator=g) * 2.0).bfloat16()
            gate, up = buf[:, :I], buf[:, I:]
        else:
            buf = None
            gate = (torch.randn(T, I, generator=g) * 2.0).bfloat16()
            up = (torch.randn(T, I, generator=g) * 2.0).bfloat16()
        gate[0, 0], gate[0, 1], gate[0, 2] = 30.0, -30.0, 0.0
        gate[-1, -1], gate[-1, -2], gate[-1, -3] = -30.0, 30.0, 0.0
        return {"name": f"T={T} I={I} {'fused' if fused else 'contiguous'}",
                "buf": buf, "gate": gate, "up": up}

    return _cached(("silu", T, I, fused), build)


def store_case(Dh, BS, T, KVH_=2, fp8=False, zero_row=False):
    """Strided k/v views of a fused buffer, random distinct slots, caches
    pre-filled with a non-zero pattern."""
    def build():
        g = torch.Generator().manual_seed(6000 + Dh + BS + T + KVH_)
        H = 2 * KVH_
        fused = torch.randn(T, (H + 2 * KVH_) * Dh, generator=g).bfloat16()
        _, k, v = qkv_views(fused, H, KVH_, Dh)
        if zero_row:
            k[T // 2, 0] = 0
            v[T // 2, KVH_ - 1] = 0
        NB = (T + BS - 1) // BS + 3
        slots = torch.randperm(NB * BS, generator=g)[:T]
        case = {"name": f"D={Dh} BS={BS} T={T} KVH={KVH_}" + (" fp8" if fp8 else ""),
                "fused": fused, "H": H, "KVH": KVH_, "D": Dh, "k": k, "v": v,
                "slots": slots, "zero": (T // 2) if zero_row else None}
        if fp8:
            pat = torch.randn(NB, KVH_, BS, Dh, generator=g)
            case["kc"] = pat.to(torch.float8_e4m3fn)
            case["vc"] = (pat * 2).to(torch.float8_e4m3fn)
            case["ks"] = torch.rand(NB, KVH_, BS, generator=g) + 0.5
            case["vs"] = torch.rand(NB, KVH_, BS, generator=g) + 0.5
        else:
            case["kc"] = (torch.randn(NB, KVH_, BS, Dh, generator=g) + 3.0).bfloat16()
            case["vc"] = (torch.randn(NB, KVH_, BS, Dh, generator=g) - 3.0).bfloat16()
        return case

    return _cached(("store", Dh, BS, T, KVH_, fp8, zero_row), build)


def check_store_fp8(kc, vc, ks, vs, want, msg):
    """The criteria of ``test_gpu_kernels::TestFp8KVCacheGPU``, unchanged:
    scales at rtol 1e-6, dequantised difference <= 32 * s_max, fewer than 1%
    of the bytes differing."""
    wkc, wvc, wks, wvs = want
    for got_c, got_s, ref_c, ref_s, nm in ((kc, ks, wkc, wks, "K"), (vc, vs, wvc, wvs, "V")):
        got_c, got_s = got_c.cpu(), got_s.cpu()
        assert torch.allclose(got_s, ref_s, rtol=1e-6), f"{msg}: per-row {nm} scales diverge"
        deq = got_c.float() * got_s.unsqueeze(-1)
        ref = ref_c.float() * ref_s.unsqueeze(-1)
        thresh = got_s.max().item() * 32 + 1e-6
        diff = (deq - ref).abs().max().item()
        assert diff <= thresh, f"{msg}: {nm} dequantised diff {diff} > {thresh}"
        frac = (got_c.view(torch.uint8) != ref_c.view(torch.uint8)).float().mean().item()
        assert frac < 0.01, f"{msg}: {frac:.4f} of the {nm} bytes differ"
