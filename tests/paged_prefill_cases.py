"""Cases, float64 oracle and defect "mutants" for paged (append / extend)
prefill attention (not a test module itself; imported like ``kernel_oracles``).

Semantics under test: sequence s has ``start`` keys already in the paged cache
and ``n`` new tokens packed at rows ``cu[s]..cu[s+1]``; row i attends to keys
``0 .. start + i`` inclusive, all read from the cache through the sequence's
ONE block-table row; q-head h reads kv-head ``h // (H // KVH)``.

The oracle is written from that definition in float64 and never calls
``ops/torch_ref.py``. Outputs are accepted by ``kernel_oracles.check`` with
``C_MFMA`` (bf16 probabilities into the MFMA, fp32 normaliser: the packed
prefill kernel's own criterion, derived in that module's docstring).

Data follows ``kernel_oracles.decode_case`` / ``prefill_case``: q std 4 as a
strided view into a fused [T, (H + 2 KVH) * 128] buffer, K/V std 0.5, disjoint
random block tables two entries wider than any sequence needs, every table
entry and cache slot past a sequence's ``start + n`` valid and filled with
100.0, so a read past the end shows in the numbers and no index leaves the
cache.
"""

import torch

import kernel_oracles as ko
from kernel_oracles import C_MFMA, JUNK, _quantise_fp8, check, f64, round_bf16  # noqa: F401

D = 128
F64 = torch.float64

# (start, q_len) per sequence: starts on and off block multiples, the 32-row
# and 64-key tile edges on both sides of the prefix boundary, a second
# workgroup of one sequence (257 rows = 9 tiles), idle waves
CASES = [
    [(0, 1)], [(0, 33)], [(16, 1)], [(16, 31)], [(48, 32)], [(100, 33)], [(255, 65)],
    [(256, 64)], [(257, 257)], [(512, 8)],
    [(16, 33), (0, 1), (320, 64), (100, 257)],
]
MULTI = CASES[-1]
BS32_CASES = [[(16, 31)], [(100, 33)], [(257, 257)], MULTI]

# (H, KVH, BS, fp8, cases)
CONFIGS = [
    (4, 4, 16, False, CASES),
    (8, 2, 16, False, CASES),
    (8, 2, 32, False, BS32_CASES),
    (8, 2, 16, True, CASES),
]


def case_id(seqs):
    return "_".join(f"{s}+{n}" for s, n in seqs)


def all_params():
    """(seqs, H, KVH, BS, fp8) of every case x configuration, with ids."""
    params, ids = [], []
    for H, KVH, BS, fp8, cases in CONFIGS:
        for seqs in cases:
            params.append((seqs, H, KVH, BS, fp8))
            ids.append(f"{case_id(seqs)}-H{H}KVH{KVH}-BS{BS}-{'fp8' if fp8 else 'bf16'}")
    return params, ids


_cases = {}


def _cached(key, fn):
    if key not in _cases:
        _cases[key] = fn()
    return _cases[key]


def make_case(seqs, H, KVH, BS=16, fp8=False):
    def build():
        g = torch.Generator().manual_seed(
            7000 + 13 * sum(s + 3 * n for s, n in seqs) + 5 * H + KVH + BS)
        tot = [s + n for s, n in seqs]
        need = [(t + BS - 1) // BS for t in tot]
        n_junk = 8
        NB = sum(need) + n_junk
        max_blocks = max(need) + 2
        kc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
        vc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
        junk = list(range(NB - n_junk, NB))
        kc[junk] = JUNK
        vc[junk] = JUNK
        it = iter(torch.randperm(NB - n_junk, generator=g).tolist())
        bt = torch.tensor([[junk[(s + j) % n_junk] for j in range(max_blocks)]
                           for s in range(len(seqs))], dtype=torch.int32)
        block_lists = []
        for s in range(len(seqs)):
            blocks = [next(it) for _ in range(need[s])]
            block_lists.append(blocks)
            bt[s, : need[s]] = torch.tensor(blocks, dtype=torch.int32)
            if tot[s] % BS:
                kc[blocks[-1], :, tot[s] % BS:, :] = JUNK
                vc[blocks[-1], :, tot[s] % BS:, :] = JUNK
        T = sum(n for _, n in seqs)
        fused = (torch.randn(T, (H + 2 * KVH) * D, generator=g) * 4.0).bfloat16()
        cu = [0]
        for _, n in seqs:
            cu.append(cu[-1] + n)
        case = {"name": f"paged prefill {case_id(seqs)} H={H} KVH={KVH} BS={BS}"
                        + (" fp8" if fp8 else ""),
                "seqs": list(seqs), "H": H, "KVH": KVH, "BS": BS, "fp8": fp8,
                "fused": fused, "q": fused[:, : H * D].view(T, H, D), "kc": kc, "vc": vc,
                "bt": bt, "block_lists": block_lists, "cu": cu,
                "starts": [s for s, _ in seqs], "lens": [n for _, n in seqs],
                "scale": D ** -0.5}
        if fp8:
            # per-row scales of different sizes; K rows are only ever scaled
            # DOWN (a scaled-up key row would own the softmax and blind the
            # test to every other key)
            def edit(k_rows, v_rows):
                k_rows[::3] *= 0.5
                v_rows[1::5] *= 0.25

            kc8, vc8, ks, vs = _quantise_fp8(kc, vc, edit)
            case.update(kc=kc8, vc=vc8, ks=ks, vs=vs)
        return case

    return _cached(("case", tuple(seqs), H, KVH, BS, fp8), build)


def permuted(case):
    """The same logical case with every physical block moved (caches, scales
    and table permuted together)."""
    def build():
        NB = case["kc"].shape[0]
        g = torch.Generator().manual_seed(99)
        perm = torch.randperm(NB, generator=g)          # old block b -> perm[b]
        out = dict(case, name=case["name"] + " permuted")
        for key in ("kc", "vc", "ks", "vs"):
            if case.get(key) is not None:
                new = torch.empty_like(case[key])
                new[perm] = case[key]
                out[key] = new
        out["bt"] = perm[case["bt"].long()].to(torch.int32)
        out["block_lists"] = [[int(perm[b]) for b in blocks] for blocks in case["block_lists"]]
        return out

    return _cached(("permuted", case["name"]), build)


# --- the float64 oracle ---------------------------------------------------------

def causal(start, n):
    """allow[i, j]: row i of the n new tokens sees key j <= start + i."""
    j = torch.arange(start + n).unsqueeze(0)
    i = torch.arange(n).unsqueeze(1)
    return j <= start + i


def oracle(case, *, round_kv_bf16=False, p_bf16=False, allow=None, head_map=None,
           bt=None, q=None):
    """(e, A), both [T, H, D] float64, A = sum_j p_j |v_j|.

    ``round_kv_bf16`` rounds dequantised fp8 K/V to bf16 first, as the HIP
    kernel does on the way into LDS. ``p_bf16`` emulates a correct kernel
    (bf16-rounded probabilities, fp32 normaliser). ``allow(s, start, n)``
    (bool [n, start + n], or None for causal), ``head_map``, ``bt`` and ``q``
    exist for the mutants. A row left without keys gives zeros."""
    H, KVH, BS = case["H"], case["KVH"], case["BS"]
    rep = H // KVH
    hm = head_map or (lambda h: h // rep)
    gidx = torch.tensor([hm(h) for h in range(H)])
    qd = f64(case["q"] if q is None else q)
    table = case["bt"] if bt is None else bt
    T = qd.shape[0]
    e_out = torch.zeros(T, H, D, dtype=F64)
    a_out = torch.zeros(T, H, D, dtype=F64)
    for s, (start, n) in enumerate(case["seqs"]):
        L = start + n
        nblk = (L + BS - 1) // BS
        blocks = table[s, :nblk].long()
        kk = f64(case["kc"][blocks]).permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L]
        vv = f64(case["vc"][blocks]).permute(1, 0, 2, 3).reshape(KVH, nblk * BS, D)[:, :L]
        if case.get("ks") is not None:
            kk = kk * f64(case["ks"][blocks]).permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
            vv = vv * f64(case["vs"][blocks]).permute(1, 0, 2).reshape(KVH, nblk * BS)[:, :L, None]
            if round_kv_bf16:
                kk, vv = round_bf16(kk), round_bf16(vv)
        kh, vh = kk[gidx], vv[gidx]                           # [H, L, D]
        r0 = case["cu"][s]
        ok = causal(start, n)
        if allow is not None:
            m = allow(s, start, n)
            if m is not None:
                ok = m
        sc = torch.einsum("ihd,hjd->hij", qd[r0: r0 + n], kh) * case["scale"]
        sc = sc.masked_fill(~ok, float("-inf"))
        mx = sc.max(dim=-1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        p = torch.exp(sc - mx)
        den = p.sum(-1, keepdim=True)
        if p_bf16:
            p32 = p.float()
            den = p32.to(F64).sum(-1, keepdim=True)
            p = p32.bfloat16().float().to(F64)
        p = torch.where(den > 0, p / den.clamp_min(1e-300), torch.zeros_like(p))
        e_out[r0: r0 + n] = torch.einsum("hij,hjd->ihd", p, vh)
        a_out[r0: r0 + n] = torch.einsum("hij,hjd->ihd", p, vh.abs())
    return e_out, a_out


def case_oracle(case, round_kv_bf16=False):
    """(e, A) of a case, computed once per rounding mode."""
    rk = bool(round_kv_bf16 and case["fp8"])
    return _cached(("oracle", case["name"], rk), lambda: oracle(case, round_kv_bf16=rk))


def expanded_rows(case):
    """(block_tables [T, max_blocks], context_lens [T]) of the per-token decode
    rows the op is defined over."""
    rows, lens = [], []
    for s, (start, n) in enumerate(case["seqs"]):
        rows.extend([s] * n)
        lens.extend(range(start + 1, start + n + 1))
    return case["bt"][torch.tensor(rows)], torch.tensor(lens, dtype=torch.int32)


def row_of(case, t):
    """(sequence, row within its new tokens) of packed row t."""
    cu = case["cu"]
    for s in range(len(cu) - 1):
        if cu[s] <= t < cu[s + 1]:
            return s, t - cu[s]
    raise IndexError(t)


def where(case):
    def fn(idx):
        s, i = row_of(case, idx[0])
        start, n = case["seqs"][s]
        return f", sequence={s} (start {start}, len {n}), row={i}"
    return fn


# --- mutants: the oracle with one defect ----------------------------------------
# Each returns the mutated float64 output, or None when the case holds nothing
# the defect would touch.

def _masked(case, applies, edit):
    """``edit(m, start, n)`` changes the causal mask of every sequence that
    ``applies(start, n)``."""
    if not any(applies(s, n) for s, n in case["seqs"]):
        return None

    def allow(s, start, n):
        if not applies(start, n):
            return None
        m = causal(start, n)
        edit(m, start, n)
        return m

    return oracle(case, allow=allow)[0]


def drop_own_key(case):
    """Causal mask off by one: a row does not see its own (diagonal) key.
    (The very first row of a sequence without a prefix keeps it: it has no
    other key.)"""
    def edit(m, start, n):
        i = torch.arange(n)
        i = i[start + i >= 1]
        m[i, start + i] = False
    return _masked(case, lambda start, n: start + n > 1, edit)


def prefix_offset_forgotten(case):
    """Row i sees only keys <= i: q_start never added to the causal limit."""
    def edit(m, start, n):
        m &= torch.arange(start + n).unsqueeze(0) <= torch.arange(n).unsqueeze(1)
    return _masked(case, lambda start, n: start > 0, edit)


def prefix_invisible(case):
    """The cached prefix is not read at all."""
    def edit(m, start, n):
        m[:, :start] = False
    return _masked(case, lambda start, n: start > 0, edit)


def drop_last_prefix_key(case):
    """Key start-1, the last one before the new tokens, is lost."""
    def edit(m, start, n):
        m[:, start - 1] = False
    return _masked(case, lambda start, n: start > 0, edit)


def drop_first_new_key(case):
    """Key ``start``, the first new one, is lost for rows >= 1."""
    def edit(m, start, n):
        m[1:, start] = False
    return _masked(case, lambda start, n: n > 1, edit)


def future_key_visible(case):
    """Row i < n-1 also sees key start+i+1 (it really is in the cache)."""
    def edit(m, start, n):
        i = torch.arange(n - 1)
        m[i, start + i + 1] = True
    return _masked(case, lambda start, n: n > 1, edit)


def drop_first_key_of_last_tile(case):
    """The first key of the sequence's last 64-key tile is lost (for the rows
    that would see it and have another key left)."""
    def edit(m, start, n):
        t0 = (start + n - 1) // 64 * 64
        i = torch.arange(n)
        m[i[start + i >= max(t0, 1)], t0] = False
    return _masked(case, lambda start, n: start + n > 1, edit)


def drop_tail_block(case):
    """The trailing partial KV block is lost."""
    BS = case["BS"]

    def edit(m, start, n):
        m[:, (start + n) // BS * BS:] = False
    return _masked(case, lambda start, n: (start + n) % BS != 0 and start + n > BS, edit)


def wrong_head_map(case):
    """q-head h reads kv-head ``h % KVH`` instead of ``h // rep``."""
    H, KVH = case["H"], case["KVH"]
    if all(h % KVH == h // (H // KVH) for h in range(H)):
        return None
    return oracle(case, head_map=lambda h: h % KVH)[0]


def table_of_sequence_0(case):
    """Every sequence reads sequence 0's block-table row."""
    if len(case["seqs"]) < 2:
        return None
    return oracle(case, bt=case["bt"][:1].expand_as(case["bt"]))[0]


def q_stride_ignored(case):
    qm = ko.misread_contiguous(case["q"])
    if torch.equal(qm, case["q"]):
        return None
    return oracle(case, q=qm)[0]


MUTANTS = {
    "own (diagonal) key dropped": drop_own_key,
    "prefix offset forgotten": prefix_offset_forgotten,
    "whole prefix invisible": prefix_invisible,
    "last prefix key dropped": drop_last_prefix_key,
    "first new key dropped for rows >= 1": drop_first_new_key,
    "one future key visible": future_key_visible,
    "first key of the last 64-key tile dropped": drop_first_key_of_last_tile,
    "trailing partial block dropped": drop_tail_block,
    "head map h % KVH": wrong_head_map,
    "every sequence reads sequence 0's table": table_of_sequence_0,
    "q token stride ignored": q_stride_ignored,
}
# the only mutant that no single-sequence case can hold
MULTI_ONLY = {"every sequence reads sequence 0's table"}
