"""Per-stream decode cases for the load-group edges of ``attn_decode_partial_t``
(not a test module itself; imported like ``kernel_oracles``).

The kernel gives each of a block's four waves a quarter of the chunk's keys
and keeps ``V_GROUP`` = 16 V rows in flight per wave; the score pass runs
64-key iterations with the next iteration's K rows prefetched. The context
lengths below put a chunk's key count on every edge of that scheme: waves
with no key (ctx 2, 3), one key per wave (4), fewer keys than a group, exactly
one group (64), one group plus one key (65), a clamped last group (95, 97,
129, ...), 64-key score iterations with and without a successor (63..65,
127..129, 191..193), and the same tails inside a second (261, 321), third
(545) and fourth (897) 256-key chunk. 4U - 1, 4U, 4U + 1 and 8U + 1 for
U = 16 are 63, 64, 65 and 129.

The cases are laid out like ``kernel_oracles.decode_case``: one row per
context length, disjoint random block tables two entries wider than any row
needs, q a strided view into a fused [B, (H + 2 KVH) D] buffer, every table
entry and cache slot past a row's context valid and filled with 100.0.
"""

import torch

import kernel_oracles as ko
from kernel_oracles import JUNK, _junk_tail, _quantise_fp8

V_GROUP = 16
CTX = [2, 3, 4, 5, 6, 7, 8, 9, 13, 31, 32, 33, 47, 63, 64, 65, 95, 96, 97, 127, 128, 129,
       191, 192, 193, 261, 321, 545, 897]
for _n in (4 * V_GROUP - 1, 4 * V_GROUP, 4 * V_GROUP + 1, 8 * V_GROUP + 1):
    assert _n in CTX, _n

KVH, D = ko.KVH, ko.D
SHAPES = [(1, 16), (2, 16), (4, 16), (8, 16), (4, 32)]     # (gqa, block size)

_cases = {}
_oracles = {}


def inflight_case(gqa, BS=16, fp8=False):
    key = (gqa, BS, fp8)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(7000 + 10 * gqa + BS)
    H = KVH * gqa
    B = len(CTX)
    need = [(c + BS - 1) // BS for c in CTX]
    n_junk = 8
    NB = sum(need) + n_junk
    max_blocks = max(need) + 2
    kc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
    vc = (torch.randn(NB, KVH, BS, D, generator=g) * 0.5).bfloat16()
    perm = torch.randperm(NB - n_junk, generator=g).tolist()
    junk = list(range(NB - n_junk, NB))
    kc[junk] = JUNK
    vc[junk] = JUNK
    bt = torch.tensor([[junk[(b + j) % n_junk] for j in range(max_blocks)] for b in range(B)],
                      dtype=torch.int32)
    it = iter(perm)
    for b in range(B):
        for j in range(need[b]):
            bt[b, j] = next(it)
        _junk_tail(kc, vc, int(bt[b, need[b] - 1]), CTX[b], BS)
    fused = (torch.randn(B, (H + 2 * KVH) * D, generator=g) * 4.0).bfloat16()
    q = fused[:, : H * D].view(B, H, D)
    case = {"name": f"inflight gqa={gqa} BS={BS}" + (" fp8" if fp8 else ""),
            "gqa": gqa, "fused": fused, "q": q, "kc": kc, "vc": vc, "bt": bt,
            "lens": torch.tensor(CTX, dtype=torch.int32), "scale": D ** -0.5, "c": ko.C_FP32}
    if fp8:
        # per-row scales of different sizes: the last key of the ctx=97 row
        # (the single key of a clamped group) and a key inside the fourth
        # chunk of the ctx=897 row are x4 rows
        def slot(b, k):
            return int(bt[b, k // BS]) * BS + k % BS

        def edit(k_rows, v_rows):
            for b, k in ((CTX.index(97), 96), (CTX.index(897), 800)):
                k_rows[slot(b, k)] *= 4.0
                v_rows[slot(b, k)] *= 4.0

        kc8, vc8, ks, vs = _quantise_fp8(kc, vc, edit)
        case.update(kc=kc8, vc=vc8, ks=ks, vs=vs)
    _cases[key] = case
    return case


def all_cases():
    return [inflight_case(gqa, BS, fp8) for fp8 in (False, True) for gqa, BS in SHAPES]


def oracle(case):
    """(e, A) of a case, computed once."""
    if case["name"] not in _oracles:
        _oracles[case["name"]] = ko.attn_decode(
            case["q"], case["kc"], case["vc"], case["bt"], case["lens"], case["scale"],
            case.get("ks"), case.get("vs"))
    return _oracles[case["name"]]


def read_one_key_past(case):
    """Every row attends to one key more than its context holds: the junk slot
    after its last key, or the first slot of the next (junk) table entry."""
    return ko._decode(dict(case, lens=case["lens"] + 1))


MUTANTS = {
    "last key dropped": ko.decode_drop_last_key,
    "one key past the context read": read_one_key_past,
    "tail partial block dropped": ko.decode_drop_tail_block,
    "q token stride ignored": ko.decode_stride_ignored,
}
