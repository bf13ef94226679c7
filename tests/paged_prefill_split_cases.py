"""Cases, plan walkers and defect "mutants" for the key-split mode of paged
prefill attention (not a test module itself; imported like
``paged_prefill_cases``, whose data, float64 oracle and bound it reuses).

A split plan (``ops.build_paged_prefill(key_splits=k)``) gives every q-tile
group of a split sequence one workgroup per contiguous key range; each writes
an unnormalised partial (O, m, l) per row and a reduce merges them. The CPU
emulation ``torch_ref.attn_prefill_paged_split`` walks exactly that plan, so
the properties and mutants here bite on a machine without a GPU.
"""

import copy

import torch

from kllms_amd import ops
from kllms_amd.ops import torch_ref

import paged_prefill_cases as pc

# (start, q_len) per sequence; each the smallest shape reaching its hazard
SPLIT_CASES = [
    [(64, 1)],          # the second split holds only the diagonal key
    [(16, 70)],         # rows 0..47 see nothing of the second split
    [(100, 33)],        # 3 rounds, one per split
    [(255, 65)],        # boundaries around the prefix edge
    [(256, 64)],
    [(257, 257)],       # two workgroups of q-tiles times splits
    [(512, 8)],         # idle waves
    [(1000, 40)],       # 17 rounds over 16 requested splits: uneven ranges
    pc.MULTI,           # mixed sequences
    [(0, 1), (600, 20), (64, 64)],   # split and unsplit sequences in one launch
]
MIXED = SPLIT_CASES[-1]
BS32_SPLIT_CASES = [[(16, 70)], [(100, 33)], [(257, 257)], MIXED]
KEY_SPLITS = (2, 3, 16)

# (H, KVH, BS, fp8, cases)
CONFIGS = [
    (8, 2, 16, False, SPLIT_CASES),
    (8, 2, 16, True, SPLIT_CASES),
    (4, 4, 16, False, SPLIT_CASES),
    (8, 2, 32, False, BS32_SPLIT_CASES),
]


def all_params():
    """(seqs, H, KVH, BS, fp8, key_splits) of every case x configuration x
    split count, with ids."""
    params, ids = [], []
    for H, KVH, BS, fp8, cases in CONFIGS:
        for seqs in cases:
            for k in KEY_SPLITS:
                params.append((seqs, H, KVH, BS, fp8, k))
                ids.append(f"{pc.case_id(seqs)}-H{H}KVH{KVH}-BS{BS}-"
                           f"{'fp8' if fp8 else 'bf16'}-k{k}")
    return params, ids


def plan(case, key_splits, device="cpu", **kw):
    return ops.build_paged_prefill(case["lens"], case["starts"], case["block_lists"], device,
                                   case["BS"], key_splits=key_splits, **kw)


def groups_of(meta):
    """[(sequence, first row of a q-tile, kbeg, kend, split index)] of every
    non-idle workgroup slot."""
    seqs, qpos = meta.grp_seq.tolist(), meta.grp_qpos0.tolist()
    kr, sp = meta.grp_krange.tolist(), meta.grp_split.tolist()
    return [(seqs[g], qpos[8 * g + w], kr[2 * g], kr[2 * g + 1], sp[g])
            for g in range(len(seqs)) for w in range(8) if qpos[8 * g + w] != -1]


# --- emulation of a correct kernel over a plan ------------------------------------

def partials(case, meta, **kw):
    return torch_ref.paged_prefill_split_partials(
        case["q"], case["kc"], case["vc"], meta, case["scale"], case.get("ks"), case.get("vs"),
        p_bf16=True, kv_bf16=True, **kw)


def emulate(case, meta):
    """bf16 probabilities into P.V, fp32 partials and merge."""
    return torch_ref.paged_prefill_split_merge(*partials(case, meta), meta)


def ratio_of(case, out):
    """Worst error / bound of ``out`` against the float64 oracle (dequantised
    fp8 K/V rounded to bf16, as the kernel and the emulation stage them)."""
    e, a = pc.case_oracle(case, round_kv_bf16=True)
    return pc.check(out, e, a, pc.C_MFMA)


# --- mutants: one defect in the plan or in the merge --------------------------------
# Each takes (case, meta) and returns the mutated output, or None when the
# plan holds nothing the defect would touch.

def _edited(meta, **fields):
    m = copy.copy(meta)
    for k, v in fields.items():
        setattr(m, k, v)
    return m


def _first_split_group(meta, want=lambda j, kb, ke: True):
    for g, j in enumerate(meta.grp_split.tolist()):
        kb, ke = meta.grp_krange[2 * g: 2 * g + 2].tolist()
        if j >= 0 and want(j, kb, ke):
            return g
    return None


def group_dropped(case, meta):
    """The workgroup of the first range of the first split q-tile group never
    runs (its slots keep the empty partial)."""
    g = _first_split_group(meta)
    if g is None:
        return None
    keep = [i for i in range(meta.n_groups) if i != g]
    m = _edited(meta, grp_seq=meta.grp_seq[keep], grp_split=meta.grp_split[keep],
                grp_qpos0=meta.grp_qpos0.view(-1, 8)[keep].reshape(-1),
                grp_krange=meta.grp_krange.view(-1, 2)[keep].reshape(-1))
    return torch_ref.paged_prefill_split_merge(*partials(case, m, empty_init=True), m)


def range_start_moved_up(case, meta):
    """Every range of split index 0 starts one round late."""
    kr = meta.grp_krange.clone().view(-1, 2)
    hit = meta.grp_split == 0
    if not bool(hit.any()):
        return None
    kr[hit, 0] += 64
    m = _edited(meta, grp_krange=kr.reshape(-1))
    return torch_ref.paged_prefill_split_merge(*partials(case, m), m)


def range_counted_twice(case, meta):
    """Every range of split index 1 starts at key 0: the first range is
    counted in two partials."""
    kr = meta.grp_krange.clone().view(-1, 2)
    hit = meta.grp_split == 1
    if not bool(hit.any()):
        return None
    kr[hit, 0] = 0
    m = _edited(meta, grp_krange=kr.reshape(-1))
    return torch_ref.paged_prefill_split_merge(*partials(case, m), m)


def _merge_with(case, meta, rule):
    """Merge by ``rule(m, l, o) -> (num [n, H, D], den [n, H])`` over the
    [n, k, H(, D)] partials of each split sequence."""
    out, pm, pl, po = partials(case, meta)
    cu = meta.cu_q.tolist()
    for s, (k, b) in enumerate(zip(meta.seq_nsplit.tolist(), meta.seq_ws_base.tolist())):
        n = cu[s + 1] - cu[s]
        if k < 2:
            continue
        H = po.shape[1]
        num, den = rule(pm[b: b + n * k].view(n, k, H), pl[b: b + n * k].view(n, k, H),
                        po[b: b + n * k].view(n, k, H, -1))
        out[cu[s]: cu[s + 1]] = torch.where(den[..., None] > 0, num / den[..., None].clamp_min(1e-38),
                                            torch.zeros_like(num))
    return out


def merge_ignores_m(case, meta):
    """Plain sum of O_j over sum of l_j."""
    return _merge_with(case, meta, lambda m, l, o: (o.sum(1), l.sum(1)))


def merge_takes_last_split(case, meta):
    return _merge_with(case, meta, lambda m, l, o: (o[:, -1], l[:, -1]))


def empty_partial_weighs_one(case, meta):
    """A merge without the ``l_j = 0 or m_j = -inf -> weight 0`` rule that
    takes exp(-inf - M) as 1: an empty partial enters the denominator as one
    key of weight 1."""
    def rule(m, l, o):
        empty = (l == 0) | (m == float("-inf"))
        if not bool(empty.any()):
            return None
        m_all = m.masked_fill(empty, float("-inf")).max(dim=1, keepdim=True).values
        w = torch.where(empty, torch.ones_like(m), torch.exp(m - m_all))
        l1 = torch.where(empty, torch.ones_like(l), l)
        return (w[..., None] * o).sum(1), (w * l1).sum(1)

    touched = []

    def counting(m, l, o):
        r = rule(m, l, o)
        if r is None:
            return merge_rule_reference(m, l, o)
        touched.append(1)
        return r

    out = _merge_with(case, meta, counting)
    return out if touched else None


def merge_rule_reference(m, l, o):
    empty = (l == 0) | (m == float("-inf"))
    m_all = m.masked_fill(empty, float("-inf")).max(dim=1, keepdim=True).values
    w = torch.where(empty, torch.zeros_like(m), torch.exp(m - m_all))
    return (w[..., None] * o).sum(1), (w * l).sum(1)


# name -> (mutant, a case that holds it, key_splits)
MUTANTS = {
    "one group dropped": (group_dropped, [(256, 64)], 2),
    "a range's start moved up by 64": (range_start_moved_up, [(255, 65)], 3),
    "a range counted twice": (range_counted_twice, [(100, 33)], 3),
    "merge ignores m_j": (merge_ignores_m, [(1000, 40)], 16),
    "merge takes only the last split": (merge_takes_last_split, [(512, 8)], 2),
    "empty partials given weight 1": (empty_partial_weighs_one, [(16, 70)], 2),
}
