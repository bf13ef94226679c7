"""The fused RoPE + KV-store kernel against the two kernels it replaces (bit for
bit: q, k, the V slice, both caches, both fp8 scale arrays) and against the
float64 oracles of ``kernel_oracles``; slots that were not written keep their
junk; rows that share one scratch slot (padded graph lanes) are harmless.

Run on an MI355X box: python -m pytest tests/test_gpu_rope_store.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import kernel_oracles as ko
import rope_store_cases as rs

DEV = "cuda:0"


def accept(kernel, case_name, out, e, mag, c, names):
    ratio, idx = ko.check(out, e, mag, c)
    msg = ko.describe(kernel, case_name, ratio, idx, names)
    print("RATIO " + msg)
    assert ratio <= 1.0, msg


def _device_state(c):
    d = lambda t: None if t is None else t.to(DEV).clone()
    return d(c["fused"]), d(c["kc"]), d(c["vc"]), d(c["ks"]), d(c["vs"])


def _bits(t):
    return t.view(torch.uint8) if t.dtype != torch.float32 else t.view(torch.int32)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("shape", rs.SHAPES, ids=rs.ids)
def test_fused_equals_two_kernels_and_oracles(shape, fp8):
    c = rs.build(*shape, fp8)
    H, KVH, D, BS = c["H"], c["KVH"], c["D"], c["BS"]
    pos, cs, slots = c["pos"].to(DEV), c["cs"].to(DEV), c["slots"].to(DEV)

    fa, kca, vca, ksa, vsa = _device_state(c)
    q, k, v = ko.qkv_views(fa, H, KVH, D)
    ops.rope_inplace(q, k, pos, cs)
    ops.store_kv(k, v, kca, vca, slots, ksa, vsa)

    fb, kcb, vcb, ksb, vsb = _device_state(c)
    q, k, v = ko.qkv_views(fb, H, KVH, D)
    assert c["T"] == 1 or not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    ops.rope_store_kv(q, k, v, pos, cs, kcb, vcb, slots, ksb, vsb)

    # identity with the two-kernel path: q, k and the V slice at once
    assert torch.equal(fa, fb), f"[{c['name']}] q/k/v buffer differs from rope_inplace"
    assert torch.equal(_bits(kca), _bits(kcb)), f"[{c['name']}] K cache differs from store_kv"
    assert torch.equal(_bits(vca), _bits(vcb)), f"[{c['name']}] V cache differs from store_kv"
    if fp8:
        assert torch.equal(_bits(ksa), _bits(ksb)) and torch.equal(_bits(vsa), _bits(vsb)), \
            f"[{c['name']}] fp8 scales differ from store_kv"

    # the float64 oracles
    q0, k0, v0 = ko.qkv_views(c["fused"], H, KVH, D)
    eq, tq = ko.rope(q0, c["pos"], c["cs"])
    ek, tk = ko.rope(k0, c["pos"], c["cs"])
    names = ("token", "head", "dim")
    accept("rope_store q", c["name"], q, eq, tq, ko.C_ELEM, names)
    accept("rope_store k", c["name"], k, ek, tk, ko.C_ELEM, names)
    assert torch.equal(v.cpu(), v0), "the V slice of the fused buffer changed"
    k_rot = k.cpu()
    if not fp8:
        want_k, want_v = ko.store_kv(k_rot, v0, c["kc"], c["vc"], c["slots"])
        # the whole cache: written slots hold the rows, all others their junk
        assert torch.equal(kcb.cpu(), want_k) and torch.equal(vcb.cpu(), want_v)
        return
    want = ko.store_kv_fp8(k_rot, v0, c["kc"], c["vc"], c["ks"], c["vs"], c["slots"])
    ko.check_store_fp8(kcb, vcb, ksb, vsb, want, f"rope_store_kv fp8 [{c['name']}]")
    NB = kcb.shape[0]
    untouched = torch.ones(NB * BS, dtype=torch.bool)
    untouched[c["slots"]] = False
    untouched = untouched.view(NB, 1, BS).expand(-1, KVH, -1)
    for got, before in ((kcb, c["kc"]), (vcb, c["vc"])):
        assert torch.equal(got.cpu().view(torch.uint8)[untouched],
                           before.view(torch.uint8)[untouched])
    for got, before in ((ksb, c["ks"]), (vsb, c["vs"])):
        assert torch.equal(got.cpu()[untouched], before[untouched])
    slot = int(c["slots"][c["zero"]])
    assert ksb[slot // BS, 0, slot % BS].item() == pytest.approx(1e-8, rel=1e-6)
    # a rotated zero is +0 or -0 (0 * c - 0 * s), so the sign bit may be set
    assert not (kcb[slot // BS, 0, slot % BS].view(torch.uint8) & 0x7F).any(), \
        "all-zero k row: codes must be zero"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_rows_sharing_one_scratch_slot(fp8):
    """Eight rows point at one scratch slot, as the padded lanes of a captured
    decode graph do: the run completes and every other slot is right."""
    c = rs.build(128, 4, 2, 50, 16, fp8)
    H, KVH, D, BS = c["H"], c["KVH"], c["D"], c["BS"]
    NB = c["kc"].shape[0]
    free = sorted(set(range(NB * BS)) - set(c["slots"].tolist()))
    scratch = free[0]
    slots_cpu = c["slots"].clone()
    slots_cpu[10:18] = scratch
    pos, cs, slots = c["pos"].to(DEV), c["cs"].to(DEV), slots_cpu.to(DEV)

    fa, kca, vca, ksa, vsa = _device_state(c)
    q, k, v = ko.qkv_views(fa, H, KVH, D)
    ops.rope_inplace(q, k, pos, cs)
    ops.store_kv(k, v, kca, vca, slots, ksa, vsa)

    fb, kcb, vcb, ksb, vsb = _device_state(c)
    q, k, v = ko.qkv_views(fb, H, KVH, D)
    ops.rope_store_kv(q, k, v, pos, cs, kcb, vcb, slots, ksb, vsb)
    torch.cuda.synchronize()

    assert torch.equal(fa, fb)
    others = torch.ones(NB * BS, dtype=torch.bool)
    others[scratch] = False
    others = others.view(NB, 1, BS).expand(-1, KVH, -1)
    for a, b in ((kca, kcb), (vca, vcb)):
        assert torch.equal(_bits(a.cpu())[others], _bits(b.cpu())[others])
    if fp8:
        for a, b in ((ksa, ksb), (vsa, vsb)):
            assert torch.equal(a.cpu()[others], b.cpu()[others])
    # and the rows written outside the scratch slot are the rotated rows
    if not fp8:
        keep = [t for t in range(c["T"]) if not 10 <= t < 18]
        want_k, want_v = ko.store_kv(k.cpu()[keep], v.cpu()[keep], c["kc"], c["vc"],
                                     slots_cpu[keep])
        assert torch.equal(kcb.cpu()[others], want_k[others])
        assert torch.equal(vcb.cpu()[others], want_v[others])
