"""Tests of the kernel tests (CPU): the float64 oracles and derived bounds of
``kernel_oracles`` must ACCEPT honest arithmetic (``ops/torch_ref.py`` in
fp32 rounded to bf16, and an emulation of the MFMA kernels that rounds the
probabilities to bf16) and REJECT every classic kernel defect, on the very
cases ``test_gpu_kernel_edges.py`` runs on the GPU.
"""

import pytest
import torch

import kernel_oracles as ko
from kllms_amd.ops import torch_ref

GQAS = [1, 2, 4, 8]


def decode_cases():
    out = []
    for fp8 in (False, True):
        out += [ko.decode_case(g, 16, fp8) for g in GQAS] + [ko.decode_case(4, 32, fp8)]
    out += [ko.cascade_case(g) for g in GQAS] + [ko.cascade_case(4, fp8=True)]
    return out


def prefill_cases():
    return [ko.prefill_case(s, H, KVH) for s in ko.PREFILL_SEQLENS for H, KVH in ko.PREFILL_HEADS]


def as_kernel_output(x64):
    """What a kernel that computed ``x64`` would store."""
    return x64.float().bfloat16()


# --- honest arithmetic is accepted ------------------------------------------------

def test_torch_ref_decode_accepted():
    worst = 0.0
    for case in decode_cases():
        if "round_kv" in case:
            # torch_ref dequantises in fp32 without the bf16 rounding step
            e, a = ko.attn_decode(case["q"], case["kc"], case["vc"], case["bt"], case["lens"],
                                  case["scale"], case["ks"], case["vs"])
        else:
            e, a = ko.decode_oracle(case)
        out = torch_ref.attn_decode_paged(case["q"], case["kc"], case["vc"], case["bt"],
                                          case["lens"], case["scale"],
                                          case.get("ks"), case.get("vs"))
        ratio, idx = ko.check(out, e, a, case["c"])
        assert ratio <= 1.0, ko.describe("torch_ref decode", case["name"], ratio, idx,
                                         ("row", "head", "dim"))
        worst = max(worst, ratio)
        if "tiles" in case:
            out = torch_ref.attn_decode_paged_shared(
                case["q"], case["kc"], case["vc"], case["bt"], case["lens"], case["scale"],
                case.get("ks"), case.get("vs"), shared=case["tiles"].to_tensors("cpu"))
            ratio, idx = ko.check(out, e, a, case["c"])
            assert ratio <= 1.0, ko.describe("torch_ref cascade", case["name"], ratio, idx,
                                             ("row", "head", "dim"))
            worst = max(worst, ratio)
    print(f"torch_ref decode worst ratio {worst:.3f}")


def test_torch_ref_prefill_accepted():
    worst = 0.0
    for case in prefill_cases():
        e, a = ko.prefill_oracle(case)
        out = torch_ref.attn_prefill_varlen(case["q"], case["k"], case["v"], case["cu"],
                                            case["scale"])
        ratio, idx = ko.check(out, e, a, case["c"])
        assert ratio <= 1.0, ko.describe("torch_ref prefill", case["name"], ratio, idx,
                                         ("token", "head", "dim"))
        worst = max(worst, ratio)
    print(f"torch_ref prefill worst ratio {worst:.3f}")


def test_bf16_probability_emulation_accepted():
    """exp(s - m) rounded to bf16 into the PV product, fp32 normaliser: the
    arithmetic of the MFMA kernels sits inside c = 2^-8."""
    worst = 0.0
    for case in decode_cases():
        e, a = ko.decode_oracle(case)
        emu, _ = ko.attn_decode(case["q"], case["kc"], case["vc"], case["bt"], case["lens"],
                                case["scale"], case.get("ks"), case.get("vs"),
                                round_kv_bf16=case.get("round_kv", False), p_bf16=True)
        ratio, idx = ko.check(as_kernel_output(emu), e, a, ko.C_MFMA)
        assert ratio <= 1.0, ko.describe("bf16-P decode", case["name"], ratio, idx,
                                         ("row", "head", "dim"))
        worst = max(worst, ratio)
    for case in prefill_cases():
        e, a = ko.prefill_oracle(case)
        emu, _ = ko.attn_prefill(case["q"], case["k"], case["v"], case["cu"], case["scale"],
                                 p_bf16=True)
        ratio, idx = ko.check(as_kernel_output(emu), e, a, ko.C_MFMA)
        assert ratio <= 1.0, ko.describe("bf16-P prefill", case["name"], ratio, idx,
                                         ("token", "head", "dim"))
        worst = max(worst, ratio)
    print(f"bf16-P emulation worst ratio {worst:.3f}")


def test_oracle_is_a_softmax_average():
    """Sanity of the oracle itself: with V = 1 everywhere the output is 1 and
    A = 1; a row with one key returns that key's V."""
    case = ko.decode_case(2)
    ones = torch.ones_like(case["vc"])
    e, a = ko.attn_decode(case["q"], case["kc"], ones, case["bt"], case["lens"], case["scale"])
    assert torch.allclose(e, torch.ones_like(e), atol=1e-12)
    assert torch.allclose(a, torch.ones_like(a), atol=1e-12)
    e, _ = ko.decode_oracle(case)
    blk = int(case["bt"][0, 0])
    want = ko.f64(case["vc"][blk, :, 0, :]).repeat_interleave(2, dim=0)
    assert torch.equal(e[0], want)
    pc = ko.prefill_case([33], 8, 2)
    e, _ = ko.prefill_oracle(pc)
    assert torch.equal(e[0], ko.f64(pc["v"][0]).repeat_interleave(4, dim=0))


def test_check_zero_bound():
    z = torch.zeros(2, 3, dtype=torch.float64)
    assert ko.check(torch.zeros(2, 3), z, z, ko.C_ELEM)[0] == 0.0
    bad = torch.zeros(2, 3)
    bad[1, 2] = 1e-30
    ratio, idx = ko.check(bad, z, z, ko.C_ELEM)
    assert ratio == float("inf") and idx == (1, 2)
    nan = torch.full((2, 3), float("nan"))
    assert ko.check(nan, z + 1, z + 1, ko.C_ELEM)[0] == float("inf")


# --- every defect is rejected -----------------------------------------------------

def _mutant_sweep(mutants, name, cases, oracle):
    applied = 0
    weakest = float("inf")
    for case in cases:
        out = mutants[name](case)
        if out is None:
            continue
        e, a = oracle(case)
        if torch.equal(out, e):
            continue           # the defect touched no key of this case
        applied += 1
        ratio, _ = ko.check(as_kernel_output(out), e, a, case["c"])
        assert ratio > 1.0, f"mutant '{name}' passes on {case['name']}: ratio {ratio:.3f}"
        weakest = min(weakest, ratio)
    assert applied > 0, f"mutant '{name}' applied to no case"
    print(f"mutant '{name}': {applied} cases, weakest ratio {weakest:.2f}")


@pytest.mark.parametrize("name", list(ko.DECODE_MUTANTS))
def test_decode_mutant_rejected(name):
    _mutant_sweep(ko.DECODE_MUTANTS, name, decode_cases(), ko.decode_oracle)


@pytest.mark.parametrize("name", list(ko.PREFILL_MUTANTS))
def test_prefill_mutant_rejected(name):
    _mutant_sweep(ko.PREFILL_MUTANTS, name, prefill_cases(), ko.prefill_oracle)


def test_mutants_apply_where_they_should():
    """No mutant hides behind 'does not apply': on the per-stream batch every
    decode mutant has a key to touch, on the 289-token prefill every prefill
    mutant has."""
    case = ko.decode_case(4)
    for name, fn in ko.DECODE_MUTANTS.items():
        assert fn(case) is not None, name
    case = ko.prefill_case([289], 8, 2)
    for name, fn in ko.PREFILL_MUTANTS.items():
        assert fn(case) is not None, name


# --- elementwise: torch_ref accepted, ignored strides rejected --------------------

@pytest.mark.parametrize("rows,n", ko.RMSNORM_SHAPES)
def test_torch_ref_rmsnorm_accepted(rows, n):
    c = ko.rmsnorm_case(rows, n)
    e, t = ko.rmsnorm(c["x"], c["w"], ko.EPS)
    ratio, idx = ko.check(torch_ref.rmsnorm(c["x"], c["w"], ko.EPS), e, t, ko.C_ELEM)
    assert ratio <= 1.0, ko.describe("torch_ref rmsnorm", c["name"], ratio, idx, ("row", "col"))
    res, e, t = ko.fused_add_rmsnorm(c["xr"], c["r"], c["w"], ko.EPS)
    out, got_res = torch_ref.fused_add_rmsnorm(c["xr"], c["r"].clone(), c["w"], ko.EPS)
    assert torch.equal(got_res, res)
    ratio, idx = ko.check(out, e, t, ko.C_ELEM)
    assert ratio <= 1.0, ko.describe("torch_ref fused_add_rmsnorm", c["name"], ratio, idx,
                                     ("row", "col"))
    if c["zero_row"] is not None:
        assert not e[c["zero_row"]].any() and not f64_any(res[c["zero_row"]])
    # normalising by the weight-less rms only (w dropped) is outside the bound
    e, t = ko.rmsnorm(c["x"], c["w"], ko.EPS)
    bad, _ = ko.rmsnorm(c["x"], torch.ones_like(c["w"]), ko.EPS)
    assert ko.check(as_kernel_output(bad), e, t, ko.C_ELEM)[0] > 1.0


def f64_any(t):
    return bool(ko.f64(t).any())


@pytest.mark.parametrize("Dh,H,KVH,T", ko.ROPE_SHAPES)
def test_torch_ref_rope_accepted(Dh, H, KVH, T):
    c = ko.rope_case(Dh, H, KVH, T)
    q, k, _ = ko.qkv_views(c["fused"], H, KVH, Dh)
    eq, tq = ko.rope(q, c["pos"], c["cs"])
    ek, tk = ko.rope(k, c["pos"], c["cs"])
    buf = c["fused"].clone()
    q2, k2, v2 = ko.qkv_views(buf, H, KVH, Dh)
    torch_ref.rope_inplace(q2, k2, c["pos"], c["cs"])
    for nm, got, e, t in (("q", q2, eq, tq), ("k", k2, ek, tk)):
        ratio, idx = ko.check(got, e, t, ko.C_ELEM)
        assert ratio <= 1.0, ko.describe(f"torch_ref rope {nm}", c["name"], ratio, idx,
                                         ("token", "head", "dim"))
    assert torch.equal(v2, ko.qkv_views(c["fused"], H, KVH, Dh)[2])
    # ignoring the token stride, or the interleaved pair layout, is rejected
    if T > 1:
        for view, e, t in ((q, eq, tq), (k, ek, tk)):
            bad, _ = ko.rope(ko.misread_contiguous(view), c["pos"], c["cs"])
            assert ko.check(as_kernel_output(bad), e, t, ko.C_ELEM)[0] > 1.0
    x = ko.f64(q)
    cs = ko.f64(c["cs"])[c["pos"]]
    cos, sin = cs[:, None, : Dh // 2], cs[:, None, Dh // 2:]
    inter = torch.empty_like(x)
    inter[..., 0::2] = x[..., 0::2] * cos - x[..., 1::2] * sin
    inter[..., 1::2] = x[..., 1::2] * cos + x[..., 0::2] * sin
    assert ko.check(as_kernel_output(inter), eq, tq, ko.C_ELEM)[0] > 1.0


@pytest.mark.parametrize("T,I", ko.SILU_SHAPES)
def test_torch_ref_silu_mul_accepted(T, I):
    c = ko.silu_case(T, I)
    e, t = ko.silu_mul(c["gate"], c["up"])
    ratio, idx = ko.check(torch_ref.silu_mul(c["gate"], c["up"]), e, t, ko.C_ELEM)
    assert ratio <= 1.0, ko.describe("torch_ref silu_mul", c["name"], ratio, idx, ("row", "col"))
    if T > 1:
        for swap in ("gate", "up"):
            args = dict(gate=c["gate"], up=c["up"])
            args[swap] = ko.misread_contiguous(c[swap])
            bad, _ = ko.silu_mul(**args)
            assert ko.check(as_kernel_output(bad), e, t, ko.C_ELEM)[0] > 1.0, swap


@pytest.mark.parametrize("Dh,BS,T", ko.STORE_SHAPES)
def test_torch_ref_store_kv_accepted(Dh, BS, T):
    c = ko.store_case(Dh, BS, T)
    wk, wv = ko.store_kv(c["k"], c["v"], c["kc"], c["vc"], c["slots"])
    kc, vc = c["kc"].clone(), c["vc"].clone()
    torch_ref.store_kv(c["k"], c["v"], kc, vc, c["slots"])
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    touched = (wk != c["kc"]).any(-1).sum().item()
    assert touched == T * c["KVH"]                      # the pattern never equals a stored row
    if T > 1:
        bk, bv = ko.store_kv(ko.misread_contiguous(c["k"]), ko.misread_contiguous(c["v"]),
                             c["kc"], c["vc"], c["slots"])
        assert not torch.equal(bk, wk) and not torch.equal(bv, wv)


@pytest.mark.parametrize("Dh", [64, 128])
def test_torch_ref_store_kv_fp8_accepted(Dh):
    c = ko.store_case(Dh, 16, 50, fp8=True, zero_row=True)
    want = ko.store_kv_fp8(c["k"], c["v"], c["kc"], c["vc"], c["ks"], c["vs"], c["slots"])
    kc, vc, ks, vs = c["kc"].clone(), c["vc"].clone(), c["ks"].clone(), c["vs"].clone()
    torch_ref.store_kv(c["k"], c["v"], kc, vc, c["slots"], ks, vs)
    ko.check_store_fp8(kc, vc, ks, vs, want, c["name"])
    slot = int(c["slots"][c["zero"]])
    assert want[2][slot // 16, 0, slot % 16].item() == pytest.approx(1e-8, rel=1e-6)
    assert not want[0][slot // 16, 0, slot % 16].float().any()
    bad = ko.store_kv_fp8(ko.misread_contiguous(c["k"]), ko.misread_contiguous(c["v"]),
                          c["kc"], c["vc"], c["ks"], c["vs"], c["slots"])
    with pytest.raises(AssertionError):
        ko.check_store_fp8(kc, vc, ks, vs, bad, c["name"])
