"""HIP kernels against float64 oracles at tile, chunk and stride edges.

Every kernel output is held to the derived bound of ``kernel_oracles``
(``|a - e| <= 2^-7 |e| + c * M``, see that module's docstring): tight enough
that a lost key, an off-by-one context length, a wrong block, a bad tail tile
or an ignored stride argument fails (``test_kernel_oracles.py`` proves that on
the CPU with the same cases). Inputs are always valid: table entries and cache
slots past a row's context point at real blocks filled with the constant
100.0, so a read past the context shows in the numbers and no index leaves
the cache.

Run on an MI355X box: python -m pytest tests/test_gpu_kernel_edges.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import kernel_oracles as ko

DEV = "cuda:0"

_dev = {}


def on_dev(case, *names):
    """Device copies of a case's tensors, made once per case."""
    key = case["name"]
    if key not in _dev:
        _dev[key] = {k: v.to(DEV) for k, v in case.items() if isinstance(v, torch.Tensor)}
    d = _dev[key]
    return [d.get(n) for n in names]


def accept(kernel, case_name, out, e, mag, c, names, extra=lambda idx: ""):
    ratio, idx = ko.check(out, e, mag, c)
    msg = ko.describe(kernel, case_name, ratio, idx, names, extra(idx))
    print("RATIO " + msg)
    assert ratio <= 1.0, msg


# --- decode attention -------------------------------------------------------------

def _decode_q(case, fused):
    B, H, D = case["q"].shape
    q = fused[:, : H * D].view(B, H, D)
    assert q.stride(0) == fused.shape[1] and not q.is_contiguous()
    return q


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("gqa,BS", [(1, 16), (2, 16), (4, 16), (8, 16), (4, 32)])
def test_decode_per_stream(gqa, BS, fp8):
    case = ko.decode_case(gqa, BS, fp8)
    e, a = ko.decode_oracle(case)
    fused, kc, vc, bt, lens, ks, vs = on_dev(case, "fused", "kc", "vc", "bt", "lens", "ks", "vs")
    assert bt.shape[1] == max((c + BS - 1) // BS for c in ko.DECODE_CTX) + 2
    out = ops.attn_decode_paged(_decode_q(case, fused), kc, vc, bt, lens, case["scale"], ks, vs)
    accept("attn_decode", case["name"], out, e, a, ko.C_FP32, ("row", "head", "dim"),
           lambda idx: f", ctx={ko.DECODE_CTX[idx[0]]}")


@pytest.mark.parametrize("gqa,fp8", [(1, False), (2, False), (4, False), (8, False), (4, True)])
def test_decode_cascade(gqa, fp8):
    case = ko.cascade_case(gqa, fp8)
    e, a = ko.decode_oracle(case)
    fused, kc, vc, bt, lens, ks, vs = on_dev(case, "fused", "kc", "vc", "bt", "lens", "ks", "vs")
    tiles = case["tiles"]
    assert tiles.n_tiles == (4 if gqa == 8 else 2)
    out = ops.attn_decode_paged(_decode_q(case, fused), kc, vc, bt, lens, case["scale"], ks, vs,
                                shared=tiles.to_tensors(DEV))
    ctx = case["lens"].tolist()
    accept("attn_decode_shared", case["name"], out, e, a, ko.C_MFMA, ("row", "head", "dim"),
           lambda idx: f", ctx={ctx[idx[0]]}, skip_chunks={tiles.skip[idx[0]]}")


# --- prefill attention ------------------------------------------------------------

@pytest.mark.parametrize("H,KVH", ko.PREFILL_HEADS)
@pytest.mark.parametrize("seqlens", ko.PREFILL_SEQLENS, ids=lambda s: "-".join(map(str, s)))
def test_prefill(seqlens, H, KVH):
    case = ko.prefill_case(seqlens, H, KVH)
    e, a = ko.prefill_oracle(case)
    fused, cu = on_dev(case, "fused", "cu")
    q, k, v = ko.qkv_views(fused, H, KVH, ko.D)
    assert not q.is_contiguous() or len(fused) == 1
    out = ops.attn_prefill_varlen(q, k, v, cu, case["scale"])

    def where(idx):
        s, pos = ko.query_pos(case, idx[0])
        return f", sequence={s} (len {seqlens[s]}), query position={pos}"

    accept("attn_prefill", case["name"], out, e, a, ko.C_MFMA, ("token", "head", "dim"), where)


# --- elementwise ------------------------------------------------------------------

@pytest.mark.parametrize("rows,n", ko.RMSNORM_SHAPES)
def test_rmsnorm(rows, n):
    c = ko.rmsnorm_case(rows, n)
    x, xr, r, w = on_dev(c, "x", "xr", "r", "w")
    e, t = ko.rmsnorm(c["x"], c["w"], ko.EPS)
    out = ops.rmsnorm(x, w, ko.EPS)
    accept("rmsnorm", c["name"], out, e, t, ko.C_ELEM, ("row", "col"))
    if c["zero_row"] is not None:
        assert not out[c["zero_row"]].float().any(), "all-zero row must give exactly 0"

    want_res, e, t = ko.fused_add_rmsnorm(c["xr"], c["r"], c["w"], ko.EPS)
    res = r.clone()
    out, res2 = ops.fused_add_rmsnorm(xr, res, w, ko.EPS)
    assert res2 is res
    assert torch.equal(res.cpu(), want_res), f"fused residual not bit-equal [{c['name']}]"
    accept("fused_add_rmsnorm", c["name"], out, e, t, ko.C_ELEM, ("row", "col"))
    if c["zero_row"] is not None:
        assert not out[c["zero_row"]].float().any() and not res[c["zero_row"]].float().any()


@pytest.mark.parametrize("Dh,H,KVH,T", ko.ROPE_SHAPES)
def test_rope(Dh, H, KVH, T):
    c = ko.rope_case(Dh, H, KVH, T)
    pos = c["pos"].tolist()
    assert ko.ROPE_MAX_POS - 1 in pos and (T == 1 or 0 in pos)
    q0, k0, v0 = ko.qkv_views(c["fused"], H, KVH, Dh)
    eq, tq = ko.rope(q0, c["pos"], c["cs"])
    ek, tk = ko.rope(k0, c["pos"], c["cs"])
    fused, posd, cs = on_dev(c, "fused", "pos", "cs")
    buf = fused.clone()
    q, k, v = ko.qkv_views(buf, H, KVH, Dh)
    ops.rope_inplace(q, k, posd, cs)
    names = ("token", "head", "dim")
    accept("rope q", c["name"], q, eq, tq, ko.C_ELEM, names, lambda i: f", position={pos[i[0]]}")
    accept("rope k", c["name"], k, ek, tk, ko.C_ELEM, names, lambda i: f", position={pos[i[0]]}")
    assert torch.equal(v.cpu(), v0), "rope touched the V slice of the fused buffer"


def _silu(c):
    e, t = ko.silu_mul(c["gate"], c["up"])
    if c["buf"] is not None:
        (buf,) = on_dev(c, "buf")
        I = c["gate"].shape[1]
        gate, up = buf[:, :I], buf[:, I:]
        assert gate.stride(0) == 2 * I
    else:
        gate, up = on_dev(c, "gate", "up")
    out = ops.silu_mul(gate, up)
    assert out.is_contiguous()
    accept("silu_mul", c["name"], out, e, t, ko.C_ELEM, ("row", "col"))


@pytest.mark.parametrize("T,I", ko.SILU_SHAPES)
def test_silu_mul_fused_halves(T, I):
    _silu(ko.silu_case(T, I))


def test_silu_mul_wraps_grid_cap():
    # 1025 * 4096 / 8 vectors > 2048 blocks * 256 threads
    _silu(ko.silu_case(1025, 4096, fused=False))


def _store_bf16(c):
    want_k, want_v = ko.store_kv(c["k"], c["v"], c["kc"], c["vc"], c["slots"])
    fused, kc, vc, slots = on_dev(c, "fused", "kc", "vc", "slots")
    kc, vc = kc.clone(), vc.clone()
    _, k, v = ko.qkv_views(fused, c["H"], c["KVH"], c["D"])
    ops.store_kv(k, v, kc, vc, slots)
    for nm, got, want in (("K", kc, want_k), ("V", vc, want_v)):
        got = got.cpu()
        if not torch.equal(got, want):
            bad = (got != want).any(-1).nonzero()[0].tolist()
            raise AssertionError(f"store_kv [{c['name']}]: {nm} cache differs first at "
                                 f"(block, kv_head, offset)={bad}")


@pytest.mark.parametrize("Dh,BS,T", ko.STORE_SHAPES)
def test_store_kv(Dh, BS, T):
    _store_bf16(ko.store_case(Dh, BS, T))


def test_store_kv_wraps_grid_cap():
    # 4097 * 8 * 16 vectors > 2048 blocks * 256 threads
    _store_bf16(ko.store_case(128, 16, 4097, KVH_=8))


def _store_fp8(c):
    want = ko.store_kv_fp8(c["k"], c["v"], c["kc"], c["vc"], c["ks"], c["vs"], c["slots"])
    fused, kc, vc, ks, vs, slots = on_dev(c, "fused", "kc", "vc", "ks", "vs", "slots")
    kc, vc, ks, vs = kc.clone(), vc.clone(), ks.clone(), vs.clone()
    _, k, v = ko.qkv_views(fused, c["H"], c["KVH"], c["D"])
    ops.store_kv(k, v, kc, vc, slots, ks, vs)
    ko.check_store_fp8(kc, vc, ks, vs, want, f"store_kv fp8 [{c['name']}]")
    # untouched slots keep their codes and scales bit for bit
    BS = kc.shape[2]
    untouched = torch.ones(kc.shape[0] * BS, dtype=torch.bool)
    untouched[c["slots"]] = False
    untouched = untouched.view(kc.shape[0], 1, BS).expand(-1, kc.shape[1], -1)
    for got, before in ((kc, c["kc"]), (vc, c["vc"])):
        assert torch.equal(got.cpu().view(torch.uint8)[untouched],
                           before.view(torch.uint8)[untouched])
    for got, before in ((ks, c["ks"]), (vs, c["vs"])):
        assert torch.equal(got.cpu()[untouched], before[untouched])
    return kc.cpu(), ks.cpu()


@pytest.mark.parametrize("Dh", [64, 128])
def test_store_kv_fp8(Dh):
    c = ko.store_case(Dh, 16, 50, fp8=True, zero_row=True)
    kc, ks = _store_fp8(c)
    slot = int(c["slots"][c["zero"]])
    assert ks[slot // 16, 0, slot % 16].item() == pytest.approx(1e-8, rel=1e-6)
    assert not kc[slot // 16, 0, slot % 16].view(torch.uint8).any(), "all-zero row: codes must be 0"


def test_store_kv_fp8_wraps_grid_cap():
    # 4100 * 2 rows > 2048 blocks * 4 rows
    _store_fp8(ko.store_case(128, 16, 4100, KVH_=2, fp8=True))


# --- sampler logprob --------------------------------------------------------------

@pytest.mark.parametrize("V", [1000, 32003])
def test_sampler_logprob(V):
    B = 6
    W = (V + 31) // 32
    g = torch.Generator().manual_seed(9000 + V)
    logits = torch.randn(B, V, generator=g) * 3.0
    temps = torch.tensor([0.0, 0.7, 1.3, 0.7, 0.0, 1.3])
    top_k = torch.tensor([0, 5, 0, 5, 0, 0], dtype=torch.int32)
    top_p = torch.tensor([1.0, 1.0, 0.7, 0.7, 1.0, 1.0])
    allowed = torch.ones(B, V, dtype=torch.bool)
    single = V - 3                                    # in the partial last mask word
    for b in (1, 4):
        allowed[b] = torch.rand(V, generator=g) < 0.5
    allowed[3] = False
    allowed[3, single] = True
    bits = torch.zeros(B, W * 32, dtype=torch.int64)
    bits[:, :V] = allowed.to(torch.int64)
    words = (bits.view(B, W, 32) << torch.arange(32)).sum(-1)
    mask = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    masked = torch.where(allowed, logits.to(torch.float64),
                         torch.full((B, V), float("-inf"), dtype=torch.float64))
    want_lp = torch.log_softmax(masked, dim=-1)

    seeds = torch.arange(B, dtype=torch.int64) + 21
    for step in range(3):
        steps = torch.full((B,), step, dtype=torch.int64)
        toks, lps = ops.sample(logits.to(DEV), temps.to(DEV), top_p.to(DEV), top_k.to(DEV),
                               seeds.to(DEV), steps.to(DEV), mask.to(DEV))
        toks, lps = toks.cpu(), lps.cpu()
        for b in range(B):
            tok = int(toks[b])
            where = f"V={V} step={step} row={b} token={tok}"
            assert 0 <= tok < V and allowed[b, tok], f"sampler chose a disallowed token: {where}"
            err = abs(lps[b].item() - want_lp[b, tok].item())
            assert err <= 1e-3, (f"sampler logprob off by {err:.3e}: {where}, got "
                                 f"{lps[b].item():.6f}, want {want_lp[b, tok].item():.6f}")
        assert int(toks[3]) == single and abs(lps[3].item()) <= 1e-3
        for b in (0, 4):
            assert int(toks[b]) == int(masked[b].argmax()), f"greedy row {b} is not the argmax"
