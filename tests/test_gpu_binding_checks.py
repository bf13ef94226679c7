"""The host argument checks of the ``_C`` bindings (``bindings.hip``): for each
binding one accepted call at the smallest shape its kernel takes, the same call
with zero rows, and one refused call per argument property the binding has to
hold before it hands raw pointers to a kernel.

Run on an MI355X box: python -m pytest tests/test_gpu_binding_checks.py -m gpu -q

Every refusal case here is harmless even if the check it tests were missing
and the kernel launched:
  - a wrong length is one element (row, block) too LONG, never short;
  - a wrong rank or stride is a view that keeps the full storage, so whatever
    layout the kernel assumed stays inside the allocation;
  - a wrong dtype is the same width or wider;
  - a wrong-device (CPU tensor) case is built on the zero-row form of the
    call, which returns before any launch.
Index values (slots, block ids, positions, pair indices) are always valid.

A refused call raises ``RuntimeError`` and, after a synchronise, every output
buffer still holds what it held before (pure outputs hold a sentinel).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops
from kllms_amd.ops import torch_ref

DEV = "cuda:0"
C = ops._hip_or_raise()
SENTINEL = -777.0
T, H, KVH, D, BS, NB = 3, 2, 1, 128, 16, 4
B, V = 2, 1000
W = (V + 31) // 32
N = 64            # hidden size of the norm / activation cases
MAX_POS = 32
FP8 = torch.float8_e4m3fn


def bf16(*shape):
    return torch.randn(*shape, device=DEV).bfloat16()


def sentinel(*shape, dtype=torch.bfloat16):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


def no_scale():
    return torch.empty(0, dtype=torch.float32, device=DEV)


def strided(t):
    """The same values as every second element of a buffer twice as long."""
    wide = torch.zeros(t.numel() * 2, dtype=t.dtype, device=t.device)
    wide[::2] = t.reshape(-1)
    return wide[::2].view(t.shape) if t.dim() == 1 else wide.view(*t.shape, 2)[..., 0]


def longer(t, dim=0):
    """One more entry along ``dim``, a copy of the last one."""
    if t.dtype == FP8:
        return longer(t.view(torch.uint8), dim).view(FP8)
    return torch.cat([t, t.narrow(dim, t.size(dim) - 1, 1)], dim).contiguous()


def offset_rows(t, elems=4):
    """The same row view moved ``elems`` elements (8 bytes) off its 16-byte
    alignment inside a wider buffer; the token stride stays a multiple of 8."""
    rows, width = t.size(0), t[0].numel()
    wide = torch.zeros(rows, width + 8, dtype=t.dtype, device=t.device)
    view = wide[:, elems:elems + width].view(t.shape)
    view.copy_(t)
    return view


def qkv(fused, h=H, kvh=KVH, d=D):
    """The strided q / k / v views of a fused-QKV projection output."""
    t = fused.shape[0]
    return (fused[:, :h * d].view(t, h, d), fused[:, h * d:(h + kvh) * d].view(t, kvh, d),
            fused[:, (h + kvh) * d:].view(t, kvh, d))


def caches(fp8):
    """Both caches, junk-filled, and the scale arrays (empty for bf16)."""
    kc = bf16(NB, KVH, BS, D)
    vc = bf16(NB, KVH, BS, D)
    if not fp8:
        return kc, vc, no_scale(), no_scale()
    return (kc.to(FP8), vc.to(FP8), torch.rand(NB, KVH, BS, device=DEV) + 0.5,
            torch.rand(NB, KVH, BS, device=DEV) + 0.5)


class Binding:
    """args(): a fresh dict of valid arguments; call(a); outs: the keys of the
    buffers the call may write; zero: edits that make it the zero-row call;
    refusals: name -> edits; cpu: keys refused as CPU tensors (zero-row form)."""

    def __init__(self, args, call, outs, zero, refusals, cpu):
        self.args, self.call, self.outs, self.zero = args, call, outs, zero
        self.refusals, self.cpu = refusals, cpu


def edit(a, edits):
    for key, fn in edits.items():
        a[key] = fn(a)


def bits(t):
    return t.contiguous().view(torch.uint8)


def run_unchanged(binding, a, edits, raises):
    """Apply ``edits`` and call; the output buffers of before and after the
    edits all keep their bits."""
    watched = [a[k] for k in binding.outs]
    edit(a, edits)
    watched += [a[k] for k in binding.outs]
    before = [bits(t).clone() for t in watched]
    if raises:
        with pytest.raises(RuntimeError):
            binding.call(a)
    else:
        binding.call(a)
    torch.cuda.synchronize()
    for t, b in zip(watched, before):
        assert torch.equal(bits(t), b), "an output buffer was written"


# --- rmsnorm / fused_add_rmsnorm / silu_mul -------------------------------------------

def _norm_args():
    return {"out": sentinel(T, N), "x": bf16(T, N), "res": bf16(T, N), "w": bf16(N)}


_norm_zero = {"out": lambda a: a["out"][:0], "x": lambda a: a["x"][:0], "res": lambda a: a["res"][:0]}
_norm_refusals = {
    "out one row longer than x": {"out": lambda a: sentinel(T + 1, N)},
    "out 1-D": {"out": lambda a: a["out"].view(-1)},
    "weight one vector longer than the row": {"w": lambda a: bf16(N + 8)},
    "weight not contiguous": {"w": lambda a: strided(a["w"])},
    "x fp32": {"x": lambda a: a["x"].float()},
}

RMSNORM = Binding(
    _norm_args, lambda a: C.rmsnorm(a["out"], a["x"], a["w"], 1e-5), ("out",), _norm_zero,
    _norm_refusals, ("x", "w"))

FUSED_ADD_RMSNORM = Binding(
    _norm_args, lambda a: C.fused_add_rmsnorm(a["out"], a["x"], a["res"], a["w"], 1e-5),
    ("out", "res"), _norm_zero,
    dict(_norm_refusals, **{
        "residual one row longer than x": {"res": lambda a: bf16(T + 1, N)},
        "residual not contiguous": {"res": lambda a: strided(a["res"])},
    }), ("x", "res", "w"))


def _silu_args():
    gu = bf16(T, 2 * N)       # the fused gate/up GEMM output
    return {"out": sentinel(T, N), "gu": gu, "gate": gu[:, :N], "up": gu[:, N:]}


SILU_MUL = Binding(
    _silu_args, lambda a: C.silu_mul(a["out"], a["gate"], a["up"]), ("out",),
    {"out": lambda a: a["out"][:0], "gate": lambda a: a["gate"][:0], "up": lambda a: a["up"][:0]},
    {
        "out one row longer than gate": {"out": lambda a: sentinel(T + 1, N)},
        "out twice as wide as gate": {"out": lambda a: sentinel(T, 2 * N)},
        "up fp32": {"up": lambda a: a["up"].float()},
        "up with another row stride": {"up": lambda a: bf16(T, 3 * N)[:, :N]},
        "gate 8 bytes off alignment": {"gate": lambda a: offset_rows(a["gate"]),
                                       "up": lambda a: offset_rows(a["up"])},
    }, ("gate", "up"))


# --- rope_inplace / store_kv / rope_store_kv --------------------------------------------

def _rope_store_args(fp8):
    fused = bf16(T, (H + 2 * KVH) * D)
    q, k, v = qkv(fused)
    kc, vc, ks, vs = caches(fp8)
    return {"fused": fused, "q": q, "k": k, "v": v, "kc": kc, "vc": vc, "ks": ks, "vs": vs,
            "pos": i64([0, MAX_POS - 1, 5]), "slots": i64([17, 0, NB * BS - 1]),
            "cs": torch_ref.build_cos_sin_cache(D, MAX_POS, 10000.0, DEV)}


def _small_dim_views(a):
    """q / k / v with head_dim 4 (not a multiple of 8), and matching caches."""
    q, k, v = qkv(a["fused"], H * 32, KVH * 32, 4)
    a["kc"], a["vc"] = a["kc"].view(NB, KVH * 32, BS, 4), a["vc"].view(NB, KVH * 32, BS, 4)
    a["cs"] = a["cs"][:, :4].contiguous()
    a["k"], a["v"] = k, v
    return q


_rows_zero = {"q": lambda a: a["q"][:0], "k": lambda a: a["k"][:0], "v": lambda a: a["v"][:0],
              "pos": lambda a: a["pos"][:0], "slots": lambda a: a["slots"][:0]}

_rope_refusals = {
    "positions one too long": {"pos": lambda a: longer(a["pos"])},
    "positions not contiguous": {"pos": lambda a: strided(a["pos"])},
    "cos_sin not contiguous": {"cs": lambda a: strided(a["cs"])},
    "cos_sin twice as wide as head_dim": {"cs": lambda a: torch.cat([a["cs"]] * 2, 1).contiguous()},
    "k one row longer than q": {"k": lambda a: bf16(T + 1, KVH, D)},
    "k with half of q's head_dim": {"k": lambda a: a["k"].view(T, 2 * KVH, D // 2)},
    "head_dim not a multiple of 8": {"q": _small_dim_views},
    "head_dim / 2 above the block size": {
        "q": lambda a: bf16(1, 1, 2056), "k": lambda a: bf16(1, 1, 2056),
        "pos": lambda a: i64([0]), "cs": lambda a: torch.zeros(MAX_POS, 2056, device=DEV)},
}

ROPE_INPLACE = Binding(
    lambda: _rope_store_args(False),
    lambda a: C.rope_inplace(a["q"], a["k"], a["pos"], a["cs"]), ("fused",), _rows_zero,
    _rope_refusals, ("pos", "cs", "k"))


def _store_refusals(fp8):
    r = {
        "slot_mapping one too long": {"slots": lambda a: longer(a["slots"])},
        "slot_mapping not contiguous": {"slots": lambda a: strided(a["slots"])},
        "v with half of k's head_dim": {"v": lambda a: a["v"].view(T, 2 * KVH, D // 2)},
        "caches with half of k's head_dim": {
            "kc": lambda a: a["kc"].view(NB, KVH, 2 * BS, D // 2),
            "vc": lambda a: a["vc"].view(NB, KVH, 2 * BS, D // 2)},
        "caches with twice k's kv heads": {
            "kc": lambda a: a["kc"].view(NB // 2, 2 * KVH, BS, D),
            "vc": lambda a: a["vc"].view(NB // 2, 2 * KVH, BS, D)},
        "v_cache one block longer than k_cache": {"vc": lambda a: longer(a["vc"])},
        "v_cache of the other cache dtype": {
            "vc": lambda a: a["vc"].to(torch.bfloat16) if fp8 else
            torch.zeros(2 * NB, KVH, BS, D, dtype=FP8, device=DEV)[:NB]},   # storage of bf16's size
        "k/v rows 8 bytes off alignment": {"k": lambda a: offset_rows(a["k"]),
                                           "v": lambda a: offset_rows(a["v"])},
    }
    if fp8:
        r.update({
            "v_scale fp64": {"vs": lambda a: a["vs"].double()},
            "v_scale not contiguous": {"vs": lambda a: strided(a["vs"])},
            "k_scale one block longer": {"ks": lambda a: longer(a["ks"])},
            "no scales with an fp8 cache": {"ks": lambda a: no_scale(), "vs": lambda a: no_scale()},
        })
    else:
        r["scales with a bf16 cache"] = {"ks": lambda a: torch.ones(NB, KVH, BS, device=DEV),
                                         "vs": lambda a: torch.ones(NB, KVH, BS, device=DEV)}
        # bf16 only: with head_dim / 8 == 0 the bf16 kernel has no work at all
        r["head_dim not a multiple of 8"] = {"q": _small_dim_views}
    return r


def _store(fp8):
    return Binding(
        lambda: _rope_store_args(fp8),
        lambda a: C.store_kv(a["k"], a["v"], a["kc"], a["vc"], a["slots"], a["ks"], a["vs"]),
        ("kc", "vc", "ks", "vs"), _rows_zero, _store_refusals(fp8),
        ("slots", "v") + (("ks", "vs") if fp8 else ()))


def _rope_store(fp8):
    both = dict(_rope_refusals, **_store_refusals(fp8))
    keep = ["positions one too long", "cos_sin not contiguous", "k one row longer than q",
            "slot_mapping one too long", "v with half of k's head_dim",
            "caches with twice k's kv heads", "v_cache one block longer than k_cache",
            "k/v rows 8 bytes off alignment"]
    keep += ["v_scale fp64", "k_scale one block longer"] if fp8 else ["scales with a bf16 cache"]
    return Binding(
        lambda: _rope_store_args(fp8),
        lambda a: C.rope_store_kv(a["q"], a["k"], a["v"], a["pos"], a["cs"], a["kc"], a["vc"],
                                  a["slots"], a["ks"], a["vs"]),
        ("fused", "kc", "vc", "ks", "vs"), _rows_zero, {k: both[k] for k in keep},
        ("pos", "slots") + (("ks",) if fp8 else ()))


# --- decode attention -----------------------------------------------------------------

def _decode_args(fp8):
    """Two rows of one block each (blocks 0 and 1 of 4), so that even a cache
    read with twice the block size stays inside the allocation."""
    fused = bf16(B, (H + 2 * KVH) * D)
    kc, vc, ks, vs = caches(fp8)
    return {"out": sentinel(B, H, D), "q": qkv(fused)[0], "kc": kc, "vc": vc, "ks": ks, "vs": vs,
            "bt": i32([[0], [1]]), "lens": i32([5, BS]),
            # one shared-prefix tile would need 256 shared keys; zero tiles is
            # the plain path behind the second binding
            "skip": i32([0, 0]), "rows": torch.zeros(0, 64, dtype=torch.int32, device=DEV),
            "nmem": i32([]), "chunks": i32([])}


def _call_decode(a):
    C.attn_decode_paged(a["out"], a["q"], a["kc"], a["vc"], a["bt"], a["lens"], D ** -0.5,
                        a["ks"], a["vs"])


def _call_decode_shared(a):
    C.attn_decode_paged_shared(a["out"], a["q"], a["kc"], a["vc"], a["bt"], a["lens"], D ** -0.5,
                               a["ks"], a["vs"], a["skip"], a["rows"], a["nmem"], a["chunks"])


_decode_zero = {"out": lambda a: a["out"][:0], "q": lambda a: a["q"][:0],
                "bt": lambda a: a["bt"][:0], "lens": lambda a: a["lens"][:0],
                "skip": lambda a: a["skip"][:0]}


def _decode_refusals(fp8):
    r = {
        "block_tables 1-D": {"bt": lambda a: a["bt"].view(-1)},
        "block_tables not contiguous": {"bt": lambda a: strided(a["bt"])},
        "block_tables one row too long": {"bt": lambda a: longer(a["bt"])},
        "block_tables int64": {"bt": lambda a: a["bt"].long()},
        "context_lens one too long": {"lens": lambda a: longer(a["lens"])},
        "context_lens not contiguous": {"lens": lambda a: strided(a["lens"])},
        "out one row longer than q": {"out": lambda a: sentinel(B + 1, H, D)},
        "out 2-D": {"out": lambda a: a["out"].view(B, H * D)},
        "cache head_dim 64": {"kc": lambda a: a["kc"].view(NB, KVH, 2 * BS, D // 2),
                              "vc": lambda a: a["vc"].view(NB, KVH, 2 * BS, D // 2)},
        "v_cache one block longer than k_cache": {"vc": lambda a: longer(a["vc"])},
        "v_cache of the other cache dtype": {
            "vc": lambda a: a["vc"].to(torch.bfloat16) if fp8 else
            torch.zeros(2 * NB, KVH, BS, D, dtype=FP8, device=DEV)[:NB]},   # storage of bf16's size
        "q rows 8 bytes off alignment": {"q": lambda a: offset_rows(a["q"])},
    }
    if fp8:
        r["v_scale fp64"] = {"vs": lambda a: a["vs"].double()}
        r["k_scale one block longer"] = {"ks": lambda a: longer(a["ks"])}
    else:
        r["scales with a bf16 cache"] = {"ks": lambda a: torch.ones(NB, KVH, BS, device=DEV),
                                         "vs": lambda a: torch.ones(NB, KVH, BS, device=DEV)}
    return r


def _decode(fp8):
    return Binding(lambda: _decode_args(fp8), _call_decode, ("out",), _decode_zero,
                   _decode_refusals(fp8), ("bt", "lens") + (("ks", "vs") if fp8 else ()))


def _decode_shared(fp8):
    r = _decode_refusals(fp8)
    r = {k: r[k] for k in ("block_tables 1-D", "context_lens one too long",
                           "out one row longer than q", "cache head_dim 64")}
    r["skip_chunks one too long"] = {"skip": lambda a: longer(a["skip"])}
    r["tile_chunks one too long"] = {"chunks": lambda a: i32([0])}
    return Binding(lambda: _decode_args(fp8), _call_decode_shared, ("out",), _decode_zero, r,
                   ("bt", "skip"))


# --- packed prefill attention ---------------------------------------------------------

def _prefill_args():
    # k and v end one head short of their buffer's row, so that a kernel handed
    # a q head past the last kv-head group would still read inside it
    fused = bf16(T, (H + 2 * (KVH + 1)) * D)
    q = fused[:, :H * D].view(T, H, D)
    k = fused[:, H * D:(H + KVH) * D].view(T, KVH, D)
    v = fused[:, (H + KVH + 1) * D:(H + 2 * KVH + 1) * D].view(T, KVH, D)
    # two sequences (2 rows and 1 row), one workgroup each
    return {"out": sentinel(T, H, D), "fused": fused, "q": q, "k": k, "v": v,
            "start": i32([0, 2]), "qpos0": i32(([0] + [-1] * 7) * 2), "seqlen": i32([2, 1])}


PREFILL = Binding(
    _prefill_args,
    lambda a: C.attn_prefill(a["out"], a["q"], a["k"], a["v"], a["start"], a["qpos0"],
                             a["seqlen"], D ** -0.5),
    ("out",),
    {"out": lambda a: a["out"][:0], "q": lambda a: a["q"][:0], "k": lambda a: a["k"][:0],
     "v": lambda a: a["v"][:0], "start": lambda a: a["start"][:0],
     "qpos0": lambda a: a["qpos0"][:0], "seqlen": lambda a: a["seqlen"][:0]},
    {
        "grp_seqlen one too long": {"seqlen": lambda a: longer(a["seqlen"])},
        "grp_seqlen not contiguous": {"seqlen": lambda a: strided(a["seqlen"])},
        "grp_seq_start not contiguous": {"start": lambda a: strided(a["start"])},
        "grp_qpos0 one too long": {"qpos0": lambda a: longer(a["qpos0"])},
        "grp_qpos0 not contiguous": {"qpos0": lambda a: strided(a["qpos0"])},
        "grp_seq_start int64": {"start": lambda a: a["start"].long()},
        "out one row longer than q": {"out": lambda a: sentinel(T + 1, H, D)},
        "k and v one row longer than q": {"k": lambda a: bf16(T + 1, KVH, D),
                                          "v": lambda a: bf16(T + 1, KVH, D)},
        "v with half of k's head_dim": {"v": lambda a: a["v"].view(T, 2 * KVH, D // 2)},
        "k and v with half of q's head_dim": {"k": lambda a: a["k"].view(T, 2 * KVH, D // 2),
                                              "v": lambda a: a["v"].view(T, 2 * KVH, D // 2)},
        # the spare head after v, inside the same fused row
        "v with twice k's kv heads": {
            "v": lambda a: a["fused"][:, (H + KVH + 1) * D:(H + KVH + 3) * D].view(T, 2 * KVH, D)},
        "H not a multiple of KVH": {"q": lambda a: bf16(T, 3, D), "out": lambda a: sentinel(T, 3, D),
                                    "k": lambda a: bf16(T, 3, D)[:, :2], "v": lambda a: bf16(T, 3, D)[:, :2]},
    }, ("start", "qpos0", "seqlen"))


# --- sampler ----------------------------------------------------------------------------

def _sample_args():
    return {"tokens": torch.full((B,), -7, dtype=torch.int64, device=DEV),
            "logprobs": sentinel(B, dtype=torch.float32),
            "logits": torch.randn(B, V, device=DEV),
            "temps": torch.tensor([0.0, 0.8], device=DEV), "top_ps": torch.tensor([1.0, 0.9], device=DEV),
            "top_ks": i32([0, 5]), "seeds": i64([1, 2]), "steps": i64([0, 3]),
            "mask": torch.full((B, W), -1, dtype=torch.int32, device=DEV),
            "dbg": torch.zeros(B, 16, device=DEV)}


_ROW_KEYS = ("tokens", "logprobs", "temps", "top_ps", "top_ks", "seeds", "steps")

SAMPLE = Binding(
    _sample_args,
    lambda a: C.sample(a["tokens"], a["logprobs"], a["logits"], a["temps"], a["top_ps"],
                       a["top_ks"], a["seeds"], a["steps"], a["mask"], a["dbg"]),
    ("tokens", "logprobs", "dbg"),
    dict({k: (lambda a, k=k: a[k][:0]) for k in _ROW_KEYS + ("logits", "mask", "dbg")}),
    dict({f"{k} one too long": {k: (lambda a, k=k: longer(a[k]))} for k in _ROW_KEYS}, **{
        "temperatures not contiguous": {"temps": lambda a: strided(a["temps"])},
        "temperatures fp64": {"temps": lambda a: a["temps"].double()},
        "top_ks int64": {"top_ks": lambda a: a["top_ks"].long()},
        "seeds not contiguous": {"seeds": lambda a: strided(a["seeds"])},
        "logits 1-D": {"logits": lambda a: a["logits"].view(-1)},
        "mask one word wider": {"mask": lambda a: longer(a["mask"], 1)},
        "mask one row longer": {"mask": lambda a: longer(a["mask"])},
        "mask int64": {"mask": lambda a: a["mask"].long()},
        "mask not contiguous": {"mask": lambda a: strided(a["mask"])},
        "dbg one column wider": {"dbg": lambda a: torch.zeros(B, 17, device=DEV)},
        "dbg fp64": {"dbg": lambda a: a["dbg"].double()},
    }), ("temps", "top_ks", "steps", "tokens"))


# --- Levenshtein, all-reduce, MFMA self-test ------------------------------------------------

def _lev_args():
    chars = torch.full((3, 64), ord("a"), dtype=torch.uint8, device=DEV)
    chars[1, :2] = ord("b")
    return {"chars": chars, "lens": i32([0, 2, 64]), "pi": i32([0, 1, 2]), "pj": i32([1, 2, 0])}


LEVENSHTEIN = Binding(
    _lev_args, lambda a: C.levenshtein_pairs(a["chars"], a["lens"], a["pi"], a["pj"]), (),
    {"pi": lambda a: a["pi"][:0], "pj": lambda a: a["pj"][:0]},
    {
        "chars 1-D": {"chars": lambda a: a["chars"].view(-1)},
        "chars 32 wide": {"chars": lambda a: a["chars"].view(6, 32)},
        "chars not contiguous": {"chars": lambda a: strided(a["chars"])},
        "lens one too long": {"lens": lambda a: longer(a["lens"])},
        "lens not contiguous": {"lens": lambda a: strided(a["lens"])},
        "lens int64": {"lens": lambda a: a["lens"].long()},
        "pair_j one too long": {"pj": lambda a: longer(a["pj"])},
        "pair_i not contiguous": {"pi": lambda a: strided(a["pi"])},
    }, ("lens", "pi", "pj", "chars"))


def _allreduce_args():
    return {"a": bf16(64), "b": bf16(64)}


ALLREDUCE = Binding(
    _allreduce_args, lambda a: C.one_shot_allreduce([a["a"], a["b"]]), ("a", "b"),
    {"a": lambda a: a["a"][:0], "b": lambda a: a["b"][:0]},
    {
        "second buffer one vector longer": {"b": lambda a: bf16(72)},
        "second buffer fp32": {"b": lambda a: a["b"].float()},
        "second buffer not contiguous": {"b": lambda a: strided(a["b"])},
        "second buffer 8 bytes off alignment": {"b": lambda a: bf16(72)[4:68]},
    }, ("b",))


BINDINGS = {
    "rmsnorm": RMSNORM, "fused_add_rmsnorm": FUSED_ADD_RMSNORM, "silu_mul": SILU_MUL,
    "rope_inplace": ROPE_INPLACE,
    "store_kv-bf16": _store(False), "store_kv-fp8": _store(True),
    "rope_store_kv-bf16": _rope_store(False), "rope_store_kv-fp8": _rope_store(True),
    "attn_decode_paged-bf16": _decode(False), "attn_decode_paged-fp8": _decode(True),
    "attn_decode_paged_shared-bf16": _decode_shared(False),
    "attn_decode_paged_shared-fp8": _decode_shared(True),
    "attn_prefill": PREFILL, "sample": SAMPLE, "levenshtein_pairs": LEVENSHTEIN,
    "one_shot_allreduce": ALLREDUCE,
}

REFUSALS = [(b, what) for b, spec in BINDINGS.items() for what in spec.refusals]
CPU_CASES = [(b, key) for b, spec in BINDINGS.items() for key in spec.cpu]


@pytest.mark.parametrize("name", list(BINDINGS))
def test_accepts_the_unedited_arguments(name):
    """The refusal cases start from a call the binding takes, and that call
    writes its outputs."""
    binding = BINDINGS[name]
    torch.manual_seed(0)
    a = binding.args()
    before = [bits(a[k]).clone() for k in binding.outs]
    result = binding.call(a)
    torch.cuda.synchronize()
    written = [not torch.equal(bits(a[k]), b) for k, b in zip(binding.outs, before) if b.numel()]
    assert all(written), dict(zip(binding.outs, written))
    if name == "levenshtein_pairs":
        assert result.tolist() == [2, 64, 64]


@pytest.mark.parametrize("name", list(BINDINGS))
def test_zero_rows_launch_nothing(name):
    binding = BINDINGS[name]
    torch.manual_seed(0)
    run_unchanged(binding, binding.args(), binding.zero, raises=False)


@pytest.mark.parametrize("name,what", REFUSALS, ids=[f"{b}: {w}" for b, w in REFUSALS])
def test_refuses(name, what):
    binding = BINDINGS[name]
    torch.manual_seed(0)
    run_unchanged(binding, binding.args(), binding.refusals[what], raises=True)


@pytest.mark.parametrize("name,key", CPU_CASES, ids=[f"{b}: {k}" for b, k in CPU_CASES])
def test_refuses_a_cpu_tensor_in_the_zero_row_call(name, key):
    binding = BINDINGS[name]
    torch.manual_seed(0)
    edits = dict(binding.zero)
    zero_edit = edits.get(key, lambda a: a[key])
    edits[key] = lambda a: zero_edit(a).cpu()
    run_unchanged(binding, binding.args(), edits, raises=True)


def test_mfma_selftest_refuses_other_shapes():
    a, b = bf16(32, 16), bf16(16, 32)
    assert C.mfma_selftest(a, b).shape == (32, 32)
    for bad_a, bad_b in ((bf16(33, 16), b), (a, bf16(16, 33)), (a.float(), b),
                         (a, strided(b)), (bf16(16, 32), bf16(32, 16))):
        with pytest.raises(RuntimeError):
            C.mfma_selftest(bad_a, bad_b)
    torch.cuda.synchronize()
