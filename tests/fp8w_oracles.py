"""Float64 oracle, derived bounds, mutants and shared cases for the weight-only
fp8 (e4m3) GEMM tests (not a test module itself; imported like
``kernel_oracles``).

The op, from its definition:

    out[m, n] = (sum_k x[m, k] * q[n, k]) * scale[n] + bias[n]

The oracle evaluates it in float64 on the exactly widened operands and never
calls ``ops/torch_ref.py`` (which is one of the things checked against it).

Bound (the rule of ``kernel_oracles``, extended): an output ``a`` is accepted
against the float64 value ``e`` when

    |a - e| <= 2^-7 * |e| + c * Mag,
    Mag[m, n] = scale[n] * sum_k |x[m, k]| * |q[n, k]|  (+ |bias[n]|)

- kernel path, ``c = K * 2^-23``: e4m3 x bf16 products are exact in fp32 (3 + 8
  significant bits); at most K accumulation steps each lose at most 2^-24
  relative to rounding, doubled in case the MFMA truncates.
- large-M path, ``c = 2^-9 + K * 2^-23``: each dequantised weight
  ``bf16(q * scale)`` is rounded to bf16 once (half a bf16 ulp, 2^-9), then
  the same accumulation.

The constants are derived, not measured, and are not to be widened.
"""

import torch

from kernel_oracles import F64, check, f64  # noqa: F401  (re-exported)


def c_kernel(K):
    return K * 2.0 ** -23


def c_large_m(K):
    return 2.0 ** -9 + K * 2.0 ** -23


def oracle(x, q, scale, bias=None, *, k_keep=None, scale_used=None):
    """(e, Mag) in float64. ``k_keep`` (slice of k) and ``scale_used`` exist
    for the mutants; Mag always comes from the true operands."""
    xd, qd, sd = f64(x), f64(q), f64(scale)
    mag = (xd.abs() @ qd.abs().t()) * sd
    su = sd if scale_used is None else f64(scale_used)
    if k_keep is not None:
        xd, qd = xd[:, k_keep], qd[:, k_keep]
    e = (xd @ qd.t()) * su
    if bias is not None:
        e = e + f64(bias)
        mag = mag + f64(bias).abs()
    return e, mag


# mutants: the oracle with a classic defect; each returns the mutated output

def drop_last_16_k(case):
    K = case["x"].shape[1]
    return oracle(case["x"], case["q"], case["scale"], case["bias"], k_keep=slice(0, K - 16))[0]


def scale_rolled(case):
    return oracle(case["x"], case["q"], case["scale"], case["bias"],
                  scale_used=torch.roll(case["scale"], 1))[0]


def scale_ignored(case):
    return oracle(case["x"], case["q"], case["scale"], case["bias"],
                  scale_used=torch.ones_like(case["scale"]))[0]


MUTANTS = {
    "last 16 k dropped": drop_last_16_k,
    "scale rolled by one channel": scale_rolled,
    "scale ignored": scale_ignored,
}


# --- shared cases (CPU tensors; the GPU tests move them to the device) ----------

_cases = {}


def quantize_rows(w):
    """The quantiser from its definition, float64 division: scale = amax / 448
    (1.0 for a zero row), q = RNE(w / scale) clamped to +-448."""
    wd = f64(w)
    amax = wd.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).float()
    q = (wd / scale.to(F64).unsqueeze(1)).clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)
    return q, scale


def gemm_case(M, N, K, bias=False, x_dtype=torch.bfloat16, wide=False):
    """x ~ N(0, 1), w ~ 0.02 * N(0, 1) with one 1.5 outlier (a row whose scale
    is ~20x its neighbours'), quantised per row; rows get scales of different
    sizes (row n scaled by 1 + n % 5). ``wide``: x is a row-strided view of a
    buffer 24 columns wider. Oracle computed once and shared."""
    key = (M, N, K, bias, x_dtype, wide)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(9000 + 7 * M + 3 * N + K + (1 if bias else 0))
    buf = torch.randn(M, K + (24 if wide else 0), generator=g).to(x_dtype)
    x = buf[:, :K]
    w = torch.randn(N, K, generator=g) * 0.02
    w = w * (1.0 + (torch.arange(N) % 5).float()).unsqueeze(1)
    w[N // 3, K // 2] = 1.5
    q, scale = quantize_rows(w.bfloat16())
    b = (torch.randn(N, generator=g) * 0.5).to(x_dtype) if bias else None
    e, mag = oracle(x, q, scale, b)
    case = {"name": f"M={M} N={N} K={K}" + (" bias" if bias else "") + (" strided" if wide else ""),
            "buf": buf, "x": x, "q": q, "scale": scale, "bias": b, "e": e, "mag": mag, "K": K}
    _cases[key] = case
    return case


def all_finite_bytes():
    """The 254 finite e4m3 encodings (0x7F and 0xFF are the NaNs)."""
    return torch.tensor([b for b in range(256) if b not in (0x7F, 0xFF)], dtype=torch.uint8)
