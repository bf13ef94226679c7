"""Float64 oracles, derived bounds, mutants and shared cases for the fp8 (e4m3)
expert-weight tests (not a test module itself; imported like ``fp8w_oracles``,
on which it builds).

The batched op, from its definition:

    out[e, m, n] = (sum_k x_e[m, k] * q[e, n, k]) * scale[e, n]

with ``x_e = x`` ([M, K], shared by all experts) or ``x_e = x[e]`` ([E, M, K]).
Per expert this is the op of ``fp8w_oracles`` without bias, so its bound
carries over slice by slice: ``|a - e| <= 2^-7 |e| + K * 2^-23 * Mag``. The
grouped fp8 ``moe_down`` with a given bf16 ``act`` is exactly this op on each
expert's rows.

The grouped fp8 ``moe_gateup`` computes ``silu(g) * u`` from the two halves
``g``, ``u`` of the gate_up product. With ``|silu'| <= 1.1`` an accumulation
error ``dg <= c * Mag_g`` moves the result by at most ``1.1 * dg * |u|`` and
``du <= c * Mag_u`` by ``|silu(g)| * du``; the ``__expf`` error and the final
bf16 rounding sit inside the relative term:

    |a - e| <= 2^-7 |e| + K * 2^-23 * (1.1 * Mag_g * |u| + |silu(g)| * Mag_u)

Inputs follow ``fp8w_oracles.gemm_case`` per expert: weight row n scaled by
``1 + n % 5``, expert e by a further ``1 + e / 2``, one 1.5 outlier per
expert, so that a scale or an expert taken from the wrong place is visible.

Mutants that need a second expert (another expert's q, scales rolled by one
expert, expert 0's x) are the identity at E = 1 and are listed only for
E > 1; "x[0] for every expert" only where x is per expert. Every mutant that
is listed for a case must exceed the bound on it.
"""

import torch

import fp8w_oracles as fo
from kernel_oracles import F64, check, f64  # noqa: F401  (re-exported)

c_kernel = fo.c_kernel
c_large_m = fo.c_large_m


def expert_weights(E, N, K, g):
    """(q [E, N, K] e4m3, scale [E, N] fp32), each expert quantised per row
    with the float64 quantiser of ``fp8w_oracles``."""
    qs, ss = [], []
    for e in range(E):
        w = torch.randn(N, K, generator=g) * 0.02
        w = w * (1.0 + (torch.arange(N) % 5).float()).unsqueeze(1) * (1.0 + 0.5 * e)
        w[N // 3, K // 2] = 1.5 * (1.0 + 0.5 * e)
        q, s = fo.quantize_rows(w.bfloat16())
        qs.append(q)
        ss.append(s)
    return torch.stack(qs), torch.stack(ss)


def oracle(x, q, scale, *, q_used=None, scale_used=None, x_used=None, k_keep=None):
    """(e, Mag) in float64, [E, M, N]. The ``*_used`` operands and ``k_keep``
    exist for the mutants; Mag always comes from the true operands."""
    E = q.shape[0]
    es, mags = [], []
    for i in range(E):
        xe = x if x.dim() == 2 else x[i]
        _, mag = fo.oracle(xe, q[i], scale[i])
        xu = xe if x_used is None else (x_used if x_used.dim() == 2 else x_used[i])
        e, _ = fo.oracle(xu, (q if q_used is None else q_used)[i], scale[i], k_keep=k_keep,
                         scale_used=(scale if scale_used is None else scale_used)[i])
        es.append(e)
        mags.append(mag)
    return torch.stack(es), torch.stack(mags)


def silu64(g):
    return g / (1.0 + torch.exp(-g))


def gateup_from(e, mag):
    """(silu(g) * u, bound magnitude) from the gate_up product's (e, Mag),
    whose last dim is the fused [gate; up] stack."""
    IN = e.shape[-1] // 2
    g, u = e[..., :IN], e[..., IN:]
    mg, mu = mag[..., :IN], mag[..., IN:]
    return silu64(g) * u, 1.1 * mg * u.abs() + silu64(g).abs() * mu


# --- mutants of the batched op: each returns the mutated [E, M, N] output ---------

def _mut(case, **kw):
    return oracle(case["x"], case["q"], case["scale"], **kw)[0]


def previous_experts_q(case):
    return _mut(case, q_used=torch.roll(case["q"].view(torch.uint8), 1, 0).view(torch.float8_e4m3fn))


def scale_rolled_expert(case):
    return _mut(case, scale_used=torch.roll(case["scale"], 1, 0))


def scale_rolled_channel(case):
    return _mut(case, scale_used=torch.roll(case["scale"], 1, 1))


def drop_last_16_k(case):
    return _mut(case, k_keep=slice(0, case["K"] - 16))


def shared_x0(case):
    return _mut(case, x_used=case["x"][0])


def mutants(case):
    """The mutants that are not the identity on this case."""
    m = {"last 16 k dropped": drop_last_16_k,
         "scale rolled by one channel": scale_rolled_channel}
    if case["E"] > 1:
        m["expert e uses expert e-1's q"] = previous_experts_q
        m["scale rolled by one expert"] = scale_rolled_expert
        if case["x"].dim() == 3:
            m["x[0] used for every expert"] = shared_x0
    return m


def gateup_scales_swapped(case):
    """gate_up only: the gate channels take the up scales and vice versa."""
    IN = case["scale"].shape[1] // 2
    sw = torch.cat([case["scale"][:, IN:], case["scale"][:, :IN]], dim=1)
    return _mut(case, scale_used=sw)


# --- shared cases (CPU tensors; the GPU tests move them to the device) --------------

_cases = {}


def batched_case(E, M, N, K, per_expert, wide=False):
    """x ~ N(0, 1) bf16, [M, K] or (``per_expert``) [E, M, K]. ``wide``: the
    per-expert x is a view of a buffer [E, M + 3, K + 24] (row stride 24
    elements wider, a gap of three rows between experts). Oracle computed once
    and shared."""
    key = (E, M, N, K, per_expert, wide)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(9100 + 1000 * E + 7 * M + 3 * N + K + (1 if per_expert else 0))
    if per_expert:
        buf = torch.randn(E, M + (3 if wide else 0), K + (24 if wide else 0), generator=g).bfloat16()
        x = buf[:, :M, :K]
    else:
        assert not wide
        buf = torch.randn(M, K, generator=g).bfloat16()
        x = buf
    q, scale = expert_weights(E, N, K, g)
    e, mag = oracle(x, q, scale)
    case = {"name": f"E={E} M={M} N={N} K={K} " + ("per-expert x" if per_expert else "shared x")
                    + (" strided" if wide else ""),
            "buf": buf, "x": x, "q": q, "scale": scale, "e": e, "mag": mag,
            "E": E, "M": M, "N": N, "K": K}
    _cases[key] = case
    return case


# sorted-row layout of the grouped kernels, E = 4: expert 0 exactly 128 rows,
# expert 1 empty, expert 2 256 rows, expert 3 37 rows padded to 128
GROUPED_PAD_OFFSETS = [0, 128, 128, 384, 512]
GROUPED_COUNTS = [128, 0, 256, 37]


def grouped_down_case(IN, H=128):
    """act [S, IN] bf16 in sorted-row space (every row random: the kernel
    computes pad rows too, row by row), w_down [E, H, IN]; the oracle per
    expert over that expert's row range, stacked to [S, H]."""
    key = ("down", IN, H)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(9300 + IN + H)
    S = GROUPED_PAD_OFFSETS[-1]
    act = torch.randn(S, IN, generator=g).bfloat16()
    q, scale = expert_weights(4, H, IN, g)
    e = torch.zeros(S, H, dtype=F64)
    mag = torch.zeros(S, H, dtype=F64)
    for i in range(4):
        lo, hi = GROUPED_PAD_OFFSETS[i], GROUPED_PAD_OFFSETS[i + 1]
        if hi > lo:
            e[lo:hi], mag[lo:hi] = fo.oracle(act[lo:hi], q[i], scale[i])
    case = {"name": f"down IN={IN} H={H}", "act": act, "q": q, "scale": scale,
            "e": e, "mag": mag, "K": IN}
    _cases[key] = case
    return case


def grouped_gateup_case(K, IN=128, T=200):
    """x [T, K], w_gate_up [E, 2*IN, K], sorted_ids [S] with -1 in expert 3's
    pad slots; oracle silu(g) * u over the sorted rows ([S, IN]; pad rows 0
    with a zero bound: silu(0) * 0 must come out exactly 0)."""
    key = ("gateup", K, IN, T)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(9400 + K + IN)
    S = GROUPED_PAD_OFFSETS[-1]
    x = torch.randn(T, K, generator=g).bfloat16()
    q, scale = expert_weights(4, 2 * IN, K, g)
    ids = torch.full((S,), -1, dtype=torch.int32)
    e = torch.zeros(S, IN, dtype=F64)
    mag = torch.zeros(S, IN, dtype=F64)
    e_sw = torch.zeros(S, IN, dtype=F64)
    IN2 = 2 * IN
    sw = torch.cat([scale[:, IN:], scale[:, :IN]], dim=1)
    for i in range(4):
        lo, n = GROUPED_PAD_OFFSETS[i], GROUPED_COUNTS[i]
        if n == 0:
            continue
        tok = torch.randint(0, T, (n,), generator=g)
        ids[lo:lo + n] = tok.to(torch.int32)
        eg, mg = fo.oracle(x[tok], q[i], scale[i])
        assert eg.shape[1] == IN2
        e[lo:lo + n], mag[lo:lo + n] = gateup_from(eg, mg)
        e_sw[lo:lo + n] = gateup_from(fo.oracle(x[tok], q[i], scale[i], scale_used=sw[i])[0], mg)[0]
    case = {"name": f"gate_up K={K} IN={IN}", "x": x, "q": q, "scale": scale, "sorted_ids": ids,
            "e": e, "mag": mag, "e_scales_swapped": e_sw, "K": K}
    _cases[key] = case
    return case
