"""Float64 oracles, derived bounds, mutants and shared cases for the bf16 grouped
MoE kernels (``moe_gateup`` / ``moe_down``) and the host path around them,
``MixtralMoE._forward_grouped_hip`` (not a test module itself; imported like
``fp8_expert_oracles``, on which it builds).

Everything is evaluated through ``fp8w_oracles.oracle`` with ``scale = ones``:
bf16 widens exactly through ``kernel_oracles.f64``, so the oracle sees the very
weights the kernel reads. Nothing here goes through ``ops/torch_ref.py`` or
``MixtralMoE._forward_grouped``.

Bounds
------
An output ``a`` is accepted against the float64 value ``e`` when
``|a - e| <= 2^-7 |e| + (absolute term)``; ``2^-7 |e|`` is one bf16 ulp of the
oracle, as in ``kernel_oracles``.

- ``moe_down``, bf16 weights: ``y[s, n] = sum_i act[s, i] * Wd[e, n, i]``.
  bf16 x bf16 products carry 8 + 8 = 16 significant bits and are exact in fp32,
  so the argument of ``fp8w_oracles`` carries over unchanged: at most ``IN``
  accumulation steps, each losing at most 2^-24 relative to rounding, doubled in
  case the MFMA truncates.

      |a - e| <= 2^-7 |e| + IN * 2^-23 * Mag,   Mag = sum_i |act_i| |Wd_ni|

- ``moe_gateup``, bf16 weights: ``act = silu(g) * u`` from the two halves of the
  gate_up product. The ``gateup_from`` bound of ``fp8_expert_oracles``: with
  ``|silu'| <= 1.1`` an accumulation error ``dg <= c * Mag_g`` moves the result
  by at most ``1.1 * dg * |u|`` and ``du <= c * Mag_u`` by ``|silu(g)| * du``;
  the ``__expf`` error and the final bf16 rounding sit inside the relative term.

      |a - e| <= 2^-7 |e| + K * 2^-23 * (1.1 * Mag_g * |u| + |silu(g)| * Mag_u)

  A pad row (``sorted_ids == -1``) reads the zero page: ``e = 0`` with a zero
  bound, so it must come out exactly 0.

- the whole ``_forward_grouped_hip``: for token t with experts j and routing
  weights w_j, ``e_t = sum_j w_j * (act_j @ Wd_j^T)`` with ``act_j`` the
  unrounded float64 ``silu(g) * u``.

      |a - e| <= 2^-7 |e| + sum_j w_j * ((2^-8 + I * 2^-23) * A_j + K * 2^-23 * G_j)
      A_j = sum_i |act_ji| |Wd_ni|,   G_j = sum_i MagAct_ji |Wd_ni|

  ``MagAct`` is the gate_up bound magnitude above: ``K * 2^-23 * MagAct`` is the
  error of ``act`` before it is stored, which the down product carries to
  ``K * 2^-23 * G_j``. ``2^-8`` is half a bf16 ulp (2^-9) for the stored ``act``
  plus half a bf16 ulp for the stored ``y`` (``|y| <= A``); ``I * 2^-23 * A`` is
  the down accumulation. The fp32 weighted sum and the final rounding sit
  inside the relative term.

The constants are derived, not measured, and are not to be widened.

Cases
-----
Op level: sorted-row layout with E = 5, ``pad_offsets = [0, 0, 128, 384, 384,
512]`` and counts ``[0, 128, 129, 0, 1]``: an empty first expert, an exact tile,
one row over a tile (two m-tiles: the block loops), an empty expert in the
middle, a last expert of one row. 192 output channels (three n-tiles, an odd
count); K (gate_up) / IN (down) in {64, 192, 1088}: one stage with no double
buffering, three stages (an odd count: the last stage sits in buffer 0 when the
next m-tile restages buffer 0), 17 stages. Weights are shaped as
``fp8_expert_oracles.expert_weights`` shapes them (row n scaled by ``1 + n % 5``,
expert e by ``1 + e / 2``, one outlier per expert), so a wrong expert or channel
is visible. ``x`` is [150, K]; tokens repeat across experts.

Module level: H = 128, I = 192, hand-made routing with peaked weights; see
``MODULE_CASES``.

Mutants are the float64 oracle with a defect, rounded to bf16, and are listed
only for the cases on which they are not the identity.
"""

import torch

import fp8_expert_oracles as eo
import fp8w_oracles as fo
from kernel_oracles import F64, check, f64  # noqa: F401  (re-exported)

c_kernel = fo.c_kernel

BM = 128
PAD_OFFSETS = [0, 0, 128, 384, 384, 512]
COUNTS = [0, 128, 129, 0, 1]
E_OP = len(COUNTS)
S_OP = PAD_OFFSETS[-1]
T_OP = 150
N_OP = 192                      # IN of gate_up, H of down: three n-tiles
OP_DEPTHS = [64, 192, 1088]     # K of gate_up, IN of down
PREFILL = 3.0                   # what the tests put into the output beforehand

_cases = {}


def _cached(key, fn):
    if key not in _cases:
        _cases[key] = fn()
    return _cases[key]


def shaped(E, N, K, g):
    """fp32 [E, N, K] with the shaping of ``fp8_expert_oracles.expert_weights``."""
    ws = []
    for e in range(E):
        w = torch.randn(N, K, generator=g) * 0.02
        w = w * (1.0 + (torch.arange(N) % 5).float()).unsqueeze(1) * (1.0 + 0.5 * e)
        w[N // 3, K // 2] = 1.5 * (1.0 + 0.5 * e)
        ws.append(w)
    return torch.stack(ws)


def bf16_weights(E, N, K, g):
    return shaped(E, N, K, g).bfloat16()


def e4m3_exact_weights(E, N, K, g):
    """(w bf16, q e4m3, ones [E, N]): the same values in both types (the
    shaped weights x4, which lifts most of them out of e4m3's subnormals,
    rounded to e4m3; e4m3 widens to bf16 exactly)."""
    q = (shaped(E, N, K, g) * 4.0).to(torch.float8_e4m3fn)
    return q.float().bfloat16(), q, torch.ones(E, N)


def _ones(w):
    return torch.ones(w.shape[0])


def _expert_rows(e):
    """(lo, n): first sorted row and number of real rows of expert e."""
    return PAD_OFFSETS[e], COUNTS[e]


# --- op level: oracles ------------------------------------------------------------

def gateup_eval(x, w, ids, *, w_used=None, k_keep=None):
    """(e, mag) [S, IN] float64 of moe_gateup over the op-level layout; pad
    rows 0 with a zero bound. ``w_used`` / ``k_keep`` exist for the mutants;
    mag always comes from the true operands."""
    IN = w.shape[1] // 2
    e = torch.zeros(S_OP, IN, dtype=F64)
    mag = torch.zeros(S_OP, IN, dtype=F64)
    wu = w if w_used is None else w_used
    for i in range(E_OP):
        lo, n = _expert_rows(i)
        if n == 0:
            continue
        xs = x[ids[lo:lo + n].long()]
        _, mg = fo.oracle(xs, w[i], _ones(w[i]))
        eg, _ = fo.oracle(xs, wu[i], _ones(w[i]), k_keep=k_keep)
        e[lo:lo + n], mag[lo:lo + n] = eo.gateup_from(eg, mg)
    return e, mag


def down_eval(act, w, *, w_used=None, k_keep=None):
    """(e, mag) [S, H] float64 of moe_down: the kernel computes every row of
    an expert's padded range, so every row is checked."""
    H = w.shape[1]
    e = torch.zeros(S_OP, H, dtype=F64)
    mag = torch.zeros(S_OP, H, dtype=F64)
    wu = w if w_used is None else w_used
    for i in range(E_OP):
        lo, hi = PAD_OFFSETS[i], PAD_OFFSETS[i + 1]
        if hi == lo:
            continue
        _, mag[lo:hi] = fo.oracle(act[lo:hi], w[i], _ones(w[i]))
        e[lo:hi], _ = fo.oracle(act[lo:hi], wu[i], _ones(w[i]), k_keep=k_keep)
    return e, mag


def _sorted_ids(g):
    ids = torch.full((S_OP,), -1, dtype=torch.int32)
    for i in range(E_OP):
        lo, n = _expert_rows(i)
        if n:
            ids[lo:lo + n] = torch.randint(0, T_OP, (n,), generator=g).to(torch.int32)
    return ids


def gateup_case(K, e4m3_exact=False):
    """x [150, K] bf16 ~ N(0, 1), w [5, 384, K] bf16, sorted_ids [512] with -1
    in pad slots. ``e4m3_exact``: the weights are e4m3-representable and the
    case also holds them as ``q`` with unit ``scale``."""
    def build():
        g = torch.Generator().manual_seed(9500 + K + (1 if e4m3_exact else 0))
        x = torch.randn(T_OP, K, generator=g).bfloat16()
        case = {"name": f"gate_up K={K} IN={N_OP}" + (" e4m3-exact" if e4m3_exact else ""),
                "kind": "gateup", "x": x, "K": K}
        if e4m3_exact:
            case["w"], case["q"], case["scale"] = e4m3_exact_weights(E_OP, 2 * N_OP, K, g)
        else:
            case["w"] = bf16_weights(E_OP, 2 * N_OP, K, g)
        case["sorted_ids"] = _sorted_ids(g)
        case["e"], case["mag"] = gateup_eval(x, case["w"], case["sorted_ids"])
        return case

    return _cached(("gateup", K, e4m3_exact), build)


def down_case(IN, e4m3_exact=False):
    """act [512, IN] bf16 ~ N(0, 1) in sorted-row space (every row random),
    w [5, 192, IN] bf16."""
    def build():
        g = torch.Generator().manual_seed(9600 + IN + (1 if e4m3_exact else 0))
        act = torch.randn(S_OP, IN, generator=g).bfloat16()
        case = {"name": f"down IN={IN} H={N_OP}" + (" e4m3-exact" if e4m3_exact else ""),
                "kind": "down", "act": act, "K": IN}
        if e4m3_exact:
            case["w"], case["q"], case["scale"] = e4m3_exact_weights(E_OP, N_OP, IN, g)
        else:
            case["w"] = bf16_weights(E_OP, N_OP, IN, g)
        case["e"], case["mag"] = down_eval(act, case["w"])
        return case

    return _cached(("down", IN, e4m3_exact), build)


def op_cases():
    return [gateup_case(K) for K in OP_DEPTHS] + [down_case(IN) for IN in OP_DEPTHS]


def _silu32(g):
    return g / (1.0 + torch.exp(-g))


def emulate_op(case):
    """The kernels' arithmetic: fp32 matmul, fp32 silu, one bf16 rounding."""
    w = case["w"].float()
    if case["kind"] == "down":
        out = torch.zeros(S_OP, w.shape[1])
        for i in range(E_OP):
            lo, hi = PAD_OFFSETS[i], PAD_OFFSETS[i + 1]
            if hi > lo:
                out[lo:hi] = case["act"][lo:hi].float() @ w[i].t()
        return out.bfloat16()
    IN = w.shape[1] // 2
    out = torch.zeros(S_OP, IN)
    ids = case["sorted_ids"]
    for i in range(E_OP):
        lo, n = _expert_rows(i)
        if n:
            gu = case["x"][ids[lo:lo + n].long()].float() @ w[i].t()
            out[lo:lo + n] = _silu32(gu[:, :IN]) * gu[:, IN:]
    return out.bfloat16()


# --- op level: mutants --------------------------------------------------------------

def _op_eval(case, **kw):
    if case["kind"] == "down":
        return down_eval(case["act"], case["w"], **kw)[0]
    return gateup_eval(case["x"], case["w"], case["sorted_ids"], **kw)[0]


def op_previous_experts_weights(case):
    return _op_eval(case, w_used=torch.roll(case["w"], 1, 0))


def op_gate_up_swapped(case):
    IN = case["w"].shape[1] // 2
    return _op_eval(case, w_used=torch.cat([case["w"][:, IN:], case["w"][:, :IN]], dim=1))


def op_drop_last_16_k(case):
    return _op_eval(case, k_keep=slice(0, case["K"] - 16))


def op_rows_shifted(case):
    return torch.roll(case["e"], 1, 0)


def op_second_m_tile_unwritten(case):
    """Rows [256, 384), the second m-tile of the 129-row expert, keep what the
    output held before the launch."""
    out = case["e"].clone()
    out[PAD_OFFSETS[2] + BM:PAD_OFFSETS[3]] = PREFILL
    return out


def op_mutants(case):
    m = {"expert e uses expert e-1's weights": op_previous_experts_weights,
         "last 16 k dropped": op_drop_last_16_k,
         "output rows shifted by one (sorted space)": op_rows_shifted,
         "second m-tile of the 129-row expert unwritten": op_second_m_tile_unwritten}
    if case["kind"] == "gateup":
        m["gate and up halves swapped"] = op_gate_up_swapped
    return m


# --- module level ---------------------------------------------------------------------

H_MOD, I_MOD = 128, 192


def module_bound_terms(K, I):
    return 2.0 ** -8 + I * 2.0 ** -23, K * 2.0 ** -23


def module_eval(x, topw, topi, wgu64, wd64):
    """(y [T, k, H], bound [T, k, H]) in float64: per (token, slot) the
    unweighted expert output and ``(2^-8 + I 2^-23) A + K 2^-23 G``.
    ``wgu64`` [E, 2I, K] / ``wd64`` [E, H, I] are float64 (for quantised
    experts ``q * scale``: the per-channel scale is a factor of every term)."""
    T, k = topi.shape
    E, H, I = wd64.shape
    K = x.shape[1]
    ca, cg = module_bound_terms(K, I)
    xd = f64(x)
    y = torch.zeros(T, k, H, dtype=F64)
    bound = torch.zeros(T, k, H, dtype=F64)
    for j in range(k):
        for e in range(E):
            sel = (topi[:, j] == e).nonzero(as_tuple=True)[0]
            if sel.numel() == 0:
                continue
            xs = xd[sel]
            gu = xs @ wgu64[e].t()
            mgu = xs.abs() @ wgu64[e].abs().t()
            act, mag_act = eo.gateup_from(gu, mgu)
            wda = wd64[e].abs().t()
            y[sel, j] = act @ wd64[e].t()
            bound[sel, j] = ca * (act.abs() @ wda) + cg * (mag_act @ wda)
    return y, bound


def _combine(topw, y):
    return (f64(topw).unsqueeze(-1) * y).sum(1)


def _peaked(T, k, g):
    """Routing weights: 0.9 / 0.1 in random order (k = 2), or one of 0.25,
    0.5, 0.75, 1.0 (k = 1; ``_forward_grouped_hip`` takes any weight)."""
    if k == 1:
        return (torch.randint(1, 5, (T, 1), generator=g).float() / 4.0)
    first = torch.rand(T, generator=g) < 0.5
    w = torch.where(first.unsqueeze(1), torch.tensor([0.9, 0.1]), torch.tensor([0.1, 0.9]))
    return w.float()


def _route_counts(counts, g):
    ex = torch.cat([torch.full((n,), e, dtype=torch.long) for e, n in enumerate(counts)])
    return ex[torch.randperm(ex.numel(), generator=g)].unsqueeze(1)


def _route_pair(T, a, b, g):
    """Every token to experts a and b, in random column order."""
    flip = torch.rand(T, generator=g) < 0.5
    return torch.where(flip.unsqueeze(1), torch.tensor([b, a]), torch.tensor([a, b]))


def _route_random(T, E, g):
    logits = torch.randn(T, E, generator=g) * 2.0
    topw, topi = torch.topk(torch.softmax(logits, -1), 2, -1)
    return topw / topw.sum(-1, keepdim=True), topi


# name -> (E, k, T, what the routing is)
MODULE_CASES = {
    "k1-counts-128-0-129-1": (4, 1, 258),
    "k2-all-to-0-and-3": (4, 2, 257),
    "k2-only-1-and-2": (4, 2, 200),
    "k2-random-E8": (8, 2, 300),
    "k2-random-T33": (4, 2, 33),
}


def module_case(name):
    """x [T, 128] bf16 ~ N(0, 1), w_gate_up [E, 384, 128], w_down [E, 128, 192]
    bf16, topw fp32 [T, k], topi long [T, k]; oracle computed once."""
    def build():
        E, k, T = MODULE_CASES[name]
        g = torch.Generator().manual_seed(9700 + 100 * E + 10 * k + T)
        x = torch.randn(T, H_MOD, generator=g).bfloat16()
        wgu = bf16_weights(E, 2 * I_MOD, H_MOD, g)
        wd = bf16_weights(E, H_MOD, I_MOD, g)
        if name == "k1-counts-128-0-129-1":
            topi, topw = _route_counts([128, 0, 129, 1], g), _peaked(T, 1, g)
        elif name == "k2-all-to-0-and-3":
            topi, topw = _route_pair(T, 0, 3, g), _peaked(T, 2, g)
        elif name == "k2-only-1-and-2":
            topi, topw = _route_pair(T, 1, 2, g), _peaked(T, 2, g)
        else:
            topw, topi = _route_random(T, E, g)
        case = {"name": f"{name} E={E} k={k} T={T}", "E": E, "k": k, "T": T, "x": x,
                "wgu": wgu, "wd": wd, "topw": topw.float().contiguous(),
                "topi": topi.contiguous()}
        case["counts"] = torch.bincount(topi.reshape(-1), minlength=E).tolist()
        case["y"], case["bound_jk"] = module_eval(x, case["topw"], topi, f64(wgu), f64(wd))
        case["e"] = _combine(case["topw"], case["y"])
        case["bound"] = _combine(case["topw"], case["bound_jk"])
        return case

    return _cached(("module", name), build)


def module_oracle_for(case, wgu64, wd64):
    """(e, bound) of the case's input and routing under other (float64)
    weights: the quantised module's ``q * scale``."""
    y, b = module_eval(case["x"], case["topw"], case["topi"], wgu64, wd64)
    return _combine(case["topw"], y), _combine(case["topw"], b)


def check_module(actual, e, bound):
    """``kernel_oracles.check`` with the absolute term already scaled."""
    return check(actual, e, bound, 1.0)


def emulate_module(case):
    """The path's arithmetic: fp32 matmuls and silu, ``act`` and ``y`` rounded
    to bf16, fp32 weighted sum, final bf16 rounding."""
    T, k = case["topi"].shape
    I = case["wd"].shape[2]
    out = torch.zeros(T, case["wd"].shape[1])
    for j in range(k):
        for e in range(case["E"]):
            sel = (case["topi"][:, j] == e).nonzero(as_tuple=True)[0]
            if sel.numel() == 0:
                continue
            gu = case["x"][sel].float() @ case["wgu"][e].float().t()
            act = (_silu32(gu[:, :I]) * gu[:, I:]).bfloat16()
            y = (act.float() @ case["wd"][e].float().t()).bfloat16()
            out[sel] += case["topw"][sel, j].unsqueeze(1) * y.float()
    return out.bfloat16()


# module-level mutants: each returns the mutated [T, H] float64 output

def _sorted_pairs(case):
    """The (token, slot) pairs in the path's sorted order (stable by expert),
    as a list per expert."""
    T, k = case["topi"].shape
    flat = case["topi"].reshape(-1)
    order = torch.argsort(flat, stable=True)
    per = {e: [] for e in range(case["E"])}
    for f in order.tolist():
        per[int(flat[f])].append((f // k, f % k))
    return per


def mod_weights_swapped(case):
    return _combine(case["topw"].flip(1), case["y"])


def mod_one_token_off(case):
    return torch.roll(case["e"], 1, 0)


def mod_row_129_dropped(case):
    e = next(e for e in range(case["E"]) if case["counts"][e] > BM)
    t, j = _sorted_pairs(case)[e][BM]
    out = case["e"].clone()
    out[t] -= float(case["topw"][t, j]) * case["y"][t, j]
    return out


def mod_pad_row_onto_last_token(case):
    """What a scatter through index -1 does: a pad slot's row lands on token
    T - 1. The pad slot here carries its expert's last real row with that
    row's weight (padding that clamps instead of zeroing)."""
    e = max(e for e in range(case["E"]) if case["counts"][e] % BM)
    t, j = _sorted_pairs(case)[e][-1]
    out = case["e"].clone()
    out[-1] += float(case["topw"][t, j]) * case["y"][t, j]
    return out


def mod_previous_experts_weights(case):
    return module_oracle_for(case, f64(torch.roll(case["wgu"], 1, 0)),
                             f64(torch.roll(case["wd"], 1, 0)))[0]


def module_mutants(case):
    m = {"rows scattered one token off": mod_one_token_off,
         "expert e uses expert e-1's weights": mod_previous_experts_weights}
    if case["k"] == 2:
        m["a token's two routing weights swapped"] = mod_weights_swapped
    if any(n > BM for n in case["counts"]):
        m["129th row of an expert dropped"] = mod_row_129_dropped
    if any(n % BM for n in case["counts"]):
        m["pad row added onto the last token"] = mod_pad_row_onto_last_token
    return m
