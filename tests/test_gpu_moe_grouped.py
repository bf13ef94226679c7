"""The bf16 grouped MoE kernels (``moe_gateup`` / ``moe_down``, the default
Mixtral prefill path) and ``MixtralMoE._forward_grouped_hip`` against the
float64 oracles of ``moe_oracles`` under their derived bounds.

Run on an MI355X box: python -m pytest tests/test_gpu_moe_grouped.py -m gpu -q

Each test prints its worst error/bound ratio and the row / column / expert of
the worst element before asserting ``<= 1.0``.
"""

import bisect

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import moe_oracles as mo
from kllms_amd import ops

DEV = "cuda:0"
GUARD = 4096
SENTINEL = -777.0


def _pad():
    return torch.tensor(mo.PAD_OFFSETS, dtype=torch.int32, device=DEV)


def _run_gateup(case, act, fp8=False):
    K = case["K"]
    zeros = torch.zeros(K, dtype=torch.bfloat16, device=DEV)
    if fp8:
        ops.moe_gateup(act, case["x"].to(DEV), case["q"].to(DEV), case["sorted_ids"].to(DEV),
                       _pad(), zeros, scale=case["scale"].to(DEV))
    else:
        ops.moe_gateup(act, case["x"].to(DEV), case["w"].to(DEV), case["sorted_ids"].to(DEV),
                       _pad(), zeros)
    return act


def _run_down(case, y, fp8=False):
    if fp8:
        ops.moe_down(y, case["act"].to(DEV), case["q"].to(DEV), _pad(), scale=case["scale"].to(DEV))
    else:
        ops.moe_down(y, case["act"].to(DEV), case["w"].to(DEV), _pad())
    return y


def _run(case, out, fp8=False):
    return (_run_gateup if case["kind"] == "gateup" else _run_down)(case, out, fp8)


def _prefilled():
    return torch.full((mo.S_OP, mo.N_OP), mo.PREFILL, dtype=torch.bfloat16, device=DEV)


def _report_op(what, case, out):
    ratio, (row, col) = mo.check(out, case["e"], case["mag"], mo.c_kernel(case["K"]))
    expert = bisect.bisect_right(mo.PAD_OFFSETS, row) - 1
    print(f"{what} [{case['name']}]: worst error/bound {ratio:.3f} at row {row}, column {col}, "
          f"expert {expert}")
    assert ratio <= 1.0, (case["name"], ratio, row, col, expert)
    return ratio


def _case(kind, depth, exact=False):
    return mo.gateup_case(depth, exact) if kind == "gateup" else mo.down_case(depth, exact)


# --- op level ---------------------------------------------------------------------------

@pytest.mark.parametrize("K", mo.OP_DEPTHS)
def test_moe_gateup_within_bound(K):
    case = mo.gateup_case(K)
    act = _run_gateup(case, _prefilled())
    _report_op("bf16 moe_gateup", case, act)
    assert (act[case["sorted_ids"].to(DEV) < 0] == 0).all(), "pad rows are not exactly zero"


@pytest.mark.parametrize("IN", mo.OP_DEPTHS)
def test_moe_down_within_bound(IN):
    case = mo.down_case(IN)
    _report_op("bf16 moe_down", case, _run_down(case, _prefilled()))


@pytest.mark.parametrize("depth", [64, 192])
@pytest.mark.parametrize("kind", ["gateup", "down"])
def test_nothing_written_outside(kind, depth):
    case = _case(kind, depth)
    n = mo.S_OP * mo.N_OP
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[GUARD:GUARD + n].view(mo.S_OP, mo.N_OP)
    _run(case, out)
    torch.cuda.synchronize()
    assert (buf[:GUARD] == SENTINEL).all(), "elements before the output were written"
    assert (buf[GUARD + n:] == SENTINEL).all(), "elements after the output were written"
    _report_op(f"bf16 moe_{kind} in a guarded buffer", case, out)


@pytest.mark.parametrize("kind", ["gateup", "down"])
def test_bf16_and_fp8_instantiations_agree_bit_for_bit(kind):
    """e4m3-representable bf16 weights against the same values as e4m3 with
    unit scales: the LDS tile and the MFMA loop are shared, the fp8 epilogue
    multiplies by 1.0f."""
    case = _case(kind, 192, exact=True)
    a = _run(case, _prefilled())
    b = _run(case, _prefilled(), fp8=True)
    _report_op(f"bf16 moe_{kind}", case, a)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("kind", ["gateup", "down"])
def test_deterministic(kind):
    case = _case(kind, 1088)
    a = _run(case, _prefilled())
    b = _run(case, torch.zeros_like(a))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# --- module level -------------------------------------------------------------------------

def _moe(case):
    from kllms_amd.engine.config import ModelArchConfig
    from kllms_amd.models.mixtral import MixtralMoE
    from kllms_amd.parallel.tp import ParallelContext

    cfg = ModelArchConfig(arch="mixtral", vocab_size=512, hidden_size=mo.H_MOD,
                          intermediate_size=mo.I_MOD, num_layers=1, num_heads=4,
                          num_kv_heads=2, num_experts=case["E"], num_experts_per_tok=case["k"])
    moe = MixtralMoE(cfg, ParallelContext(), torch.bfloat16).to(DEV)
    with torch.no_grad():
        moe.w_gate_up.copy_(case["wgu"])
        moe.w_down.copy_(case["wd"])
    return moe


def _report_module(what, case, out, e, bound):
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == tuple(e.shape)
    ratio, (tok, col) = mo.check_module(out, e, bound)
    experts = case["topi"][tok].tolist()
    print(f"{what} [{case['name']}]: worst error/bound {ratio:.3f} at token {tok}, column {col}, "
          f"experts {experts} (weights {case['topw'][tok].tolist()})")
    assert ratio <= 1.0, (case["name"], ratio, tok, col, experts)


@pytest.mark.parametrize("name", list(mo.MODULE_CASES))
def test_forward_grouped_hip_within_bound(name):
    case = mo.module_case(name)
    moe = _moe(case)
    out = moe._forward_grouped_hip(case["x"].to(DEV), case["topw"].to(DEV), case["topi"].to(DEV))
    _report_module("_forward_grouped_hip bf16", case, out, case["e"], case["bound"])


def test_forward_grouped_hip_quantised_within_bound():
    """The quantised module against the oracle of its own e4m3 weights and
    scales (``q * scale`` in float64), under the same bound."""
    case = mo.module_case("k2-random-E8")
    moe = _moe(case)
    moe.quantize_fp8_()
    assert moe.quantized and moe.w_down_q.dtype == torch.float8_e4m3fn
    wgu64 = mo.f64(moe.w_gate_up_q.cpu()) * mo.f64(moe.w_gate_up_scale.cpu()).unsqueeze(-1)
    wd64 = mo.f64(moe.w_down_q.cpu()) * mo.f64(moe.w_down_scale.cpu()).unsqueeze(-1)
    e, bound = mo.module_oracle_for(case, wgu64, wd64)
    out = moe._forward_grouped_hip(case["x"].to(DEV), case["topw"].to(DEV), case["topi"].to(DEV))
    _report_module("_forward_grouped_hip fp8 experts", case, out, e, bound)


# --- the bindings refuse on the host what would write out of bounds ----------------------

def _gateup_args():
    case = mo.gateup_case(64)
    return {"act": torch.zeros(mo.S_OP, mo.N_OP, dtype=torch.bfloat16, device=DEV),
            "x": case["x"].to(DEV), "w": case["w"].to(DEV),
            "sorted_ids": case["sorted_ids"].to(DEV), "pad_offsets": _pad(),
            "zeros": torch.zeros(64, dtype=torch.bfloat16, device=DEV)}


def _down_args():
    case = mo.down_case(64)
    return {"y": torch.zeros(mo.S_OP, mo.N_OP, dtype=torch.bfloat16, device=DEV),
            "act": case["act"].to(DEV), "w": case["w"].to(DEV), "pad_offsets": _pad()}


def _call_gateup(a):
    ops.moe_gateup(a["act"], a["x"], a["w"], a["sorted_ids"], a["pad_offsets"], a["zeros"])


def _call_down(a):
    ops.moe_down(a["y"], a["act"], a["w"], a["pad_offsets"])


def _wide_x(a):
    wide = torch.zeros(mo.T_OP, 64 + 24, dtype=torch.bfloat16, device=DEV)
    return wide[:, :64]


GATEUP_REFUSALS = {
    "sorted_ids one short": {"sorted_ids": lambda a: a["sorted_ids"][:-1].contiguous()},
    "sorted_ids one tile long": {"sorted_ids": lambda a: torch.cat([a["sorted_ids"]] * 2)[:mo.S_OP + 128]},
    "sorted_ids 2-D": {"sorted_ids": lambda a: a["sorted_ids"].view(4, -1)},
    "sorted_ids on the CPU": {"sorted_ids": lambda a: a["sorted_ids"].cpu()},
    "sorted_ids int64": {"sorted_ids": lambda a: a["sorted_ids"].long()},
    "pad_offsets 2-D": {"pad_offsets": lambda a: a["pad_offsets"].view(1, -1)},
    "pad_offsets on the CPU": {"pad_offsets": lambda a: a["pad_offsets"].cpu()},
    "x 1-D": {"x": lambda a: a["x"].reshape(-1)},
    "x 3-D": {"x": lambda a: a["x"].unsqueeze(0)},
    "x on the CPU": {"x": lambda a: a["x"].cpu()},
    "x not contiguous": {"x": _wide_x},
    "w 2-D": {"w": lambda a: a["w"][0]},
    "w on the CPU": {"w": lambda a: a["w"].cpu()},
    "act rows not a multiple of 128": {"act": lambda a: a["act"][:500], "sorted_ids": lambda a: a["sorted_ids"][:500].contiguous()},
    "act 1-D": {"act": lambda a: a["act"].reshape(-1)},
}

DOWN_REFUSALS = {
    "y one tile longer than act": {"y": lambda a: torch.zeros(mo.S_OP + 128, mo.N_OP, dtype=torch.bfloat16, device=DEV)},
    "y one tile shorter than act": {"y": lambda a: a["y"][:mo.S_OP - 128]},
    "rows not a multiple of 128": {"y": lambda a: a["y"][:500], "act": lambda a: a["act"][:500]},
    "y 1-D": {"y": lambda a: a["y"].reshape(-1)},
    "act 3-D": {"act": lambda a: a["act"].unsqueeze(0)},
    "act on the CPU": {"act": lambda a: a["act"].cpu()},
    "w 2-D": {"w": lambda a: a["w"][0]},
    "w on the CPU": {"w": lambda a: a["w"].cpu()},
    "pad_offsets 2-D": {"pad_offsets": lambda a: a["pad_offsets"].view(1, -1)},
    "pad_offsets on the CPU": {"pad_offsets": lambda a: a["pad_offsets"].cpu()},
    "pad_offsets int64": {"pad_offsets": lambda a: a["pad_offsets"].long()},
}


def _refused(args, call, edits):
    """No kernel is launched: the output keeps its sentinel."""
    out_key = "act" if "zeros" in args else "y"
    args[out_key].fill_(SENTINEL)
    out = args[out_key]
    for key, fn in edits.items():
        args[key] = fn(args)
    with pytest.raises(RuntimeError):
        call(args)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("what", list(GATEUP_REFUSALS))
def test_moe_gateup_binding_refuses(what):
    _refused(_gateup_args(), _call_gateup, GATEUP_REFUSALS[what])


@pytest.mark.parametrize("what", list(DOWN_REFUSALS))
def test_moe_down_binding_refuses(what):
    _refused(_down_args(), _call_down, DOWN_REFUSALS[what])


def test_bindings_accept_the_unedited_arguments():
    """The refusal tests start from arguments that the bindings take."""
    g, d = _gateup_args(), _down_args()
    _call_gateup(g)
    _call_down(d)
    _report_op("bf16 moe_gateup", mo.gateup_case(64), g["act"])
    _report_op("bf16 moe_down", mo.down_case(64), d["y"])
