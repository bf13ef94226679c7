"""The bf16 grouped-MoE oracles test the kernels; this module (CPU) tests the
oracles: an emulation of the kernels' arithmetic is accepted on every case,
every mutant listed for a case exceeds the bound on it, and the CPU
``_forward_grouped`` in bf16 is measured against the module-level bound.
"""

import math

import pytest
import torch

import moe_oracles as mo

OP_IDS = [f"{kind}-{d}" for kind in ("gateup", "down") for d in mo.OP_DEPTHS]


def _op_case(cid):
    kind, d = cid.split("-")
    return mo.gateup_case(int(d)) if kind == "gateup" else mo.down_case(int(d))


def test_op_layout_is_what_the_cases_claim():
    assert mo.PAD_OFFSETS[0] == 0 and len(mo.PAD_OFFSETS) == mo.E_OP + 1
    for e, n in enumerate(mo.COUNTS):
        assert mo.PAD_OFFSETS[e + 1] - mo.PAD_OFFSETS[e] == (n + mo.BM - 1) // mo.BM * mo.BM
    ids = mo.gateup_case(64)["sorted_ids"]
    for e, n in enumerate(mo.COUNTS):
        lo, hi = mo.PAD_OFFSETS[e], mo.PAD_OFFSETS[e + 1]
        assert (ids[lo:lo + n] >= 0).all() and (ids[lo:lo + n] < mo.T_OP).all()
        assert (ids[lo + n:hi] == -1).all()
    assert int((ids >= 0).sum()) == sum(mo.COUNTS) > mo.T_OP      # tokens repeat


@pytest.mark.parametrize("cid", OP_IDS)
def test_op_emulation_within_bound(cid):
    case = _op_case(cid)
    out = mo.emulate_op(case)
    ratio, idx = mo.check(out, case["e"], case["mag"], mo.c_kernel(case["K"]))
    print(f"emulation [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (case["name"], ratio, idx)
    if case["kind"] == "gateup":
        assert (out[case["sorted_ids"] < 0] == 0).all()


@pytest.mark.parametrize("cid", OP_IDS)
def test_op_mutants_exceed_bound(cid):
    case = _op_case(cid)
    muts = mo.op_mutants(case)
    assert len(muts) == (5 if case["kind"] == "gateup" else 4)
    for name, fn in muts.items():
        bad = fn(case).float().bfloat16()
        ratio, _ = mo.check(bad, case["e"], case["mag"], mo.c_kernel(case["K"]))
        print(f"mutant '{name}' [{case['name']}]: error/bound {ratio:.1f}")
        assert ratio > 1.0, f"bound has no teeth against '{name}' on {case['name']}: {ratio}"


@pytest.mark.parametrize("kind", ["gateup", "down"])
def test_e4m3_exact_weights_are_exact(kind):
    case = mo.gateup_case(192, True) if kind == "gateup" else mo.down_case(192, True)
    assert torch.equal(case["w"].float(), case["q"].float())
    assert (case["scale"] == 1.0).all()
    ratio, _ = mo.check(mo.emulate_op(case), case["e"], case["mag"], mo.c_kernel(192))
    assert ratio <= 1.0


def test_module_cases_route_as_described():
    want = {"k1-counts-128-0-129-1": [128, 0, 129, 1], "k2-all-to-0-and-3": [257, 0, 0, 257],
            "k2-only-1-and-2": [0, 200, 200, 0]}
    for name in mo.MODULE_CASES:
        case = mo.module_case(name)
        E, k, T = mo.MODULE_CASES[name]
        assert case["topi"].shape == (T, k) and case["topw"].shape == (T, k)
        assert T > 8 * E, "forward() would take the dense path"
        if name in want:
            assert case["counts"] == want[name]
        if k == 2:
            assert (case["topi"][:, 0] != case["topi"][:, 1]).all()
            assert torch.allclose(case["topw"].sum(1), torch.ones(T))
    assert mo.MODULE_CASES["k2-random-T33"][2] == 8 * 4 + 1
    assert all(n <= mo.BM for n in mo.module_case("k2-random-T33")["counts"])


@pytest.mark.parametrize("name", list(mo.MODULE_CASES))
def test_module_emulation_within_bound(name):
    case = mo.module_case(name)
    ratio, idx = mo.check_module(mo.emulate_module(case), case["e"], case["bound"])
    print(f"module emulation [{case['name']}]: worst error/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (case["name"], ratio, idx)


@pytest.mark.parametrize("name", list(mo.MODULE_CASES))
def test_module_mutants_exceed_bound(name):
    case = mo.module_case(name)
    muts = mo.module_mutants(case)
    assert len(muts) >= 3
    for mname, fn in muts.items():
        bad = fn(case).float().bfloat16()
        ratio, _ = mo.check_module(bad, case["e"], case["bound"])
        print(f"module mutant '{mname}' [{case['name']}]: error/bound {ratio:.1f}")
        assert ratio > 1.0, f"bound has no teeth against '{mname}' on {case['name']}: {ratio}"


def test_every_module_mutant_is_listed_somewhere():
    listed = set()
    for name in mo.MODULE_CASES:
        listed |= set(mo.module_mutants(mo.module_case(name)))
    assert len(listed) == 5, listed


@pytest.mark.parametrize("name", list(mo.MODULE_CASES))
def test_cpu_forward_grouped_measured_against_the_bound(name):
    """Where the old reference lands: ``_forward_grouped`` on the CPU in bf16
    rounds the gate_up product to bf16 before silu_mul, casts the routing
    weights to bf16 and accumulates ``index_add_`` in bf16. Measured and
    printed, not required to pass (tests/README.md records the figures)."""
    from kllms_amd.engine.config import ModelArchConfig
    from kllms_amd.models.mixtral import MixtralMoE
    from kllms_amd.parallel.tp import ParallelContext

    case = mo.module_case(name)
    cfg = ModelArchConfig(arch="mixtral", vocab_size=512, hidden_size=mo.H_MOD,
                          intermediate_size=mo.I_MOD, num_layers=1, num_heads=4,
                          num_kv_heads=2, num_experts=case["E"], num_experts_per_tok=case["k"])
    moe = MixtralMoE(cfg, ParallelContext(), torch.bfloat16)
    with torch.no_grad():
        moe.w_gate_up.copy_(case["wgu"])
        moe.w_down.copy_(case["wd"])
    out = moe._forward_grouped(case["x"], case["topw"], case["topi"])
    ratio, idx = mo.check_module(out, case["e"], case["bound"])
    print(f"CPU _forward_grouped bf16 [{case['name']}]: error/bound {ratio:.2f} at {idx}")
    assert out.shape == case["e"].shape and math.isfinite(ratio)
