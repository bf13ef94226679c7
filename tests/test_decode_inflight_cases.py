"""Tests of ``test_gpu_decode_inflight.py``'s cases (CPU): on the load-group
edge cases of ``decode_inflight_cases`` the float64 oracle and the ``C_FP32``
bound must ACCEPT the CPU path of ``ops.attn_decode_paged`` (``torch_ref``,
fp32 rounded to bf16) and REJECT the defects a mis-clamped or mis-guarded load
group would produce: the last key dropped, one key past the context read, the
tail block dropped, the q stride ignored.
"""

import pytest
import torch

import decode_inflight_cases as dic
import kernel_oracles as ko
from kllms_amd import ops


def test_cases_have_the_promised_layout():
    for case in dic.all_cases():
        BS = case["kc"].shape[2]
        need = max((c + BS - 1) // BS for c in dic.CTX)
        assert case["bt"].shape == (len(dic.CTX), need + 2)
        assert case["lens"].tolist() == dic.CTX
        assert not case["q"].is_contiguous()
        used = [int(x) for b, c in enumerate(dic.CTX)
                for x in case["bt"][b, : (c + BS - 1) // BS]]
        assert len(set(used)) == len(used), "block tables overlap"
        for b, c in enumerate(dic.CTX):
            # the slot after the last key and the next table entry hold junk
            blk = int(case["bt"][b, c // BS])
            assert float(case["vc"][blk, 0, c % BS, 0].float()) != 0.0
            if "ks" not in case:
                assert float(case["vc"][blk, 0, c % BS, 0]) == dic.JUNK


def test_cpu_path_accepted():
    worst = 0.0
    for case in dic.all_cases():
        e, a = dic.oracle(case)
        out = ops.attn_decode_paged(case["q"], case["kc"], case["vc"], case["bt"], case["lens"],
                                    case["scale"], case.get("ks"), case.get("vs"))
        ratio, idx = ko.check(out, e, a, ko.C_FP32)
        assert ratio <= 1.0, ko.describe("torch_ref decode", case["name"], ratio, idx,
                                         ("row", "head", "dim"), f", ctx={dic.CTX[idx[0]]}")
        worst = max(worst, ratio)
    print(f"torch_ref decode worst ratio {worst:.3f}")


@pytest.mark.parametrize("name", list(dic.MUTANTS))
def test_mutant_rejected(name):
    applied = 0
    weakest = float("inf")
    for case in dic.all_cases():
        out = dic.MUTANTS[name](case)
        assert out is not None, f"mutant '{name}' does not apply to {case['name']}"
        e, a = dic.oracle(case)
        assert not torch.equal(out, e)
        applied += 1
        ratio, _ = ko.check(out.float().bfloat16(), e, a, ko.C_FP32)
        assert ratio > 1.0, f"mutant '{name}' passes on {case['name']}: ratio {ratio:.3f}"
        weakest = min(weakest, ratio)
    assert applied == len(dic.all_cases())
    print(f"mutant '{name}': {applied} cases, weakest ratio {weakest:.2f}")
