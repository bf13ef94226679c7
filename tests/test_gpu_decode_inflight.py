"""Per-stream decode attention at the load-group edges of
``attn_decode_partial_t``: ``ops.attn_decode_paged`` against the float64
oracle ``kernel_oracles.attn_decode``, held to the ``C_FP32`` bound of
``kernel_oracles`` (not widened), on the cases of ``decode_inflight_cases``
(waves with no key, one key, exactly one group of in-flight V rows, a group
plus one key, a clamped last group, inside the first to fourth chunk).
``test_decode_inflight_cases.py`` shows on the CPU that the bound accepts the
reference and rejects a dropped or an extra key on the same cases.

Run on an MI355X box: python -m pytest tests/test_gpu_decode_inflight.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import decode_inflight_cases as dic
import kernel_oracles as ko

DEV = "cuda:0"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("gqa,BS", dic.SHAPES)
def test_decode_inflight(gqa, BS, fp8):
    case = dic.inflight_case(gqa, BS, fp8)
    e, a = dic.oracle(case)
    d = {k: v.to(DEV) for k, v in case.items() if isinstance(v, torch.Tensor)}
    B, H, D = case["q"].shape
    q = d["fused"][:, : H * D].view(B, H, D)
    assert q.stride(0) == d["fused"].shape[1] and not q.is_contiguous()
    out = ops.attn_decode_paged(q, d["kc"], d["vc"], d["bt"], d["lens"], case["scale"],
                                d.get("ks"), d.get("vs"))
    ratio, idx = ko.check(out, e, a, ko.C_FP32)
    msg = ko.describe("attn_decode", case["name"], ratio, idx, ("row", "head", "dim"),
                      f", ctx={dic.CTX[idx[0]]}")
    print("RATIO " + msg)
    assert ratio <= 1.0, msg
