"""ops.rope_store_kv dispatch on the CPU: the fused op is torch_ref.rope_inplace
followed by torch_ref.store_kv, on strided views of one fused QKV buffer."""

import pytest
import torch

from kllms_amd import ops
from kllms_amd.ops import torch_ref

import kernel_oracles as ko
import rope_store_cases as rs


def _clone(c):
    caches = [c["kc"].clone(), c["vc"].clone()]
    scales = [c["ks"].clone(), c["vs"].clone()] if c["fp8"] else [None, None]
    return c["fused"].clone(), caches, scales


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("shape", rs.CPU_SHAPES, ids=rs.ids)
def test_cpu_dispatch_equals_the_two_refs(shape, fp8):
    c = rs.build(*shape, fp8)
    H, KVH, D = c["H"], c["KVH"], c["D"]

    fa, (kca, vca), (ksa, vsa) = _clone(c)
    q, k, v = ko.qkv_views(fa, H, KVH, D)
    assert c["T"] == 1 or not k.is_contiguous()
    torch_ref.rope_inplace(q, k, c["pos"], c["cs"])
    torch_ref.store_kv(k, v, kca, vca, c["slots"], ksa, vsa)

    fb, (kcb, vcb), (ksb, vsb) = _clone(c)
    q, k, v = ko.qkv_views(fb, H, KVH, D)
    ops.rope_store_kv(q, k, v, c["pos"], c["cs"], kcb, vcb, c["slots"], ksb, vsb)

    assert torch.equal(fa, fb)
    assert not torch.equal(fb, c["fused"])
    for a, b in ((kca, kcb), (vca, vcb)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    if fp8:
        assert torch.equal(ksa, ksb) and torch.equal(vsa, vsb)
        assert not torch.equal(ksb, c["ks"])
