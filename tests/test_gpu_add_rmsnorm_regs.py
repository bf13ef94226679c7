"""fused_add_rmsnorm with the summed row kept in registers (n <= 8192) and the
read-back fallback above it: both sides of the limit, a vector tail (n = 2056,
8200: the last vectors of a pass are owned by a few threads only), one and many
rows. Output against ``kernel_oracles.fused_add_rmsnorm`` with the bound of the
existing rmsnorm test (C_ELEM); the residual written back must be bit-equal.

Run on an MI355X box: python -m pytest tests/test_gpu_add_rmsnorm_regs.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import kernel_oracles as ko

DEV = "cuda:0"


@pytest.mark.parametrize("n", [8, 2048, 2056, 4096, 8192, 8200, 16384])
@pytest.mark.parametrize("rows", [1, 3, 128])
def test_fused_add_rmsnorm(rows, n):
    c = ko.rmsnorm_case(rows, n)
    want_res, e, t = ko.fused_add_rmsnorm(c["xr"], c["r"], c["w"], ko.EPS)
    x, w = c["xr"].to(DEV), c["w"].to(DEV)
    res = c["r"].to(DEV).clone()
    out, res2 = ops.fused_add_rmsnorm(x, res, w, ko.EPS)
    assert res2 is res
    assert torch.equal(x.cpu(), c["xr"]), "the input x changed"
    assert torch.equal(res.cpu(), want_res), f"residual not bit-equal [{c['name']}]"
    ratio, idx = ko.check(out, e, t, ko.C_ELEM)
    msg = ko.describe("fused_add_rmsnorm", c["name"], ratio, idx, ("row", "col"))
    print("RATIO " + msg)
    assert ratio <= 1.0, msg
    if c["zero_row"] is not None:
        z = c["zero_row"]
        assert not out[z].float().any() and not res[z].float().any()
