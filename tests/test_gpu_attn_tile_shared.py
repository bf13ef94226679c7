"""The packed and the paged prefill kernel run the same MFMA tile core
(``attn_mfma.h``): with a bf16 cache, no cached prefix, no key splits and the
default tile packing they walk the same 64-key rounds from key 0 with the same
per-wave arithmetic, so ``ops.attn_prefill_paged`` equals
``ops.attn_prefill_varlen`` bit for bit. (How many q-tiles share a workgroup
differs, which only moves the bound of the keys a round stages; the keys past a
wave's own rows are masked in both.) A change to the core that reaches only
one of the two kernels shows here.

The cases are ``paged_prefill_cases.make_case`` with ``start = 0``: the same q
goes to both kernels, and the packed K/V are the cache rows read back through
the case's shuffled block table.

Run on an MI355X box: python -m pytest tests/test_gpu_attn_tile_shared.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from kllms_amd import ops

import paged_prefill_cases as pc

DEV = "cuda:0"
BS = 16
# the q-tile (32 rows), the 64-key round and the workgroup (8 tiles) edges
SEQLENS = [[1], [33], [64], [65], [257], [33, 1, 64, 257]]


def packed_kv(case):
    """K and V [T, KVH, D] of the case's tokens, gathered from its cache."""
    ks, vs = [], []
    for blocks, n in zip(case["block_lists"], case["lens"]):
        idx = torch.tensor(blocks)
        for src, dst in ((case["kc"], ks), (case["vc"], vs)):
            rows = src[idx].permute(0, 2, 1, 3).reshape(len(blocks) * BS, case["KVH"], pc.D)
            dst.append(rows[:n])
    return torch.cat(ks).contiguous(), torch.cat(vs).contiguous()


@pytest.mark.parametrize("H,KVH", [(8, 2), (4, 4)], ids=["H8KVH2", "H4KVH4"])
@pytest.mark.parametrize("lens", SEQLENS, ids=lambda lens: "_".join(map(str, lens)))
def test_paged_equals_packed_bitwise(lens, H, KVH):
    case = pc.make_case([(0, n) for n in lens], H, KVH, BS, False)
    table = case["bt"].long()
    flat = [b for blocks in case["block_lists"] for b in blocks]
    assert len(flat) < 4 or flat != sorted(flat), "the block table must be shuffled"
    assert all(table[s, : len(b)].tolist() == b for s, b in enumerate(case["block_lists"]))
    T = sum(lens)
    q = case["fused"].to(DEV)[:, : H * pc.D].view(T, H, pc.D)
    k, v = (t.to(DEV) for t in packed_kv(case))
    cu = torch.tensor(case["cu"], dtype=torch.int32, device=DEV)
    packed = ops.attn_prefill_varlen(q, k, v, cu, case["scale"])
    meta = ops.build_paged_prefill(case["lens"], case["starts"], case["block_lists"], DEV, BS)
    assert not meta.has_splits
    paged = ops.attn_prefill_paged(q, case["kc"].to(DEV), case["vc"].to(DEV), meta, case["scale"])
    torch.cuda.synchronize()
    diff = (paged != packed).any(dim=-1).nonzero().tolist()
    assert torch.equal(paged, packed), f"(token, head) that differ: {diff[:8]} of {len(diff)}"
