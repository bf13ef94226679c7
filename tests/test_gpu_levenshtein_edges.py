"""The batched Levenshtein kernel at the edges of its 64-bit word, through its
swap branch both ways, with non-zero padding, and past its grid cap.

Run on an MI355X box: python -m pytest tests/test_gpu_levenshtein_edges.py -m gpu -q
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import levenshtein_cases as lc
from kllms_amd import ops

DEV = "cuda:0"
GRID_CAP = 2048 * 256


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _packed():
    chars, lens = lc.packed()
    return chars.to(DEV), lens.to(DEV)


def test_every_pair_equals_the_dp():
    chars, lens = _packed()
    pairs = lc.pairs()
    out = ops.levenshtein_pairs(chars, lens, _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs]))
    assert out.dtype == torch.int32 and out.shape == (len(pairs),)
    got, exp, s = out.cpu().tolist(), lc.expected(), lc.strings()
    bad = [(s[i], s[j], g, exp[(i, j)]) for (i, j), g in zip(pairs, got) if g != exp[(i, j)]]
    print(f"levenshtein_pairs: {len(pairs)} pairs over lengths {lc.LENGTHS}, {len(bad)} wrong")
    assert not bad, bad[:5]


def test_grid_stride_past_the_block_cap():
    """2048 * 256 + 4097 pairs: 4097 threads take a second pair. Pairs drawn
    cyclically from the distinct ones; every element is checked against the
    per-pair table."""
    chars, lens = _packed()
    distinct = lc.distinct_pairs()
    exp = lc.expected()
    table = _i32([exp[p] for p in distinct])
    P = GRID_CAP + 4097
    idx = torch.arange(P, device=DEV) % len(distinct)
    out = ops.levenshtein_pairs(chars, lens, _i32([p[0] for p in distinct])[idx],
                                _i32([p[1] for p in distinct])[idx])
    assert out.shape == (P,)
    wrong = (out != table[idx]).nonzero().flatten()
    print(f"levenshtein_pairs grid-stride: {P} pairs, {wrong.numel()} wrong")
    assert wrong.numel() == 0, (wrong[:5].tolist(), out[wrong[:5]].tolist())


def test_zero_pairs():
    chars, lens = _packed()
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    out = ops.levenshtein_pairs(chars, lens, empty, empty)
    torch.cuda.synchronize()
    assert out.shape == (0,) and out.dtype == torch.int32
