"""Cases for the fused RoPE + KV-store op, assembled from the cached
``kernel_oracles.rope_case`` (fused QKV buffer, positions that differ from the
row index, cos/sin table) and ``kernel_oracles.store_case`` (shuffled,
non-contiguous slots and junk-filled caches) of the same shape. Nothing of a
cached case is modified: the fp8 zero rows go into a copy."""

import torch

import kernel_oracles as ko

HEADS = [(1, 1), (4, 2), (32, 8)]
# (Dh, H, KVH, T, BS): every head_dim x heads x block_size at T = 50, T = 1 for
# every head_dim x heads, and T = 4100 (more rows than any capped grid) over
# both head dims, all three head counts and both block sizes
SHAPES = ([(Dh, H, KVH, 50, BS) for Dh in (64, 128) for H, KVH in HEADS for BS in (16, 32)]
          + [(Dh, H, KVH, 1, 16) for Dh in (64, 128) for H, KVH in HEADS]
          + [(64, 1, 1, 4100, 16), (128, 4, 2, 4100, 32), (128, 32, 8, 4100, 16),
             (64, 32, 8, 4100, 32)])
CPU_SHAPES = [s for s in SHAPES if s[3] <= 50] + [(64, 1, 1, 4100, 16)]


def build(Dh, H, KVH, T, BS, fp8):
    r = ko.rope_case(Dh, H, KVH, T)
    s = ko.store_case(Dh, BS, T, KVH_=KVH, fp8=fp8, zero_row=fp8)
    fused = r["fused"].clone()
    if T > 1:
        assert not torch.equal(r["pos"], torch.arange(T)), "positions must differ from the row index"
    _, k, v = ko.qkv_views(fused, H, KVH, Dh)
    zero = None
    if fp8:
        zero = T // 2
        k[zero, 0] = 0
        v[zero, KVH - 1] = 0
    case = {"name": f"D={Dh} H={H} KVH={KVH} T={T} BS={BS}" + (" fp8" if fp8 else ""),
            "fused": fused, "pos": r["pos"], "cs": r["cs"], "slots": s["slots"],
            "kc": s["kc"], "vc": s["vc"], "ks": s.get("ks"), "vs": s.get("vs"),
            "H": H, "KVH": KVH, "D": Dh, "BS": BS, "T": T, "zero": zero, "fp8": fp8}
    return case


def ids(shape):
    return "D{}-H{}-KVH{}-T{}-BS{}".format(*shape)
