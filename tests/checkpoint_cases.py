"""Inputs of the map checkpoint tests (test_checkpoint_abi.py, test_gpu_checkpoint.py): maps of random bit patterns, and the vertex table
written out by hand."""
import numpy as np


def values(P, M, seed):
    """A map of P rows as arrays, filled with random BIT PATTERNS (NaNs with payloads, infinities, -0 and denormals among them)."""
    rng = np.random.default_rng(seed)
    bits = lambda *shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v = dict(xyz=bits(P, 3), shs=bits(P, M, 3), opacity_raw=bits(P, 1), scaling_raw=bits(P, 3), rotation_raw=bits(P, 4), confidence=bits(P, 1))
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], np.uint32).view(np.float32)
    for a in v.values():
        flat = a.reshape(-1)
        flat[rng.integers(0, flat.size, size=min(flat.size, 8))] = special[:min(flat.size, 8)]
    return v


def hand_table(v, include_confidence):
    """The vertex table written out column by column, in the order of construct_list_of_attributes."""
    P, M = v["shs"].shape[:2]
    C = 6 + 3 * M + 8 + (1 if include_confidence else 0)
    t = np.zeros((P, C), np.uint32)
    u = lambda a: a.view(np.uint32)
    t[:, 0:3] = u(v["xyz"])
    t[:, 6:9] = u(v["shs"])[:, 0, :]
    for ch in range(3):
        for k in range(1, M):
            t[:, 9 + ch * (M - 1) + (k - 1)] = u(v["shs"])[:, k, ch]
    o = 9 + 3 * (M - 1)
    t[:, o] = u(v["opacity_raw"])[:, 0]
    t[:, o + 1:o + 4] = u(v["scaling_raw"])
    t[:, o + 4:o + 8] = u(v["rotation_raw"])
    if include_confidence:
        t[:, o + 8] = u(v["confidence"])[:, 0]
    return t.view(np.float32)
