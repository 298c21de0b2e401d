"""Host restatement of the dropout mask of csrc/common.h, in numpy, for the tests.

The header's contract: Philox4x32 (Salmon et al., SC'11) with IQ_PHILOX_ROUNDS = 7 rounds, counter =
(group_lo, group_hi, site, step), key = (seed_lo, seed_hi).  One call decides the 8 consecutive elements
[8 * group, 8 * group + 8) of a row-major tensor: word i holds element 2i in its low 16 bits and element 2i + 1 in
its high 16 bits, and an element is kept iff its 16-bit value >= thresh, thresh = floor(p * 65536 + 0.5) clamped to
[0, 65535], all in fp32.  Kept values are multiplied by 65536 / (65536 - thresh).

Everything is written in uint64 arithmetic masked to 32 bits, so nothing here depends on the device; the round
function is pinned to the published Random123 known-answer vectors by tests/test_dropout_ref_cpu.py.
"""
import numpy as np

ROUNDS = 7                                  # IQ_PHILOX_ROUNDS
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds):
    """counter: (..., 4) and key: (..., 2) (or (2,)) arrays of 32-bit values -> (..., 4) uint64 array of 32-bit words."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0 = _M0 * c0                       # 32 x 32 -> 64 bits: exact in uint64
        p1 = _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n2 = (p0 >> _S32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _MASK, n2, p0 & _MASK
        k0 = (k0 + _W0) & _MASK
        k1 = (k1 + _W1) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def dropout_thresh(p):
    """The header's dropout_thresh: fp32 p * 65536 + 0.5, clamped, truncated."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    t = min(max(t, np.float32(0.0)), np.float32(65535.0))
    return int(t)


def dropout_scale(p):
    """The header's dropout_scale, as the fp32 value the kernels multiply by."""
    return np.float32(65536.0) / (np.float32(65536.0) - np.float32(dropout_thresh(p)))


def keep_groups(seed, step, site, p, groups):
    """Keep flags of the 8-element groups `groups` (any integer array) -> bool array groups.shape + (8,)."""
    g = np.asarray(groups, dtype=np.uint64)
    ctr = np.stack([g & _MASK, g >> _S32, np.full_like(g, np.uint64(site)), np.full_like(g, np.uint64(step))], axis=-1)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    w = philox4x32(ctr, key, ROUNDS)
    u16 = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=-1)       # (..., word, half): element 2 * word + half
    return (u16 >= np.uint64(dropout_thresh(p))).reshape(g.shape + (8,))


def keep_mask(seed, step, site, p, n_elements):
    """Keep flags of elements [0, n_elements) of a row-major tensor -> bool array (n_elements,)."""
    groups = np.arange((n_elements + 7) // 8, dtype=np.uint64)
    return keep_groups(seed, step, site, p, groups).reshape(-1)[:n_elements]
