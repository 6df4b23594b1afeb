"""Test infrastructure (numpy only): Philox4x32-10 as the device draws use it (csrc/adv_head.hip ``dropout_body``,
csrc/pool_head.hip ``randn_body``), restated plainly and vectorised over an array of quads.

One quad = one counter value = four uint32 words = four output elements: element ``4q + j`` of a draw comes from word
``j`` of the block at counter ``offset + q`` (64-bit, wrapping), with counter words ``{lo, hi, 0, 0}`` and key words
``{seed lo, seed hi}``.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key schedule's Weyl increments
MASK32 = 0xFFFFFFFF
INV32 = np.float32(2.0 ** -32)
TWO_PI = np.float32(6.283185307179586)


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32_10_full(c0, c1, c2, c3, k0, k1, rounds=10):
    """The generator itself: four counter words and two key words (each an array of uint32 values or a scalar) ->
    (N, 4) uint32.  ``rounds`` is 10 everywhere but in the tests that show a dropped round is noticed."""
    c = [_u64(w) & np.uint64(MASK32) for w in (c0, c1, c2, c3)]
    n = max(w.size for w in c)
    c = [np.broadcast_to(w, (n,)).copy() for w in c]
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    lo = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, axis=1).astype(np.uint32)


def philox4x32_10(ctr_lo, ctr_hi, seed):
    """The kernel-shaped entry point: counter ``{lo, hi, 0, 0}``, key ``{seed lo, seed hi}``."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10_full(ctr_lo, ctr_hi, 0, 0, seed & MASK32, seed >> 32)


def words(n, seed, offset):
    """The first ``n`` uint32 words of the stream (seed, offset): (n,) uint32."""
    quads = (n + 3) // 4
    offset = int(offset) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + np.arange(quads, dtype=np.uint64)  # wraps at 2^64 like the device's uint64_t
    w = philox4x32_10(ctr & np.uint64(MASK32), ctr >> np.uint64(32), seed)
    return w.reshape(-1)[:n]


def dropout_keep(n, p, seed, offset):
    """air_dropout_mask's output, bit for bit: (n,) float32 of 0 and 1/(1-p).  Every step is a single correctly
    rounded float32 operation (uint32 -> float32 conversion rounds to nearest even, as ``astype`` does)."""
    p = np.float32(p)
    u = words(n, seed, offset).astype(np.float32) * INV32
    scale = np.float32(1.0) / (np.float32(1.0) - p)
    return np.where(u >= p, scale, np.float32(0.0)).astype(np.float32)


def randn_ref(n, seed, offset, scale):
    """air_randn's output to fp64: the uniforms and the angle in float32 exactly as the kernel forms them, then
    Box-Muller in float64.  Per quad: [r0 cos0, r0 sin0, r1 cos1, r1 sin1], words 0, 1 feeding the first pair and
    words 2, 3 the second."""
    quads = (n + 3) // 4
    c = words(quads * 4, seed, offset).astype(np.float32).reshape(quads, 2, 2)  # (quad, pair, {radius word, angle word})
    u1 = (c[:, :, 0] + np.float32(1.0)) * INV32  # (0, 1]
    u2 = c[:, :, 1] * INV32
    arg = (TWO_PI * u2).astype(np.float64)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    z = np.stack([r * np.cos(arg), r * np.sin(arg)], axis=2)  # (quad, pair, {cos, sin})
    return (float(np.float32(scale)) * z).reshape(-1)[:n]
