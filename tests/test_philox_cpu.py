"""CPU: the Philox4x32-10 oracle (tests/philox_oracle.py) that the GPU tests of air_dropout_mask / air_randn compare
against, pinned to the published Random123 known-answer vectors - nothing here touches a GPU."""
import numpy as np
import pytest

import philox_oracle as po

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter words, key words, output words)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def scalar_philox(ctr, key, rounds=10):
    """One block with Python integers: shares nothing with the vectorised helper."""
    c, k = list(ctr), list(key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_known_answer_vectors(ctr, key, want):
    got = po.philox4x32_10_full(*ctr, *key)
    assert got.shape == (1, 4) and got.dtype == np.uint32
    assert tuple(int(w) for w in got[0]) == want, [hex(int(w)) for w in got[0]]
    assert scalar_philox(ctr, key) == want
    # the vectors tell 10 rounds from 9: a reference with a dropped round would not pass them
    assert tuple(int(w) for w in po.philox4x32_10_full(*ctr, *key, rounds=9)[0]) != want


def test_kernel_shaped_entry_point():
    """Counter {lo, hi, 0, 0}, key {seed lo, seed hi}; a batch of quads equals one block at a time."""
    assert tuple(int(w) for w in po.philox4x32_10(0, 0, 0)[0]) == KAT[0][2]
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
    hi = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
    for seed in (0, 7, 2 ** 32 + 5, 2 ** 63 + 11):
        got = po.philox4x32_10(lo, hi, seed)
        for i in range(64):
            want = scalar_philox((int(lo[i]), int(hi[i]), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
            assert tuple(int(w) for w in got[i]) == want, (seed, i)


def test_stream_offsets_carry_into_the_high_counter_word():
    seed = 2 ** 32 + 5
    w = po.words(12, seed, 2 ** 32 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    assert tuple(int(x) for x in w[0:4]) == scalar_philox((0xFFFFFFFF, 0, 0, 0), key)
    assert tuple(int(x) for x in w[4:8]) == scalar_philox((0, 1, 0, 0), key)
    assert tuple(int(x) for x in w[8:12]) == scalar_philox((1, 1, 0, 0), key)
    # element 4q + j is word j of quad q whatever n is: a shorter draw is a prefix of a longer one
    assert np.array_equal(po.words(7, seed, 2 ** 32 - 1), w[:7])
    # the 64-bit counter wraps like the device's uint64_t
    assert tuple(int(x) for x in po.words(8, 0, 2 ** 64 - 1)[4:8]) == KAT[0][2]


def test_dropout_keep_arithmetic():
    # first quad of (seed 0, offset 0) = the first known-answer block: u = word * 2^-32 = .399, .880, .735, .605
    assert [int(w) * 2.0 ** -32 >= 0.7 for w in KAT[0][2]] == [False, True, True, False]
    k = po.dropout_keep(4, 0.7, 0, 0)
    assert k.dtype == np.float32
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(0.7))
    assert k.tolist() == [0.0, float(scale), float(scale), 0.0]
    assert np.array_equal(po.dropout_keep(1025, 0.0, 7, 3), np.ones(1025, np.float32))  # p = 0 keeps everything


@pytest.mark.parametrize("p", [0.3, 0.7, 0.999])
def test_dropout_keep_fraction(p):
    """Guards the reference itself: the kept fraction of 2^16 elements lies within 3 sigma of 1 - p."""
    n = 1 << 16
    k = po.dropout_keep(n, p, 12345, 17)
    q = 1.0 - float(np.float32(p))
    kept = np.count_nonzero(k)
    assert abs(kept - n * q) <= 3.0 * np.sqrt(n * q * (1.0 - q)), (kept, n * q)
    assert set(np.unique(k).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}


def test_randn_ref_layout_and_moments():
    n = 1 << 16
    z = po.randn_ref(n, 99, 5, 1.0)
    assert z.dtype == np.float64 and z.shape == (n,)
    assert abs(z.mean()) <= 4.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)
    # per quad [r0 cos0, r0 sin0, r1 cos1, r1 sin1] from words (0, 1) and (2, 3), written out for one quad
    w = [int(x) for x in po.words(4, 99, 5)]
    f32 = np.float32
    for h in range(2):
        u1 = (f32(w[2 * h]) + f32(1.0)) * f32(2.0 ** -32)
        arg = float(f32(6.283185307179586) * (f32(w[2 * h + 1]) * f32(2.0 ** -32)))
        r = np.sqrt(-2.0 * np.log(float(u1)))
        assert abs(z[2 * h] - r * np.cos(arg)) <= 1e-14 and abs(z[2 * h + 1] - r * np.sin(arg)) <= 1e-14
    assert np.array_equal(po.randn_ref(7, 99, 5, 1e-5), float(f32(1e-5)) * z[:7])
    assert np.all(np.isfinite(po.randn_ref(4096, 2 ** 63 + 11, 2 ** 32 - 1, 1.0)))
