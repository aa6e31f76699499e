"""Slice 4's C-init of the log2 int8 kernels formed by one 16-bit shift
(i8l_cinit16, nemo_factored_i8.hip), restated in Python integers with the
instructions' own 16- and 32-bit wrap-around.

The two-tile walk needs R = (T_0 & 511) 2^18 + l_0 2^12 + l_1 (units of
2^-38).  Slice 4 stores its digits doubled, so its accumulator holds
C + 2 l_0 with the C-init C = (T_0 & 511) 2^7, and R = acc 2^11 + l_1.  C is
one v_lshlrev_b16 by 7 of T_0's low half: bits 0-8 land at bits 7-15, the
rest falls off the 16-bit result, and the destination's high half is zero."""
import numpy as np

M16, M32 = 0xFFFF, 0xFFFFFFFF
L0_MAX = 64 * 32   # 64 parents, slice-4 digits in [-32, 32]


def cinit16(t0):
    """v_lshlrev_b16 d, 7, t0 (high half of d zero)."""
    return ((t0 & M16) << 7) & M16


def r_new(t0, l0, l1):
    acc = (cinit16(t0) + 2 * l0) & M32            # the int32 MFMA accumulator of slice 4
    return ((acc << 11) + l1) & M32               # one v_lshl_add_u32


def r_parent(t0, l0, l1):
    return ((t0 & 511) * 2 ** 18 + (l0 * 2 ** 12 + l1)) & M32


def _cases():
    rng = np.random.default_rng(16)
    t0s = [0, 511, 512, 0xFFFFFE00, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x0000FE00, 0x0000FFFF, 0xFFFF0000,
           0xFFFF01FF, 1, 256, 255]
    l0s = [0, 1, -1, L0_MAX, -L0_MAX, L0_MAX - 1, -L0_MAX + 1]
    l1s = [0, 1, -1, 2 ** 18, -2 ** 18, -2 ** 17 - 64 * 2080, 2 ** 17 + 64 * 2080, -3]
    for t0 in t0s:
        for l0 in l0s:
            for l1 in l1s:
                yield t0, l0, l1
    for _ in range(20000):
        yield (int(rng.integers(0, 2 ** 32)), int(rng.integers(-L0_MAX, L0_MAX + 1)),
               int(rng.integers(-2 ** 19, 2 ** 19)))
    for _ in range(2000):    # every upper bit of T_0 set, the low field random
        yield 0xFFFFFE00 | int(rng.integers(0, 512)), int(rng.integers(-L0_MAX, L0_MAX + 1)), -int(rng.integers(1, 2 ** 19))


def test_cinit16_gives_the_parents_remainder():
    n = 0
    for t0, l0, l1 in _cases():
        assert cinit16(t0) == (t0 & 511) << 7 <= 65408
        assert r_new(t0, l0, l1) == r_parent(t0, l0, l1), (hex(t0), l0, l1)
        n += 1
    assert n > 20000


def test_remainder_stays_a_small_signed_integer():
    """|R| < 2^28 at the extremes, so the int32 -> f64 conversion of R is exact
    and the wrap-around above is never the value's."""
    for low in (0, 511):
        for l0 in (-L0_MAX, L0_MAX):
            for l1 in (-2 ** 18, 2 ** 18):
                r = r_new(0xABCDE000 | low, l0, l1)
                r -= 2 ** 32 if r >= 2 ** 31 else 0
                assert r == low * 2 ** 18 + l0 * 2 ** 12 + l1 and abs(r) < 2 ** 28


def test_doubled_slice4_digit_fits_int8():
    l = np.arange(-2 ** 17, 2 ** 17 + 1, dtype=np.int64)
    lb = l + 32 * (1 + 64)                        # i8l_digits' balancing bias
    d4 = 2 * (lb >> 12)
    assert d4.min() >= -128 and d4.max() <= 127
    assert d4.min() == -64 and d4.max() == 64
    # the three digits still spell l: slice 4 at 2^11 per (doubled) unit
    d5, d6 = ((lb >> 6) & 63) - 32, (lb & 63) - 32
    assert np.array_equal(d4 * 2 ** 11 + d5 * 64 + d6, l)
