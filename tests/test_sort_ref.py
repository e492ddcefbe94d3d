"""The host predictor of the build's key sort (tests/sort_ref.py) on synthetic keys: the GPU tests of the radix sort
(tests/test_radix_sort_gpu.py) compare the device's order with it element for element, so it is pinned here without a GPU."""
import numpy as np
import pytest

from tests import sort_ref


def test_ties_keep_their_index_order():
    keys = np.array([5, 1, 5, 0, 1, 5, 0], np.uint64) << np.uint64(40)
    np.testing.assert_array_equal(sort_ref.expected_order(keys, 40, 8), [3, 6, 1, 4, 0, 2, 5])
    same = np.full(1000, 0x1234_5678_9abc_def0, np.uint64)
    np.testing.assert_array_equal(sort_ref.expected_order(same, 31, 32), np.arange(1000))


def test_against_a_plain_python_sort_of_the_masked_digits():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 63, 3000, dtype=np.uint64)
    keys[::3] = keys[5]                                                   # long tie runs
    for lo, n in ((46, 17), (31, 32), (55, 8), (62, 1)):
        digits = [(int(k) >> lo) & ((1 << n) - 1) for k in keys]
        want = sorted(range(len(keys)), key=lambda i: (digits[i], i))
        np.testing.assert_array_equal(sort_ref.expected_order(keys, lo, n), want)


def test_bits_outside_the_range_do_not_count():
    rng = np.random.default_rng(2)
    base = rng.integers(0, 1 << 12, 500, dtype=np.uint64) << np.uint64(46)        # bits [46, 58)
    want = sort_ref.expected_order(base, 46, 12)
    noise = rng.integers(0, 1 << 46, 500, dtype=np.uint64) | (rng.integers(0, 1 << 5, 500, dtype=np.uint64) << np.uint64(58))
    np.testing.assert_array_equal(sort_ref.expected_order(base | noise, 46, 12), want)
    assert not np.array_equal(sort_ref.expected_order(base | noise, 45, 13), want)     # one bit more: the noise below shows
    assert not np.array_equal(sort_ref.expected_order(base | noise, 46, 13), want)     # ... and above


def test_a_32_bit_key_is_the_64_bit_key_shifted_by_31():
    rng = np.random.default_rng(3)
    k64 = rng.integers(0, 1 << 63, 4000, dtype=np.uint64)
    k32 = (k64 >> np.uint64(31)).astype(np.uint32)
    assert k32.dtype == np.uint32 and int(k32.max()) < 1 << 32
    for P, extra in ((5121, 4), (40_000, 12), (2, 0), (300_000, 12)):
        lo64, n64 = sort_ref.bit_range(P, extra, "own", 8)
        lo32, n32 = sort_ref.bit_range(P, extra, "own", 4)
        assert n32 == n64 and lo64 - lo32 == 31
        np.testing.assert_array_equal(sort_ref.expected_order(k32, lo32, n32), sort_ref.expected_order(k64, lo64, n64))


def test_the_bit_range_rule():
    assert [sort_ref.ceil_log2(P) for P in (1, 2, 3, 4, 5, 256, 257, 131_071, 131_072, 131_073)] == [1, 1, 2, 2, 3, 8, 9, 17, 17, 18]
    # P = 5121: 13 bits; + 4 = 17 sorted bits; rocPRIM rounds up to 24
    assert sort_ref.bit_range(5121, 4, "own", 8) == (46, 17)
    assert sort_ref.bit_range(5121, 4, "own", 4) == (15, 17)
    assert sort_ref.bit_range(5121, 4, "rocprim") == (39, 24)
    # the clamps: never fewer than 8 bits, never below bit 31 of the code
    assert sort_ref.bit_range(1, 0, "own", 8) == (55, 8) and sort_ref.bit_range(2, 4, "own", 4) == (24, 8)
    assert sort_ref.bit_range(1, 0, "rocprim") == (55, 8)
    assert sort_ref.bit_range(1 << 22, 12, "own", 8) == (31, 32) and sort_ref.bit_range(1 << 22, 12, "own", 4) == (0, 32)
    assert sort_ref.bit_range(300_000, 12, "own", 4) == (1, 31) and sort_ref.bit_range(300_000, 12, "rocprim") == (31, 32)
    assert sort_ref.bit_range(40_000, 0, "own", 8) == (47, 16) and sort_ref.bit_range(40_000, 0, "rocprim") == (47, 16)
    with pytest.raises(ValueError):
        sort_ref.bit_range(5121, 4, "rocprim", 4)
    # which sort a build takes
    assert [sort_ref.uses_own_sort(P, 2) for P in (131_071, 131_072)] == [False, True]
    assert sort_ref.uses_own_sort(1, 1) and not sort_ref.uses_own_sort(300_000, 0)


def test_bad_arguments_are_refused():
    with pytest.raises(TypeError):
        sort_ref.expected_order(np.zeros(4, np.int64), 0, 8)
    with pytest.raises(ValueError):
        sort_ref.expected_order(np.zeros(4, np.uint32), 25, 8)
    with pytest.raises(ValueError):
        sort_ref.expected_order(np.zeros(4, np.uint64), 60, 8)
