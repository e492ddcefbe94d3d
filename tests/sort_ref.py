"""Host predictor of the build's key sort (tests/ only, pure numpy): what a correct, stable sort on a bit range of the Morton keys must
return, and the bit range each of the build's sorts works on (restated from sort_all in lidar_rt_amd/csrc/lrt_kernels.hip)."""
import numpy as np

SORT_LO_BIT = 31            # LRT_SORT_LO_BIT: no build sorts below this bit of the 63-bit Morton code
CODE_BITS = 63
MERGE_LIMIT = 131072        # LRT_BUILD_MERGE_LIMIT: own_sort = 2 takes the own radix sort from this many primitives on
RS_TILE, RS_WAVE_CHUNK = 256 * 20, 64 * 20      # lrt_radix.inc: keys per tile, keys per wave


def expected_order(keys_by_index, lo_bit, n_bits):
    """The order a stable sort of bits [lo_bit, lo_bit + n_bits) of keys_by_index (key of primitive i at position i) produces: equal
    digits keep their index order, bits outside the range do not count."""
    keys = np.asarray(keys_by_index)
    if keys.dtype not in (np.uint32, np.uint64):
        raise TypeError("keys must be uint32 or uint64")
    if lo_bit < 0 or n_bits < 1 or lo_bit + n_bits > keys.dtype.itemsize * 8:
        raise ValueError(f"bits [{lo_bit}, {lo_bit + n_bits}) outside a {keys.dtype.itemsize * 8}-bit key")
    k = keys.astype(np.uint64)
    mask = np.uint64((1 << n_bits) - 1)
    return np.argsort((k >> np.uint64(lo_bit)) & mask, kind="stable")


def ceil_log2(P):
    """Smallest b >= 1 with 2**b >= P (the build's pbits)."""
    b = 1
    while (1 << b) < P:
        b += 1
    return b


def sorted_bits(P, morton_extra_bits):
    """sb: the number of top Morton bits the own radix sort orders."""
    return min(max(ceil_log2(P) + morton_extra_bits, 8), CODE_BITS - SORT_LO_BIT)


def rocprim_sorted_bits(P, morton_extra_bits):
    """rocPRIM's sort of the build: the same count rounded up to whole 8-bit digits."""
    return min(max(((ceil_log2(P) + morton_extra_bits + 7) // 8) * 8, 8), CODE_BITS - SORT_LO_BIT)


def bit_range(P, morton_extra_bits, sorter, key_bytes=8):
    """(lo_bit, n_bits) of the build's sort of P primitives, in the key the sort sees: sorter "own" with 64-bit keys (the 63-bit code) or
    32-bit keys (code >> 31), or "rocprim" (always 64-bit keys)."""
    if sorter == "rocprim":
        if key_bytes != 8:
            raise ValueError("rocPRIM builds keep 64-bit keys")
        n = rocprim_sorted_bits(P, morton_extra_bits)
        return CODE_BITS - n, n
    if sorter != "own":
        raise ValueError(sorter)
    n = sorted_bits(P, morton_extra_bits)
    return {8: CODE_BITS - n, 4: 32 - n}[key_bytes], n


def uses_own_sort(P, own_sort):
    """The build's rule (no launch graph): 0 rocPRIM, 1 own, 2 own from MERGE_LIMIT primitives on."""
    return own_sort == 1 or (own_sort == 2 and P >= MERGE_LIMIT)
