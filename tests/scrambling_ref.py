"""Brute-force CPU reference of the TS 38.211 5.2.1 pseudo-random sequence, written from the specification:

    x1(n + 31) = x1(n + 3) ^ x1(n),                            x1(0) = 1, x1(1..30) = 0
    x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n),    x2(i) = (c_init >> i) & 1
    c(n)       = x1(n + 1600) ^ x2(n + 1600)

It walks the recurrences from n = 0 (the generator srsRAN's own unit test checks against,
pseudo_random_generator_test.cpp:101-123). plain = True walks them exactly as written, 28 steps per numpy operation
(x(n + 31) needs nothing newer than x(n + 3)). The default walk is vectorised further with the squared recurrences: over
GF(2) a sequence that obeys x(n + 31) = x(n + 3) ^ x(n) also obeys x(n + 31 m) = x(n + 3 m) ^ x(n) for m = 2^k (and
likewise x2), so once 31 m bits are known the next 28 m follow in one operation. test_scrambling_host.py checks the
two walks against each other. The device and host code under test jump instead of walking."""
import functools

import numpy as np

NC = 1600


def _walk(x: np.ndarray, taps, total: int, plain: bool = False) -> None:
    known = 31
    while known < total:
        m = 1
        while not plain and 62 * m <= known:
            m *= 2
        lo, k = known - 31 * m, min(28 * m, total - known)
        acc = np.zeros(k, np.uint8)
        for t in taps:
            acc ^= x[lo + t * m:lo + t * m + k]
        x[known:known + k] = acc
        known += k


def walk_registers(c_init: int, total: int, plain: bool):
    """x1 and x2 from n = 0, `total` bits each (no Nc offset)."""
    x1, x2 = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> i) & 1 for i in range(31)]
    _walk(x1, (3, 0), total, plain)
    _walk(x2, (3, 2, 1, 0), total, plain)
    return x1, x2


@functools.lru_cache(maxsize=4)
def _x1(total: int) -> np.ndarray:
    x = np.zeros(total, np.uint8)
    x[0] = 1
    _walk(x, (3, 0), total)
    return x


@functools.lru_cache(maxsize=16)
def _x2(c_init: int, total: int) -> np.ndarray:
    x = np.zeros(total, np.uint8)
    x[:31] = [(c_init >> i) & 1 for i in range(31)]
    _walk(x, (3, 2, 1, 0), total)
    return x


def _total(n: int) -> int:
    return max(4096, 1 << (NC + n + 64).bit_length())   # few distinct sizes, so the cache is shared


def sequence(c_init: int, offset: int, n: int) -> np.ndarray:
    """c(offset) .. c(offset + n - 1), one bit per uint8."""
    t = _total(offset + n)
    a = NC + offset
    return _x1(t)[a:a + n] ^ _x2(c_init, t)[a:a + n]


def state(c_init: int, offset: int):
    """(x1, x2) words: bit i = x(1600 + offset + i), i < 31."""
    t = _total(offset + 31)
    a = NC + offset
    w = 1 << np.arange(31, dtype=np.uint64)
    return (int((_x1(t)[a:a + 31].astype(np.uint64) * w).sum()),
            int((_x2(c_init, t)[a:a + 31].astype(np.uint64) * w).sum()))


def packed(c_init: int, offset: int, nbits: int) -> np.ndarray:
    """The sequence packed MSB first; the last byte's trailing bits are zero."""
    return np.packbits(sequence(c_init, offset, nbits))


def descramble(llr: np.ndarray, c_init: int, offset: int = 0) -> np.ndarray:
    """out[i] = c(offset + i) ? -llr[i] : llr[i] (int8 in [-127, 127])."""
    llr = np.asarray(llr, np.int8)
    c = sequence(c_init, offset, llr.size).astype(bool)
    return np.where(c, -llr.astype(np.int16), llr).astype(np.int8)


def xor_packed(data: np.ndarray, c_init: int, offset: int, nbits: int) -> np.ndarray:
    """Packed bits XOR the sequence over the first nbits; the last byte's other bits unchanged."""
    return np.asarray(data, np.uint8) ^ packed(c_init, offset, nbits)
