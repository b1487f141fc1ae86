"""The row tail of the specialised decoder (ldpc_decode_body.h: fold_halves, sign_word, dec::ext_seed / ext_fold),
restated in numpy with its 16-bit words against the sequential scan it replaces. CPU only.

1. The extension edge's magnitude joins the two minima after the packed scan (ext_fold) instead of seeding it: the
   sequential two-minimum scan of the reference (start (120, 120), strict <) over the extension edge first and the
   row's other edges after it must leave the same (min1, min2) as the per-half scans of the pairs, their fold and the
   extension edge last.
2. The parity word: every half of SX is the XOR of +-1 words (0x0001 / 0xffff). lo ^ hi is the check node's sign, +-1,
   as it stands when an odd number of words went in (a row with an extension edge: its sign and two per pair), and
   after | 1 for an even number."""
from __future__ import annotations

import numpy as np

INF = 241  # an infinite v2c's magnitude in the packed scan (pass1); the extension state's markers are 241..255


def _scan(vals, m1, m2):
    """the reference's scan: strict <, values above 120 (infinite) never move a minimum that starts at 120"""
    for v in vals.T:
        m2 = np.where(v < m1, m1, np.where(v < m2, v, m2))
        m1 = np.minimum(m1, v)
    return m1, m2


def _packed_tail(pairs, a_ext):
    """pass1's per-half minima over the pairs (columns 2 i: low half, 2 i + 1: high half), fold_halves, ext_fold"""
    n = pairs.shape[0]
    M1 = np.full((n, 2), 120, np.int64)
    M2 = np.full((n, 2), 120, np.int64)
    for i in range(0, pairs.shape[1], 2):
        a = pairs[:, i:i + 2]
        M2 = np.minimum(M2, np.maximum(M1, a))
        M1 = np.minimum(M1, a)
    m1 = np.minimum(M1[:, 0], M1[:, 1])
    m2 = np.minimum(np.minimum(M2[:, 0], M2[:, 1]), np.maximum(M1[:, 0], M1[:, 1]))
    if a_ext is not None:
        a = np.minimum(a_ext & 0xFFFF, 120)
        m2 = np.minimum(m2, np.maximum(m1, a))
        m1 = np.minimum(m1, a)
    return m1, m2


def test_extension_edge_folded_last_equals_scanned_first():
    rng = np.random.default_rng(11)
    a_vals = np.array(list(range(121)) + list(range(241, 256)), np.int64)
    # one pair, exhaustively: every (a_ext, lo, hi)
    v = np.array(list(range(121)) + [INF], np.int64)
    A, LO, HI = (x.ravel() for x in np.meshgrid(a_vals, v, v, indexing="ij"))
    cases = [(A, np.stack([LO, HI], 1))]
    # 2 to 9 pairs, random, with many ties, 120s and infinities
    for npairs in range(2, 10):
        n = 20000
        p = rng.integers(0, 122, (n, 2 * npairs))
        p = np.where(rng.random(p.shape) < 0.15, rng.choice([0, 1, 119, 120, INF], p.shape), p)
        p[p == 121] = INF
        cases.append((rng.choice(a_vals, n), p.astype(np.int64)))
    for a_ext, pairs in cases:
        n = a_ext.size
        start = np.full(n, 120, np.int64)
        ref1, ref2 = _scan(np.concatenate([np.minimum(a_ext, 127)[:, None], pairs], 1), start, start)
        got1, got2 = _packed_tail(pairs, a_ext)
        assert np.array_equal(got1, ref1) and np.array_equal(got2, ref2)
        # and a row without an extension edge
        ref1, ref2 = _scan(pairs, start, start)
        got1, got2 = _packed_tail(pairs, None)
        assert np.array_equal(got1, ref1) and np.array_equal(got2, ref2)


def test_parity_word_needs_no_or_for_an_odd_count():
    rng = np.random.default_rng(12)
    for npairs in range(1, 10):
        for ext in (False, True):
            n = 4000
            g = np.where(rng.integers(0, 2, (n, 2 * npairs + int(ext))) == 1, 0xFFFF, 0x0001).astype(np.int64)
            want = np.where(np.count_nonzero(g == 0xFFFF, axis=1) % 2 == 1, 0xFFFF, 0x0001)
            SX = np.zeros(n, np.int64)
            if ext:  # ext_seed: the extension edge's sign word starts the low half
                SX = g[:, -1].copy()
            for i in range(npairs):  # pass1: SX ^= (g_lo | g_hi << 16)
                SX ^= g[:, 2 * i] | (g[:, 2 * i + 1] << 16)
            sx = (SX ^ (SX >> 16)) & 0xFFFF  # fold_halves, low half
            if ext:
                assert np.array_equal(sx, want)  # sign_word<true>: as it stands
            else:
                assert np.all((sx & 1) == 0)  # an even count leaves bit 0 clear ...
                assert np.array_equal(sx | 1, want)  # ... and sign_word<false> sets it
