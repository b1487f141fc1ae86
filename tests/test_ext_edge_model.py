"""The message of a degree-1 extension column, as the specialised decoder keeps it in a register (ldpc_spec.h,
ext_reg_edge; ldpc_decode_body.h, dec::ext_state / ext_seed / ext_update), against the oracle's LLR arithmetic.

An extension column (>= K + 4) has one edge, shift 0, and is read and written by its row's own lane only. Its v2c at
the next visit is llr_sub(llr_promotion_sum(c2v', v2c), c2v'): the same v2c unless the promotion sum overflowed, and
+-infinity with v2c's sign from then on. The kernel therefore keeps |v2c| (a, 241 or more once infinite) and its sign g
and updates a with 16-bit integer operations; the second test restates those operations in numpy, with their 16-bit
wrap-around, and compares the next state with the oracle chain for every reachable input. CPU only."""
from __future__ import annotations

import numpy as np
import pytest

import oracle as O

V2C = [-127] + list(range(-120, 121)) + [127]  # the 243 valid LLR values
C2V = list(range(-96, 97))  # |c2v'| <= round(0.8 * 120)


@pytest.fixture(scope="module")
def chain():
    """next v2c = llr_sub(llr_promotion_sum(c, v), c) for every valid v and every c in [-96, 96], from the oracle:
    table[v + 127, c + 96]."""
    t = np.full((255, 193), -128, dtype=np.int32)
    for v in V2C:
        for c in C2V:
            t[v + 127, c + 96] = O.llr_sub(O.llr_promotion_sum(c, v), c)
    return t


def test_extension_v2c_is_sticky(chain):
    """llr_sub(llr_promotion_sum(c, v), c) == v when |v| > 120 or |v + c| <= 120, else +-127 with the sign of v."""
    n = n_sat = 0
    for v in V2C:
        for c in C2V:
            got = int(chain[v + 127, c + 96])
            if abs(v) > 120 or abs(v + c) <= 120:
                want = v
            else:
                want = 127 if v > 0 else -127
                n_sat += 1
            assert got == want, (v, c, got, want)
            n += 1
    assert n == 243 * 193 == 46899
    assert n_sat == 9312


def _scale(m):
    """round(0.8f * m), half away from zero, in float32 as ldpc_decoder_generic.cpp scales a magnitude."""
    v = m.astype(np.float32) * np.float32(0.8)
    return np.floor(v + np.float32(0.5)).astype(np.int64)


def _i16(x):
    """the low 16 bits of x as a signed 16-bit integer"""
    x = x & 0xFFFF
    return np.where(x >= 0x8000, x - 0x10000, x)


def _model_update(X, m1, m2, sx):
    """dec::ext_update on the state word X (int64 arrays holding 32-bit words), operation by operation; n1, n2 + m1
    and sx | 1 are row_consts' N1, CC and PP."""
    n1 = (m1 * 52432 + 26216) >> 16
    n2 = (m2 * 52432 + 26216) >> 16
    d = ((n2 + m1) - (X & 0xFFFF)) & 0xFFFF  # v_sub_u16
    f = np.maximum(_i16(n1), _i16(d)) & 0xFFFF  # v_max_i16
    pf = (f * ((sx | 1) & 0xFFFF)) & 0xFFFF  # v_mul_lo_u16
    u = ((X & 0xFFFF) + pf) & 0xFFFF  # v_add_u16
    x = (120 - u) & 0xFFFF  # v_sub_u16: negative, upper byte 0xff, iff u >= 121
    assert np.all((_i16(x) >= -256) & (_i16(x) < 256))
    return X | (x >> 8)  # v_lshrrev_b16 8, v_or_b32


def test_register_update_matches_oracle_chain(chain):
    """Every a in [0, 120] and every infinity marker in [241, 255], g = +-1, P = +-1 and (m1, m2) with
    m1 <= m2 <= 120 that the two-minimum scan can leave when the edge takes part in it: min(a, 120) >= m1, and
    min(a, 120) >= m2 unless it equals m1 (the scan starts at (120, 120) with a strict <, so an edge above the minimum
    is at least the second minimum). The reference gives n2 to the edge with |v2c| == m1 and n1 to the others."""
    a_vals = np.array(list(range(0, 121)) + list(range(241, 256)), dtype=np.int64)
    mm = np.array([(p, q) for p in range(121) for q in range(p, 121)], dtype=np.int64)
    a, g, P, k = np.meshgrid(a_vals, np.array([1, -1]), np.array([1, -1]), np.arange(len(mm)), indexing="ij")
    a, g, P, k = a.ravel(), g.ravel(), P.ravel(), k.ravel()
    m1, m2 = mm[k, 0], mm[k, 1]
    ac = np.minimum(a, 120)
    keep = (ac >= m1) & ((ac == m1) | (ac >= m2))
    a, g, P, m1, m2, ac = a[keep], g[keep], P[keep], m1[keep], m2[keep], ac[keep]
    assert a.size > 1_000_000

    # the integer scaling is the reference's float one
    m = np.arange(121, dtype=np.int64)
    assert np.array_equal((m * 52432 + 26216) >> 16, _scale(m))

    # oracle chain: v2c, the reference's c2v' for this edge, the next v2c
    inf = a >= 241
    v2c = np.where(inf, 127 * g, a * g)
    mag = np.where(inf, 127, a)
    f_ref = np.where(mag == m1, _scale(m2), _scale(m1))
    c2v = g * P * f_ref
    nxt = chain[v2c + 127, c2v + 96]
    assert nxt.min() >= -127

    # the kernel's state word: a in the low half, g (0x0001 / 0xffff) in the high half; the parity word's low half is
    # +-1 up to bit 0 (fold_halves), here with bit 0 clear to show that sx | 1 is what is used
    X = a | ((g & 0xFFFF) << 16)
    sx = np.where(P < 0, 0xFFFE, 0x0000) | (np.int64(0x5A5A) << 16)  # garbage in the high half
    # seed (dec::ext_seed): first edge of the scan, and the parity's start
    assert np.array_equal(np.minimum(X & 0xFFFF, 120), np.minimum(mag, 120))
    assert np.array_equal(_i16(X >> 16), g)
    X2 = _model_update(X, m1, m2, sx)
    a2 = X2 & 0xFFFF
    assert np.array_equal(X2 >> 16, X >> 16)  # g never changes
    assert np.all((a2 <= 120) | ((a2 >= 241) & (a2 <= 255)))
    got = np.where(a2 >= 241, 127 * g, a2 * g)
    bad = np.nonzero(got != nxt)[0]
    assert bad.size == 0, [(int(a[i]), int(g[i]), int(P[i]), int(m1[i]), int(m2[i]), int(got[i]), int(nxt[i]))
                           for i in bad[:5]]
    # both outcomes occur: some finite states stay finite, some go infinite
    fin = ~inf
    assert np.any(fin & (a2 >= 241)) and np.any(fin & (a2 <= 120))
    # and the initial state (dec::ext_state) of every soft bit the prologue can leave in LDS
    for s in range(-121, 122):
        sv = -1 if s < 0 else 0
        mag0 = (s ^ sv) - sv
        st = (241 if mag0 > 120 else mag0) | (((sv | 1) & 0xFFFF) << 16)
        assert (st & 0xFFFF) == (241 if abs(s) == 121 else abs(s))
        assert _i16(np.int64(st >> 16)) == (1 if s >= 0 else -1)
