"""The channel equalizer's NumPy restatement, its fixture cases and the fixture's loader (tests/golden/ref_equalize.npz,
recorded by tests/golden/make_equalizer_fixtures.py from the compiled reference).

`equalize(...)` restates channel_equalizer_generic_impl.cpp:165-221 and the scalar loops of equalize_zf_1xn.h:136-178,
equalize_mmse_1xn.h:56-96 and equalize_zf_2xn.h:58-63, 182-252 in float32, operand by operand: every product and sum is
one NumPy float32 operation (nothing fused), a complex product is (ac - bd, ad + bc), a division is IEEE, denormals are
kept, std::isnormal is the exponent test and cbf16 to float is bits << 16.

Inputs are bf16 bit patterns from integer draws only (tests/vectors.py's splitmix64), so a case is its parameters and
a seed; cbf16 arrays are uint16[..., 2] (re, im), received symbols [port, re], estimates [layer, port, re]."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from tests.ref_cases import digest
from tests.vectors import sm_ints

ZF, MMSE = 0, 1
TOPOLOGIES = [(ZF, p, 1) for p in (1, 2, 3, 4)] + [(MMSE, p, 1) for p in (1, 2, 3, 4)] + [(ZF, 2, 2), (ZF, 4, 2)]
NOF_RES = (1, 7, 67, 257)
TX_SCALINGS = (1.0, 0.7071, 2.5)
# a special estimate: +-0, a value whose squared norm is denormal (2^-64 in both components), +-inf, NaN
SPECIALS = (0x0000, 0x8000, 0x1F80, 0x7F80, 0xFF80, 0x7FC0)
# a bad port variance: 0, -1, +inf, NaN, 1e-40 (denormal), as float32 bit patterns
BAD_VARIANCES = (0x00000000, 0xBF800000, 0x7F800000, 0x7FC00000, 0x000116C2)
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_equalize.npz"


def f32(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def bits_of(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def from_cbf16(a: np.ndarray):
    """uint16[..., 2] -> (re, im) float32: bits << 16."""
    w = np.asarray(a, np.uint16).astype(np.uint32) << np.uint32(16)
    return w[..., 0].view(np.float32), w[..., 1].view(np.float32)


def isnormal(x) -> np.ndarray:
    e = (bits_of(x) >> np.uint32(23)) & np.uint32(0xFF)
    return (e != 0) & (e != 0xFF)


def _mul(a, b):
    """(ac - bd, ad + bc)"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _conj(a):
    return a[0], -a[1]


def _norm(a):
    return a[0] * a[0] + a[1] * a[1]


def _max_element(v):
    """std::max_element: the first largest; a NaN never replaces and is never replaced."""
    m = v[0]
    for x in v[1:]:
        if m < x:
            m = x
    return m


def equalize(algorithm, ch_symbols, ch_estimates, noise_vars, tx_scaling):
    """(eq_symbols complex64 [nof_re * layers], eq_noise_vars float32 [nof_re * layers]), two layers interleaved per RE."""
    P, n = ch_symbols.shape[0], ch_symbols.shape[1]
    L = ch_estimates.shape[0]
    assert ch_estimates.shape[:3] == (L, P, n) and len(noise_vars) == P
    assert (L == 1 and 1 <= P <= 4 and algorithm in (ZF, MMSE)) or (L == 2 and P in (2, 4) and algorithm == ZF)
    nv = np.asarray(noise_vars, np.float32)
    ts = np.float32(tx_scaling)
    inf, zero = np.float32(np.inf), np.zeros(n, np.float32)
    y = [from_cbf16(ch_symbols[p]) for p in range(P)]
    h = [[from_cbf16(ch_estimates[l, p]) for p in range(P)] for l in range(L)]
    with np.errstate(all="ignore"):
        if L == 1:
            ch_mod_sq, nvar_acc, out_re, out_im = zero.copy(), zero.copy(), zero.copy(), zero.copy()
            for p in range(P):
                est = h[0][p]
                if algorithm == MMSE:
                    est = (est[0] * ts, est[1] * ts)
                norm = _norm(est)
                use = isnormal(norm) & bool(isnormal(nv[p]) and nv[p] > 0)
                m = _mul(y[p], _conj(est))
                ch_mod_sq = np.where(use, ch_mod_sq + norm, ch_mod_sq)
                nvar_acc = np.where(use, nvar_acc + norm * nv[p], nvar_acc)
                out_re = np.where(use, out_re + m[0], out_re)
                out_im = np.where(use, out_im + m[1], out_im)
            if algorithm == MMSE:
                good = isnormal(ch_mod_sq) & isnormal(nvar_acc)
                rcp = np.float32(1) / (ch_mod_sq * ch_mod_sq + nvar_acc)
                s_re, s_im, var = out_re * ch_mod_sq * rcp, out_im * ch_mod_sq * rcp, nvar_acc * rcp
            else:
                d_pinv = ts * ch_mod_sq
                good = isnormal(d_pinv) & isnormal(nvar_acc)
                rcp = np.float32(1) / d_pinv
                s_re, s_im, var = out_re * rcp, out_im * rcp, nvar_acc * rcp * rcp
            sym = np.where(good, s_re, zero) + 1j * np.where(good, s_im, zero)
            return sym.astype(np.complex64), np.where(good, var, inf).astype(np.float32)
        noise_var = _max_element(nv)
        sym = np.zeros((n, 2, 2), np.float32)
        var = np.full((n, 2), inf, np.float32)
        if not isnormal(noise_var) or noise_var < 0:
            return sym.view(np.complex64).reshape(-1), var.reshape(-1)
        norm_sq = []
        for l in range(2):
            s = zero.copy()
            for p in range(P):
                s = s + _norm(h[l][p])
            norm_sq.append(s)
        xi = (zero.copy(), zero.copy())
        for p in range(P):
            m = _mul(_conj(h[0][p]), h[1][p])
            xi = (xi[0] + m[0], xi[1] + m[1])
        xi_mod_sq = _norm(xi)
        matched = []
        for l in range(2):
            acc = (zero.copy(), zero.copy())
            for p in range(P):
                m = _mul(_conj(h[l][p]), y[p])
                acc = (acc[0] + m[0], acc[1] + m[1])
            matched.append(acc)
        d_pinv = ts * ((norm_sq[0] * norm_sq[1]) - xi_mod_sq)
        d_nvars = ts * d_pinv
        good = isnormal(d_pinv)
        rcp, nrcp = np.float32(1) / d_pinv, np.float32(1) / d_nvars
        a, b = _mul(xi, matched[1]), _mul(_conj(xi), matched[0])
        for l, (own, other, prod) in enumerate(((0, 1, a), (1, 0, b))):
            sym[:, l, 0] = np.where(good, (norm_sq[other] * matched[own][0] - prod[0]) * rcp, zero)
            sym[:, l, 1] = np.where(good, (norm_sq[other] * matched[own][1] - prod[1]) * rcp, zero)
            var[:, l] = np.where(good, noise_var * norm_sq[other] * nrcp, inf)
        return sym.view(np.complex64).reshape(-1), var.reshape(-1)


# ---- cases --------------------------------------------------------------------------------------------------------
def cases():
    """The ten topologies x nof_re x tx_scaling; per topology the (67, 0.7071) case carries one bad port variance.
    nv: the port variances as float32 bit patterns ((1 + draw % 64) / 1024 where they are good)."""
    out = []
    for t, (alg, P, L) in enumerate(TOPOLOGIES):
        for i, n in enumerate(NOF_RES):
            for j, ts in enumerate(TX_SCALINGS):
                seed = 91000 + 100 * t + 10 * i + j
                nv = [int(bits_of(np.float32(1 + d) / np.float32(1024))) for d in sm_ints(seed + 5, P, 0, 64)]
                c = dict(alg=alg, ports=P, layers=L, n=n, ts=ts, seed=seed, nv=nv)
                if n == 67 and j == 1:
                    c["bad_port"] = int(sm_ints(seed + 6, 1, 0, P)[0])
                    nv[c["bad_port"]] = BAD_VARIANCES[t % len(BAD_VARIANCES)]
                out.append(c)
    return out


def _bf16(seed, shape, e_lo, e_hi):
    """random finite bf16 patterns: any sign, exponent in [e_lo, e_hi), any mantissa"""
    k = int(np.prod(shape))
    d = sm_ints(seed, k, 0, 1 << 16)
    e = sm_ints(seed + 1, k, e_lo, e_hi)
    return (((d & 0x8000) | (e << 7) | (d & 0x7F)).astype(np.uint16)).reshape(shape)


def to_bf16(x) -> np.ndarray:
    """bf16.h:38-55: float32 to bf16, round to nearest, ties to even."""
    u = bits_of(x)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


DISTINCT = 96  # a case's REs from this one on repeat earlier ones' inputs (see case_input)


def case_input(c):
    """(ch_symbols uint16 [P, n, 2], ch_estimates uint16 [L, P, n, 2]). Symbols are finite (2^-7 .. 2^3); estimates
    2^-9 .. 2^3.
    RE i >= DISTINCT takes the inputs of RE (29 i + 7) % DISTINCT: the 257-RE cases are there for the layout (more
    than one block, every vector path), the arithmetic's variety is in the first DISTINCT REs and the smaller cases, and
    the recorded outputs of repeated REs compress, which keeps the fixture under the size every golden file observes.
    Then about one RE in 16 becomes special: a SPECIALS pattern in both components of one estimate plane or of all
    of them. With two layers one more RE in 16 is a singular channel whose sums are not exact: six-bit mantissas,
    every component at its own exponent, layer 1 = 3 x layer 0 exactly, so that n0 n1 - |xi|^2 is the difference of
    two roundings of the same number: zero or a last bit of either sign (the negative-variance outcome)."""
    P, L, n, s = c["ports"], c["layers"], c["n"], c["seed"]
    sym = _bf16(s, (P, n, 2), 120, 131)
    est = _bf16(s + 2, (L, P, n, 2), 118, 131)
    if n > DISTINCT:
        src = (29 * np.arange(DISTINCT, n) + 7) % DISTINCT
        sym[:, DISTINCT:] = sym[:, src]
        est[:, :, DISTINCT:] = est[:, :, src]
    pick = sm_ints(s + 4, n, 0, 16)
    what = sm_ints(s + 7, n, 0, len(SPECIALS))
    plane = sm_ints(s + 8, n, 0, L * P)
    scope = sm_ints(s + 9, n, 0, 2)
    flat = est.reshape(L * P, n, 2)
    for i in np.flatnonzero(pick == 0):
        if scope[i]:
            flat[:, i, :] = SPECIALS[what[i]]
        else:
            flat[plane[i], i, :] = SPECIALS[what[i]]
    if L == 2:
        m = (32 + sm_ints(s + 10, P * n * 2, 0, 32)) * (1 - 2 * sm_ints(s + 11, P * n * 2, 0, 2))
        e = sm_ints(s + 12, P * n * 2, 118, 131).reshape(P, n, 2)
        h0 = np.ldexp(m.reshape(P, n, 2).astype(np.float32), e - 132).astype(np.float32)
        h1 = np.float32(3) * h0
        sing = pick == 1
        est[0][:, sing] = to_bf16(h0)[:, sing]
        est[1][:, sing] = to_bf16(h1)[:, sing]
    return sym, est


def run(fn, c, inp):
    """{name: integer array} of one implementation fn(alg, sym, est, noise_vars, tx_scaling) -> (complex64, float32)"""
    sym, var = fn(c["alg"], inp[0], inp[1], f32(c["nv"]), np.float32(c["ts"]))
    return {"sym": np.ascontiguousarray(sym, np.complex64).view(np.uint32), "var": bits_of(var)}


def load_fixture():
    """(cases, recorded reference outputs {sym, var: uint32 bit patterns}, regenerated inputs); every input's SHA-256
    must equal the recorded one."""
    d = np.load(GOLDEN, allow_pickle=False)
    cs = json.loads(str(d["index"]))
    outs, inputs = [], []
    for i, c in enumerate(cs):
        inp = case_input(c)
        assert digest(*inp) == c["sha"], f"ref_equalize.npz: the regenerated input of case {i} has another digest"
        inputs.append(inp)
        outs.append(unpack_outputs(d["out"][int(d["off"][i]):int(d["off"][i + 1])]))
    return cs, outs, inputs


def pack_outputs(o: dict) -> np.ndarray:
    """uint32[k, 3]: (symbol re, symbol im, variance) per output, so that a repeated RE is one repeated record"""
    return np.column_stack([o["sym"][0::2], o["sym"][1::2], o["var"]]).astype(np.uint32)


def unpack_outputs(rec: np.ndarray) -> dict:
    return {"sym": np.ascontiguousarray(rec[:, :2]).reshape(-1), "var": np.ascontiguousarray(rec[:, 2])}
