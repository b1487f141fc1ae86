"""The precoder's NumPy restatement, its fixture cases and the fixture's loader (tests/golden/ref_precode.npz, recorded
by tests/golden/make_precoder_fixtures.py from the compiled reference).

`precode(...)` restates channel_precoder_generic.cpp:27-70 in float32, operand by operand: per port the first product
is assigned (sum = x_0 w_0, so a zero keeps the product's sign), then sum += x_i w_i for i = 1 .. L - 1; a complex
product is (ac - bd, ad + bc), every product and sum one NumPy float32 operation (nothing fused). `map_grid(...)`
restates resource_grid_mapper_impl.cpp:293-436 with re_skip == 0 over it: the masked REs in ascending (symbol,
subcarrier) order, the r-th reading layer i at input[L r + i], the PRG of subcarrier k being k / (12 prg_size) from grid
subcarrier 0, and the result put as cbf16 (bf16.h:38-55: u += 0x7fff + ((u >> 16) & 1), u >>= 16; Re in the low half).

Inputs come from integer draws only (tests/vectors.py's splitmix64), so a case is its parameters and a seed. ci8 arrays
are int8[n, 2]; a grid is uint32[port, symbol, subcarrier], one cbf16 element each."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from tests.ref_cases import digest
from tests.vectors import sm_ints

NRE = 12
NSYMB = 14
TOPOLOGIES = [(L, P) for L in range(1, 5) for P in range(L, 5)]
WIDEBAND = 275  # precoding_configuration::make_wideband: one PRG of MAX_NOF_PRBS
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_precode.npz"
GUARD = 0xDEADBEEF  # what a test's grid holds before the launch
TIE_DOWN, TIE_UP = 0x3F808000, 0x3F818000  # bf16 ties: to the even 0x3f80 below, to the even 0x3f82 above


def f32(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def bits_of(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def to_bf16(x) -> np.ndarray:
    u = bits_of(x)
    return (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)


def to_cbf16(re, im) -> np.ndarray:
    """uint32: bf16 re in the low half, bf16 im in the high half"""
    return to_bf16(re) | (to_bf16(im) << np.uint32(16))


def modulation_scaling(qm: int) -> np.float32:
    """modulation_mapper::get_modulation_scaling"""
    if qm == 2:
        return np.float32(0.70710678118654752440)
    return np.sqrt(np.float32(1.0) / np.float32({4: 10, 6: 42, 8: 170}[qm]))


def precode(xr, xi, wr, wi):
    """x: float32 [L, n]; w: float32 [P, L] or, per RE, [P, L, n]. Returns (re, im) float32 [P, n]."""
    L, n = xr.shape
    P = wr.shape[0]
    if wr.ndim == 2:
        wr, wi = wr[:, :, None], wi[:, :, None]
    out_re, out_im = np.empty((P, n), np.float32), np.empty((P, n), np.float32)
    with np.errstate(all="ignore"):
        for p in range(P):
            sr = xr[0] * wr[p, 0] - xi[0] * wi[p, 0]
            si = xr[0] * wi[p, 0] + xi[0] * wr[p, 0]
            for i in range(1, L):
                sr = sr + (xr[i] * wr[p, i] - xi[i] * wi[p, i])
                si = si + (xr[i] * wi[p, i] + xi[i] * wr[p, i])
            out_re[p], out_im[p] = sr, si
    return out_re, out_im


def _parts(z):
    z = np.ascontiguousarray(z, np.complex64)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def _complex(re, im) -> np.ndarray:
    return np.ascontiguousarray(np.stack([re, im], axis=-1), np.float32).view(np.complex64)[..., 0]


def layer_map(sym, L):
    """ci8 int8[n L, 2] -> float32 (re, im) [L, n]: to_cf of input[L r + i]"""
    s = np.asarray(sym, np.int8).reshape(-1, L, 2).astype(np.float32)
    return np.ascontiguousarray(s[:, :, 0].T), np.ascontiguousarray(s[:, :, 1].T)


def apply_layer_map_and_precoding(sym, w) -> np.ndarray:
    """ci8 int8[n L, 2], complex64 [P, L] -> complex64 [P, n]"""
    w = np.ascontiguousarray(w, np.complex64)
    return _complex(*precode(*layer_map(sym, w.shape[1]), *_parts(w)))


def apply_precoding(x, w) -> np.ndarray:
    """complex64 [L, n], complex64 [P, L] -> complex64 [P, n]"""
    return _complex(*precode(*_parts(x), *_parts(w)))


def map_values(masks, prg_size, w, sym):
    """The masked REs of one transmission before the cbf16 conversion: (l, k) index arrays in mapping order and
    (re, im) float32 [P, count]. masks bool[nsym, nsubc]; w complex64 [prg, P, L], scaling applied."""
    w = np.ascontiguousarray(w, np.complex64)
    L = w.shape[2]
    l_idx, k_idx = np.nonzero(masks)  # row-major: ascending symbol, then subcarrier
    prg = k_idx // (NRE * prg_size)
    assert prg.size == 0 or prg.max() < w.shape[0]
    wr, wi = _parts(w)
    wr, wi = np.moveaxis(wr[prg], 0, -1), np.moveaxis(wi[prg], 0, -1)  # [P, L, count]
    xr, xi = layer_map(np.asarray(sym)[:L * l_idx.size], L)
    return l_idx, k_idx, precode(xr, xi, wr, wi)


def map_grid(grid, masks, prg_size, w, sym) -> int:
    """Writes one transmission into grid (uint32 [port, symbol, subcarrier]); returns its number of REs."""
    l_idx, k_idx, (re, im) = map_values(masks, prg_size, w, sym)
    for p in range(re.shape[0]):
        grid[p, l_idx, k_idx] = to_cbf16(re[p], im[p])
    return l_idx.size


def scaled(w, s) -> np.ndarray:
    """srsvec::sc_prod: (re s, im s) in float32"""
    w = np.ascontiguousarray(w, np.complex64)
    return (w.view(np.float32) * np.float32(s)).astype(np.float32).view(np.complex64).reshape(w.shape)


# ---- cases ------------------------------------------------------------------------------------------------------------
def pattern_mask(patterns, nrb) -> np.ndarray:
    """re_pattern_list::get_inclusion_mask per symbol: patterns of (PRB ranges [[begin, end), ..], 12-bit RE mask with
    bit i for RE i, OFDM symbols) -> bool[NSYMB, 12 nrb]"""
    m = np.zeros((NSYMB, nrb * NRE), bool)
    for prbs, re_mask, symbols in patterns:
        res = [i for i in range(NRE) if (re_mask >> i) & 1]
        for b, e in prbs:
            for prb in range(b, e):
                for l in symbols:
                    m[l, [prb * NRE + i for i in res]] = True
    return m


def case_masks(c) -> np.ndarray:
    """The allocation minus the reserved REs, per symbol."""
    return pattern_mask(c["incl"], c["nrb"]) & ~pattern_mask(c["resv"], c["nrb"])


def _grid_case(seed, L, P, nrb, prg_size, qm, incl, resv=(), weights="rand"):
    return dict(form="grid", layers=L, ports=P, nrb=nrb, prg_size=prg_size, qm=qm, incl=[list(x) for x in incl],
                resv=[list(x) for x in resv], weights=weights, seed=seed)


def cases():
    full = 0xFFF
    g = [
        # 11 RB, wideband; a DM-RS symbol whose data REs are the comb 0xAAA between two full data symbols
        _grid_case(93000, 1, 1, 11, WIDEBAND, 2, [([[0, 11]], full, [2, 3, 4])], [([[0, 11]], 0x555, [3])]),
        # begins inside mask word 0 and ends inside word 1; prg_size 4 from PRB 1: PRGs 0, 1 and 2; comb 0x555
        _grid_case(93001, 1, 2, 11, 4, 4, [([[1, 10]], full, [0, 1, 2])], [([[1, 10]], 0xAAA, [1])]),
        # symbol 6 wholly reserved between symbols 5 and 7
        _grid_case(93002, 1, 3, 25, 8, 6, [([[3, 12]], full, [5, 6, 7])], [([[3, 12]], full, [6])]),
        # one reserved RE per RB: partial nibbles that are no comb
        _grid_case(93003, 1, 4, 25, WIDEBAND, 8, [([[10, 25]], full, [1])], [([[0, 25]], 0x010, [1])]),
        # a non-contiguous allocation, prg_size 4
        _grid_case(93004, 2, 2, 25, 4, 8, [([[2, 5], [9, 10], [14, 19]], full, [3, 4])], [([[0, 25]], 0x555, [3])]),
        _grid_case(93005, 2, 3, 25, 11, 4, [([[5, 24]], full, [0])]),
        # 52 RB: a row of ten mask words
        _grid_case(93006, 2, 4, 52, WIDEBAND, 8, [([[0, 52]], full, [13])], [([[0, 52]], 0xAAA, [13])]),
        _grid_case(93007, 3, 3, 11, 4, 8, [([[0, 11]], full, [0, 1])]),
        _grid_case(93008, 3, 4, 25, 8, 6, [([[7, 18]], full, [2])], [([[0, 25]], 0x800, [2])]),
        _grid_case(93009, 4, 4, 11, 4, 6, [([[2, 9]], full, [6, 7])]),
        # one masked RE
        _grid_case(93010, 2, 4, 25, WIDEBAND, 2, [([[4, 5]], 0x020, [9])]),
        # one layer and zero weights: a level of -1 stores a negative zero
        _grid_case(93011, 1, 2, 11, WIDEBAND, 2, [([[0, 2]], full, [0])], weights="zero"),
        # levels +-1 on the weights (TIE_DOWN, 0) and (TIE_UP, 0): bf16 ties that round down and up
        _grid_case(93012, 1, 2, 11, WIDEBAND, 2, [([[3, 5]], full, [1])], weights="tie"),
    ]
    k = []
    for t, (L, P) in enumerate(TOPOLOGIES):
        # 261 REs: more than one block of 256, and a last, partial nibble
        n = 261 if (L, P) in ((1, 1), (2, 4)) else (37, 5, 64)[t % 3]
        k.append(dict(form="compact", layers=L, ports=P, n=n, qm=(2, 4, 6, 8)[t % 4], seed=94000 + t))
    return g + k


def _levels(seed, n, qm) -> np.ndarray:
    """ci8 int8[n, 2]: odd levels of a 2^qm-QAM, +-1 .. +-(2^(qm / 2) - 1)"""
    m = 1 << (qm // 2)
    return (2 * sm_ints(seed, 2 * n, 0, m) - (m - 1)).astype(np.int8).reshape(n, 2)


def _weights(seed, shape, qm) -> np.ndarray:
    """complex64: integers in [-64, 64] over 37, times the modulation scaling, so nearly every product needs rounding"""
    k = int(np.prod(shape))
    v = sm_ints(seed, 2 * k, -64, 65).astype(np.float32) / np.float32(37)
    return scaled(v.view(np.complex64).reshape(shape), modulation_scaling(qm))


def case_input(c):
    """grid: (ci8 symbols int8[count L, 2], weights complex64 [prg, P, L]); compact: (ci8 symbols int8[n L, 2], cf32
    layers complex64 [L, n], weights complex64 [P, L])."""
    L, P, s, qm = c["layers"], c["ports"], c["seed"], c["qm"]
    if c["form"] == "compact":
        x = (sm_ints(s + 2, 2 * L * c["n"], -512, 513).astype(np.float32) / np.float32(37)).view(np.complex64)
        return _levels(s, c["n"] * L, qm), x.reshape(L, c["n"]), _weights(s + 1, (P, L), qm)
    masks = case_masks(c)
    nprg = 1 if c["prg_size"] == WIDEBAND else -(-c["nrb"] // c["prg_size"])
    if c["weights"] == "zero":
        w = np.zeros((nprg, P, L), np.complex64)
    elif c["weights"] == "tie":
        w = np.zeros((nprg, P, L), np.complex64)
        w[:, 0, 0] = f32(TIE_DOWN)
        w[:, 1, 0] = f32(TIE_UP)
    else:
        w = _weights(s + 1, (nprg, P, L), qm)
    return _levels(s, int(masks.sum()) * L, qm), w


def run_grid(c, inp) -> np.ndarray:
    """The restatement on a grid case: uint32 [P count], port by port the masked REs in mapping order."""
    masks = case_masks(c)
    grid = np.full((c["ports"], NSYMB, c["nrb"] * NRE), GUARD, np.uint32)
    map_grid(grid, masks, c["prg_size"], inp[1], inp[0])
    assert np.all(grid[:, ~masks] == GUARD)
    return np.ascontiguousarray(grid[:, masks]).reshape(-1)


def run_compact(c, inp):
    """(apply_layer_map_and_precoding, apply_precoding) as uint32 [P n 2] each"""
    return (apply_layer_map_and_precoding(inp[0], inp[2]).view(np.uint32).reshape(-1),
            apply_precoding(inp[1], inp[2]).view(np.uint32).reshape(-1))


def load_fixture():
    """(cases, recorded reference outputs, regenerated inputs); a grid case's output is uint32 [P count], a compact
    one's the pair of uint32 [P n 2]. Every input's SHA-256 must equal the recorded one."""
    d = np.load(GOLDEN, allow_pickle=False)
    cs = json.loads(str(d["index"]))
    off, out = d["off"], d["out"]
    outs, inputs = [], []
    for i, c in enumerate(cs):
        inp = case_input(c)
        assert digest(*inp) == c["sha"], f"ref_precode.npz: the regenerated input of case {i} has another digest"
        inputs.append(inp)
        o = out[int(off[i]):int(off[i + 1])]
        outs.append(o if c["form"] == "grid" else (o[:o.size // 2], o[o.size // 2:]))
    return cs, outs, inputs
