"""The PDSCH DM-RS generator's NumPy restatement, its fixture cases and the fixture's loader (tests/golden/ref_dmrs.npz,
recorded by tests/golden/make_dmrs_fixtures.py from the compiled reference).

`dmrs_values(...)` restates dmrs_pdsch_processor_impl.cpp:84-262 over dmrs_helper.h:44-109,
pseudo_random_generator_impl.cpp:154-246 and resource_grid_mapper_impl.cpp:47-147, 165-291:
  on DM-RS symbol l the sequence of c_init = ((14 slot + l + 1) (2 id + 1) 2^17 + 2 id + n_scid) mod 2^31 (exact
  integer); pilot j (0 <= j < dpr; dpr = 6 for type 1, 4 for type 2) of resource block n uses the sequence bits
  b = 2 (dpr (n - reference_point_k_rb) + j) and b + 1, whatever the rest of the RB mask; its value is a with the sign
  bit of Re XORed with c(b) and that of Im with c(b + 1), a = float32(M_SQRT1_2 * float64(amplitude));
  DM-RS port i is layer i in CDM group i / 2, on subcarriers 2 j + g (type 1) or {2 g, 2 g + 1, 6 + 2 g, 7 + 2 g}
  (type 2) of the RB; an odd port's odd-j pilots have both sign bits flipped;
  per CDM group the precoder's arithmetic on its one or two layers (tests/precoder_ref.py's precode) with the weight
  matrix [port][layer] of the one PRG, then cbf16 (to_cbf16); one layer on one port with a weight equal to 1 stores the
  pilots as they are.

Weights come from integer draws only (tests/vectors.py's splitmix64), so a case is its parameters and a seed. A grid is
uint32[port, symbol, subcarrier], one cbf16 element each; the values before the rounding are uint32[..., 2], the bits of
(float32 re, float32 im)."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from tests import precoder_ref as P
from tests import scrambling_ref as S
from tests.ref_cases import digest

NRE = 12
NSYMB = 14
TOPOLOGIES = P.TOPOLOGIES
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_dmrs.npz"
GUARD = P.GUARD
SQRT1_2 = 0.70710678118654752440  # M_SQRT1_2


def c_init(slot: int, l: int, scrambling_id: int, n_scid: int) -> int:
    return ((14 * slot + l + 1) * (2 * scrambling_id + 1) * (1 << 17) + 2 * scrambling_id + n_scid) % (1 << 31)


def dpr_of(dmrs_type: int) -> int:
    return 6 if dmrs_type == 1 else 4


def pilot_subcarriers(dmrs_type: int, g: int) -> np.ndarray:
    """the subcarriers of CDM group g's pilots j = 0 .. dpr - 1 inside a resource block"""
    if dmrs_type == 1:
        return 2 * np.arange(6) + g
    return np.array([2 * g, 2 * g + 1, 6 + 2 * g, 7 + 2 * g])


def amplitude_a(amplitude) -> np.float32:
    return np.float32(SQRT1_2 * float(np.float32(amplitude)))


def base_pilots(dmrs_type, rbs, ref_rb, a, cinit):
    """(re, im) float32 [len(rbs) dpr]: the pilots of the resource blocks `rbs` (ascending) before any CDM code"""
    dpr = dpr_of(dmrs_type)
    rbs = np.asarray(rbs, np.int64)
    assert rbs.size and rbs.min() >= ref_rb, "an RB below the reference point is a contract violation"
    seq = S.sequence(cinit, 0, 2 * dpr * (int(rbs.max()) - ref_rb + 1)).astype(np.uint32)
    b = 2 * (dpr * (rbs[:, None] - ref_rb) + np.arange(dpr)[None, :]).reshape(-1)
    au = np.uint32(np.float32(a).view(np.uint32))
    return P.f32(au ^ (seq[b] << np.uint32(31))), P.f32(au ^ (seq[b + 1] << np.uint32(31)))


def is_bypass(w) -> bool:
    """resource_grid_mapper_impl.cpp:94-95, 230-231: one layer, one port, one PRG and the coefficient == 1.0F"""
    w = np.ascontiguousarray(w, np.complex64)
    return w.shape == (1, 1) and w[0, 0] == np.complex64(1.0)


def dmrs_values(dmrs_type, rb_mask, ref_rb, symbols, slot, scrambling_id, n_scid, amplitude, w):
    """The DM-RS REs of one transmission before the cbf16 conversion: a list of (l, k int64 [count], re float32
    [P, count], im) per DM-RS symbol and CDM group. w complex64 [P, L]."""
    w = np.ascontiguousarray(w, np.complex64)
    nports, L = w.shape
    rbs = np.flatnonzero(np.asarray(rb_mask, bool))
    dpr = dpr_of(dmrs_type)
    a = amplitude_a(amplitude)
    wr, wi = P._parts(w)
    flip = np.tile((np.arange(dpr) % 2).astype(np.uint32) << np.uint32(31), rbs.size)
    out = []
    for l in symbols:
        xr, xi = base_pilots(dmrs_type, rbs, ref_rb, a, c_init(slot, l, scrambling_id, n_scid))
        for g in range((L + 1) // 2):
            lg = min(2, L - 2 * g)
            k = (NRE * rbs[:, None] + pilot_subcarriers(dmrs_type, g)[None, :]).reshape(-1)
            lr, li = [xr], [xi]
            if lg == 2:  # the group's second port: w_f = {+1, -1}
                lr.append(P.f32(P.bits_of(xr) ^ flip))
                li.append(P.f32(P.bits_of(xi) ^ flip))
            if is_bypass(w):
                re, im = xr[None, :].copy(), xi[None, :].copy()
            else:
                re, im = P.precode(np.stack(lr), np.stack(li), np.ascontiguousarray(wr[:, 2 * g:2 * g + lg]),
                                   np.ascontiguousarray(wi[:, 2 * g:2 * g + lg]))
            out.append((l, k, re, im))
    return out


def map_dmrs(grid, pre, *args) -> int:
    """Writes one transmission's DM-RS into grid (uint32 [port, symbol, subcarrier], cbf16) and, when given, the bits
    of the values before the rounding into pre (uint32 [port, symbol, subcarrier, 2]); args as dmrs_values. Returns
    the REs written per port."""
    count = 0
    for l, k, re, im in dmrs_values(*args):
        for p in range(re.shape[0]):
            if grid is not None:
                grid[p, l, k] = P.to_cbf16(re[p], im[p])
            if pre is not None:
                pre[p, l, k, 0] = P.bits_of(re[p])
                pre[p, l, k, 1] = P.bits_of(im[p])
        count += k.size
    return count


# ---- cases ------------------------------------------------------------------------------------------------------------
def _case(seed, dmrs_type, L, nports, nrb, rbs, symbols, ref=0, slot=0, sid=0, n_scid=0, amplitude=1.0, weights="rand",
          grid_ports=None):
    return dict(type=dmrs_type, layers=L, ports=nports, grid_ports=nports if grid_ports is None else grid_ports,
                nrb=nrb, rbs=[list(x) for x in rbs], ref=ref, symbols=list(symbols), slot=slot, id=sid, n_scid=n_scid,
                amplitude=float(np.float32(amplitude)), weights=weights, seed=seed)


def cases():
    c = []
    for t in (1, 2):
        s = 95000 + 100 * t
        c += [
            # the identity bypass at amplitude 0: (-0, -0) where both sequence bits are set
            _case(s + 0, t, 1, 1, 11, [[0, 11]], [2], sid=41, amplitude=0.0, weights="identity"),
            # nine consecutive RBs (type 1: every residue of the bit offset mod 32); adjacent DM-RS symbols
            _case(s + 1, t, 1, 2, 25, [[3, 12]], [2, 3], slot=7, sid=1000, n_scid=1),
            # non-contiguous, the reference point above 0 and the first RB above it; grid ports above P
            _case(s + 2, t, 1, 3, 13, [[2, 3], [5, 8], [10, 13]], [2], ref=1, slot=3, sid=77, amplitude=0.75,
                  grid_ports=4),
            # one RB
            _case(s + 3, t, 1, 4, 11, [[7, 8]], [2, 11], slot=19, sid=65535, amplitude=1.4125375),
            # a full 25-RB grid on symbols {2, 11}
            _case(s + 4, t, 2, 2, 25, [[0, 25]], [2, 11], slot=9, sid=513, n_scid=1, amplitude=1.4125375),
            # the c_init wrap: slot 159, symbol 13, id 65535, n_scid 1
            _case(s + 5, t, 2, 3, 11, [[1, 6]], [13], slot=159, sid=65535, n_scid=1, grid_ports=4),
            # RB 274 of a 275-RB grid (sequence words above 32: a jump of two digits), several blocks, few RBs set
            _case(s + 6, t, 2, 4, 275, [[3, 4], [140, 142], [274, 275]], [3], slot=11, sid=29, amplitude=0.5),
            # a zero weight
            _case(s + 7, t, 3, 3, 11, [[0, 4], [6, 11]], [2], slot=1, sid=5, weights="zero"),
            # contiguous from above a reference point above 0; adjacent DM-RS symbols
            _case(s + 8, t, 3, 4, 24, [[4, 16]], [2, 3], ref=2, slot=4, sid=300),
            _case(s + 9, t, 4, 4, 17, [[0, 17]], [2], slot=2, sid=1, n_scid=1, amplitude=0.5),
        ]
    c += [
        # one layer on one port without the bypass, and with it at an amplitude where it changes nothing
        _case(95300, 1, 1, 1, 11, [[2, 9]], [2], slot=5, sid=9, amplitude=0.75, grid_ports=2),
        _case(95301, 2, 1, 1, 11, [[2, 9]], [5], slot=5, sid=9, amplitude=0.75),
        _case(95302, 1, 1, 1, 12, [[1, 12]], [2, 7], slot=6, sid=10, weights="identity"),
        # 1 - 0j compares equal to 1: the bypass, which shows at amplitude -0
        _case(95303, 2, 1, 1, 11, [[0, 7]], [2], slot=8, sid=12, amplitude=-0.0, weights="identity_negzero"),
        # amplitude 0 through the multiply: never (-0, -0) from (1 + 0j)-like weights on two ports
        _case(95304, 1, 1, 2, 11, [[0, 6]], [2], slot=8, sid=12, amplitude=0.0, weights="ones"),
    ]
    return c


def case_rb_mask(c) -> np.ndarray:
    m = np.zeros(c["nrb"], bool)
    for b, e in c["rbs"]:
        m[b:e] = True
    return m


def case_input(c) -> np.ndarray:
    """weights complex64 [P, L]"""
    L, nports = c["layers"], c["ports"]
    kind = c["weights"]
    if kind == "identity":
        return np.ones((1, 1), np.complex64)
    if kind == "identity_negzero":
        return np.array([[complex(1.0, -0.0)]], np.complex64)
    if kind == "ones":
        return np.ones((nports, L), np.complex64)
    w = P._weights(c["seed"], (nports, L), 2)
    if kind == "zero":
        w[0, 0] = 0
        w[nports - 1, L - 1] = complex(-0.0, 0.0)
    return w


def case_args(c, w):
    return (c["type"], case_rb_mask(c), c["ref"], c["symbols"], c["slot"], c["id"], c["n_scid"], c["amplitude"], w)


def case_mask(c) -> np.ndarray:
    """bool [NSYMB, 12 nrb]: the REs the transmission's CDM groups occupy"""
    m = np.zeros((NSYMB, c["nrb"] * NRE), bool)
    rbs = np.flatnonzero(case_rb_mask(c))
    for g in range((c["layers"] + 1) // 2):
        k = (NRE * rbs[:, None] + pilot_subcarriers(c["type"], g)[None, :]).reshape(-1)
        for l in c["symbols"]:
            m[l, k] = True
    return m


def run_case(c, w):
    """The restatement on a case: (cbf16 uint32 [P count], bits before the rounding uint32 [P count 2]), port by port
    the DM-RS REs in ascending (symbol, subcarrier) order; everything else must still hold the guard."""
    shape = (c["grid_ports"], NSYMB, c["nrb"] * NRE)
    grid, pre = np.full(shape, GUARD, np.uint32), np.full(shape + (2,), GUARD, np.uint32)
    count = map_dmrs(grid, pre, *case_args(c, w))
    mask = case_mask(c)
    assert count == int(mask.sum())
    assert np.all(grid[:c["ports"]][:, ~mask] == GUARD) and np.all(grid[c["ports"]:] == GUARD)
    assert np.all(pre[:c["ports"]][:, ~mask] == GUARD) and np.all(pre[c["ports"]:] == GUARD)
    return (np.ascontiguousarray(grid[:c["ports"]][:, mask]).reshape(-1),
            np.ascontiguousarray(pre[:c["ports"]][:, mask]).reshape(-1))


def fixture_classes(cs, outs) -> dict:
    """The classes the fixture must hold, each the smallest shape at which the kernel can go wrong: name -> present.
    outs as load_fixture gives them."""
    def runs(c):  # lengths of the runs of consecutive allocated RBs
        return [e - b for b, e in c["rbs"]]

    def contiguous(c):
        return len(c["rbs"]) == 1

    def first(c):
        return c["rbs"][0][0]

    topo = {t: {(c["layers"], c["ports"]) for c in cs if c["type"] == t} for t in (1, 2)}
    return {
        "both types": {c["type"] for c in cs} == {1, 2},
        "all ten topologies in type 1": topo[1] == set(TOPOLOGIES),
        "all ten topologies in type 2": topo[2] == set(TOPOLOGIES),
        "a contiguous RB mask": any(contiguous(c) for c in cs),
        "a non-contiguous RB mask": any(not contiguous(c) for c in cs),
        "a one-RB allocation": any(sum(runs(c)) == 1 for c in cs),
        "reference_point_k_rb of 0": any(c["ref"] == 0 for c in cs),
        "reference_point_k_rb above 0 with the first RB above it": any(0 < c["ref"] < first(c) for c in cs),
        "at least 9 consecutive RBs in type 1": any(c["type"] == 1 and max(runs(c)) >= 9 for c in cs),
        "at least 5 consecutive RBs in type 2": any(c["type"] == 2 and max(runs(c)) >= 5 for c in cs),
        "RB 274 of a 275-RB grid with few RBs set": any(
            c["nrb"] == 275 and c["rbs"][-1][1] == 275 and sum(runs(c)) <= 8 and
            2 * dpr_of(c["type"]) * (274 - c["ref"]) // 32 > 32 for c in cs),
        "adjacent DM-RS symbols {2, 3}": any(c["symbols"] == [2, 3] for c in cs),
        "DM-RS symbols {2, 11}": any(c["symbols"] == [2, 11] for c in cs),
        "the c_init wrap case": any(
            (c["slot"], c["symbols"], c["id"], c["n_scid"]) == (159, [13], 65535, 1) and
            (14 * 159 + 14) * (2 * 65535 + 1) * (1 << 17) >= 1 << 32 for c in cs),
        "grid ports above P": any(c["grid_ports"] > c["ports"] for c in cs),
        "the identity bypass at amplitude 0.0 showing 0x80008000": any(
            c["weights"] == "identity" and c["amplitude"] == 0.0 and (o[0] == 0x80008000).any() and
            set(o[0].tolist()) == {0x00000000, 0x00008000, 0x80000000, 0x80008000} for c, o in zip(cs, outs)),
        "amplitude 0.0 through the multiply never showing 0x80008000": any(
            c["weights"] == "ones" and c["amplitude"] == 0.0 and not (o[0] == 0x80008000).any() and
            (o[0] == 0x00008000).any() for c, o in zip(cs, outs)),
        "a zero weight": any(c["weights"] == "zero" for c in cs),
        "amplitudes other than 1": len({c["amplitude"] for c in cs} - {1.0, 0.0}) >= 2,
        "a row of more than one block": any(c["rbs"][-1][1] - first(c) > 128 for c in cs),
    }


def load_fixture():
    """(cases, recorded reference outputs, regenerated weights); a case's output is the pair (cbf16 uint32 [P count],
    bits before the rounding uint32 [P count 2]). Every input's SHA-256 must equal the recorded one."""
    d = np.load(GOLDEN, allow_pickle=False)
    cs = json.loads(str(d["index"]))
    off, out = d["off"], d["out"]
    outs, inputs = [], []
    for i, c in enumerate(cs):
        w = case_input(c)
        assert digest(w) == c["sha"], f"ref_dmrs.npz: the regenerated weights of case {i} have another digest"
        inputs.append(w)
        o = out[int(off[i]):int(off[i + 1])]
        outs.append((o[:o.size // 3], o[o.size // 3:]))
    return cs, outs, inputs
