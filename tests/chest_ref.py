"""The PUSCH DM-RS channel estimator's NumPy restatement, its fixture cases and the fixture's loader
(tests/golden/ref_chest.npz, recorded by tests/golden/make_chest_fixtures.py from the compiled reference).

`estimate_plane(...)` restates, for one (rx port, layer) plane, dmrs_pusch_estimator_impl.cpp:71-212 over
port_channel_estimator_average_impl.cpp:215-408, 467-582, 608-720 and interpolator_linear_impl.cpp:32-79:
  pilots: tests/dmrs_ref.py's base_pilots with amplitude (float)M_SQRT1_2 and reference point 0; layer i's are layer
  0's, the odd-indexed ones (along the concatenated allocated RBs) negated for odd i; pilot j of RB n lies on subcarrier
  12 n + 2 j + i / 2;
  prod_s = rx_s conj(x_s) as (ac - b(-d), a(-d) + bc); lse = prod_0, += prod_s in symbol order, times
  1.0F / ((float)nsym scaling);
  EPRE = sum over s of (E_s / n) n, E_s the sequential sum of |rx_s|^2; the CFO dot the sequential sum of
  prod_1 conj(prod_0); RSRP from the sequential sum of |filtered|^2; noise = sum over s of (N_s / n) n, N_s the
  sequential sum of |(filtered (-beta + 0j)) x_s + rx_s|^2; the finals of :257-281;
  smoothing `filter`: every second tap of the 31-tap raised cosine around its centre (5, 11 or 15 for 1, 2, 3 or more
  RBs), normalised by their float32 sum; min(12, taps / 2) virtual pilots per side (6 for 1 RB) from the least-squares
  line through hypotf and the unwrapped atan2f of the outermost true pilots, std::polar; then convolution_same, whose
  outputs at the true pilots are all ((0 + x[m - T/2] y[T-1]) + x[m - T/2 + 1] y[T-2]) + ...;
  interpolation at stride 2 from offset i / 2 as one recurrence; cbf16 by round-to-nearest-even.
Two modes: float32, every operation in the reference's order (the C library's float functions through ctypes, because
NumPy's own float32 sin and cos are not the C library's), and float64.

A case's received grid is, per plane, a smooth channel (a quadratic in the subcarrier, complex coefficients from integer
draws) times the pilots, summed over the layers of a CDM group, plus noise (the sum of four uniform draws, centred: near
enough Gaussian) at the case's SNR, rounded to cbf16; every other RE holds the guard. Only IEEE-exact operations, so a
case is its parameters and a seed. A grid is uint32[port, symbol, subcarrier], one cbf16 element each."""
from __future__ import annotations

import ctypes
import ctypes.util
import json
import math
from pathlib import Path

import numpy as np

from tests import dmrs_ref as D
from tests import precoder_ref as P
from tests.ref_cases import digest
from tests.vectors import sm_unit

NRE = 12
NSYMB = 14
DPR = 6
MAX_V_PILOTS = 12
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_chest.npz"
GUARD = P.GUARD
NONE, FILTER = 0, 1
# The `filter` bound: max |device - file| / max |file| per plane, over the filtered pilots and the interpolated values
# of every `filter` case, measured on the MI355X (profiles/r17/chest_tolerance.json), times 4, rounded up to a power of
# two; never above 2^-16. The device differs from the reference only through hypotf, atan2f and sincosf in at most 24
# virtual pilots per plane.
FILTER_BOUND = 2.0 ** -18
RC_FILTER = [-0.0641253, -0.0660711, -0.0611526, -0.0485918, -0.0281126, 0.0000000, 0.0348830, 0.0751249,
             0.1188406, 0.1637874, 0.2075139, 0.2475302, 0.2814857, 0.3073415, 0.3235207, 0.3290274,
             0.3235207, 0.3073415, 0.2814857, 0.2475302, 0.2075139, 0.1637874, 0.1188406, 0.0751249,
             0.0348830, 0.0000000, -0.0281126, -0.0485918, -0.0611526, -0.0660711, -0.0641253]

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _k in (("hypotf", 2), ("atan2f", 2), ("cosf", 1), ("sinf", 1)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k


class _Math:
    """the four library functions of a mode"""

    def __init__(self, ft):
        self.ft = ft
        if ft is np.float32:
            self.hypot = lambda a, b: np.float32(_libm.hypotf(float(a), float(b)))
            self.atan2 = lambda a, b: np.float32(_libm.atan2f(float(a), float(b)))
            self.cos = lambda a: np.float32(_libm.cosf(float(a)))
            self.sin = lambda a: np.float32(_libm.sinf(float(a)))
        else:
            self.hypot = lambda a, b: np.float64(math.hypot(a, b))
            self.atan2 = lambda a, b: np.float64(math.atan2(a, b))
            self.cos = lambda a: np.float64(math.cos(a))
            self.sin = lambda a: np.float64(math.sin(a))


def seq_sum(x, ft):
    """0 + x[0] + x[1] + ..., one rounding per addition"""
    return np.cumsum(np.asarray(x, ft), dtype=ft)[-1] + ft(0)


def pilots(rbs, layer, l, slot, sid, n_scid):
    """(re, im) float32 [6 len(rbs)]: layer `layer`'s pilots on DM-RS symbol l"""
    re, im = D.base_pilots(1, rbs, 0, D.amplitude_a(1.0), D.c_init(slot, l, sid, n_scid))
    if layer % 2 == 1:
        flip = (np.arange(re.size, dtype=np.uint32) % np.uint32(2)) << np.uint32(31)
        re, im = P.f32(P.bits_of(re) ^ flip), P.f32(P.bits_of(im) ^ flip)
    return re, im


def pilot_subcarriers(rbs, layer):
    rbs = np.asarray(rbs, np.int64)
    return (NRE * rbs[:, None] + 2 * np.arange(DPR)[None, :] + layer // 2).reshape(-1)


def filter_taps(nof_rb, ft=np.float32):
    """filter_type (port_channel_estimator_average_impl.cpp:74-101) at stride 2"""
    stride = 2
    half = (min(nof_rb, 3) * 10 + 1) // 2 // stride
    idx = 31 // 2 - half * stride + stride * np.arange(2 * half + 1)
    taps = np.array(RC_FILTER, np.float32)[idx].astype(ft)
    total = seq_sum(taps, ft)
    return taps * (ft(1) / total)


def nof_virtual_pilots(nof_rb):
    return DPR if nof_rb == 1 else min(MAX_V_PILOTS, filter_taps(nof_rb).size // 2)


def _v_pilots(base_re, base_im, is_start, m):
    """compute_v_pilots over add_v_pilots' abs and unwrapped arg (:651-720, unwrap.cpp:42-73)"""
    ft = m.ft
    nv = base_re.size
    ab = np.array([m.hypot(a, b) for a, b in zip(base_re, base_im)], ft)
    ar = np.array([m.atan2(b, a) for a, b in zip(base_re, base_im)], ft)
    width = ft(np.float32(math.pi))
    k = ft(0)
    for i in range(nv - 1):
        old_a, next_a = ar[i], ar[i + 1]
        ar[i] = old_a + ft(2) * k * width
        jump = next_a - old_a
        if abs(jump) > width:
            k = k - ft(math.copysign(1.0, jump))
    ar[nv - 1] = ar[nv - 1] + ft(2) * k * width
    fnv = ft(nv)
    mean_x = ft(nv * (nv - 1)) / ft(2) / fnv
    norm_x_sq = ft((nv - 1) * nv * (2 * nv - 1)) / ft(6)
    den = norm_x_sq - fnv * mean_x * mean_x
    line = []
    for v in (ab, ar):
        mean = seq_sum(v, ft) / fnv
        dot = ft(0)
        for i in range(nv):
            dot = dot + v[i] * ft(i)
        dot = dot - mean_x * mean * fnv
        dot = dot / den
        line.append((dot, mean - dot * mean_x))
    off = -nv if is_start else nv
    re, im = np.empty(nv, ft), np.empty(nv, ft)
    for i in range(nv):
        iv = ft(i + off)
        rho = line[0][0] * iv + line[0][1]
        theta = line[1][0] * iv + line[1][1]
        re[i], im[i] = rho * m.cos(theta), rho * m.sin(theta)
    return re, im


def smooth(lse_re, lse_im, nof_rb, strategy, m):
    ft = m.ft
    if strategy == NONE:
        return lse_re.copy(), lse_im.copy()
    taps = filter_taps(nof_rb, ft)
    T, nv, n = taps.size, nof_virtual_pilots(nof_rb), lse_re.size
    sr, si = _v_pilots(lse_re[:nv], lse_im[:nv], True, m)
    er, ei = _v_pilots(lse_re[n - nv:], lse_im[n - nv:], False, m)
    xr, xi = np.concatenate([sr, lse_re, er]), np.concatenate([si, lse_im, ei])
    out_re, out_im = np.zeros(n, ft), np.zeros(n, ft)
    for i in range(T):
        lo = nv - T // 2 + i
        out_re = out_re + xr[lo:lo + n] * taps[T - 1 - i]
        out_im = out_im + xi[lo:lo + n] * taps[T - 1 - i]
    return out_re, out_im


def interpolate(in_re, in_im, layer, ft):
    """interpolator_linear_impl.cpp:32-79 with offset layer / 2 and stride 2, onto 2 len(in) values"""
    off, n = layer // 2, in_re.size
    out = []
    for v in (in_re, in_im):
        jump = (v[1:] - v[:-1]) / ft(2)
        steps = np.concatenate([[v[0]], np.repeat(jump, 2)]).astype(ft)
        run = np.cumsum(steps, dtype=ft)                  # out[off], out[off + 1], ..., out[off + 2 (n - 1)]
        o = np.empty(2 * n, ft)
        o[:off] = v[0]
        o[off:off + run.size] = run
        o[off + run.size:] = v[n - 1]
        out.append(o)
    return out[0], out[1]


def symbol_start_epochs(numerology):
    """:454-465, normal cyclic prefix: float32 accumulated through float64 sums"""
    t_c = 1.0 / float(480000 * 4096)
    khz = 15 << numerology
    e = np.zeros(NSYMB, np.float32)
    for i in range(NSYMB):
        cp = (144 >> numerology) + (16 if i == 0 or i == 7 * (1 << numerology) else 0)
        sec = float(cp * 64) * t_c
        e[i] = np.float32(sec * khz * 1000) if i == 0 else np.float32(float(e[i - 1]) + sec * khz * 1000 + 1.0)
    return e


def finals(sums, scaling, dmrs_symbols, numerology, m):
    """:257-281 and :495-497 from (epre_sum, filt_power, noise_sum, dot_re, dot_im, n): epre, rsrp, noise_var, snr,
    cfo_Hz (nan: none)"""
    ft = m.ft
    epre_sum, power, noise_sum, dot_re, dot_im, n = sums
    nsym, fn, beta = len(dmrs_symbols), ft(n), ft(np.float32(scaling))
    pilots_total = n * nsym
    rsrp = ft(power) / fn * fn * beta * beta * ft(nsym)
    rsrp = rsrp / ft(pilots_total)
    epre = ft(epre_sum) / ft(pilots_total)
    noise_var = ft(noise_sum) / ft(pilots_total - 1)
    noise_var = max(rsrp / ft(1e10), noise_var)
    datarp = rsrp / beta / beta
    snr = datarp / noise_var if noise_var != 0 else ft(1000)
    cfo = ft(np.nan)
    if nsym > 1:
        e = symbol_start_epochs(numerology).astype(ft)
        l0, l1 = sorted(dmrs_symbols)[:2]
        twopi = ft(np.float32(2.0) * np.float32(math.pi))
        cfo = m.atan2(ft(dot_im), ft(dot_re)) / twopi / (e[l1] - e[l0])
        cfo = cfo * ft(15 << numerology) * ft(1000)
    return np.array([epre, rsrp, noise_var, snr, cfo], ft)


def estimate_plane(rx, x, scaling, strategy, layer, nof_rb, ft=np.float32, filtered=None):
    """rx, x: per DM-RS symbol (re, im) float32 [6 nof_rb]. Returns a dict: filtered (re, im), interp (re, im), sums
    (epre_sum, filt_power, noise_sum, dot_re, dot_im, n) and terms, the float32 terms behind the five sums. With
    `filtered` (re, im) given, the smoothing is skipped and everything behind it computed from these pilots."""
    m = _Math(ft)
    nsym, n, fn = len(rx), rx[0][0].size, ft(rx[0][0].size)
    beta = ft(np.float32(scaling))
    rx = [(r.astype(ft), i.astype(ft)) for r, i in rx]
    x = [(r.astype(ft), i.astype(ft)) for r, i in x]
    prods, terms = [], dict(epre=[], noise=[])
    for (a, b), (c, d) in zip(rx, x):
        prods.append((a * c - b * (-d), a * (-d) + b * c))
        terms["epre"].append(a * a - b * (-b))
    lse_re, lse_im = prods[0]
    for pr, pi in prods[1:]:
        lse_re, lse_im = lse_re + pr, lse_im + pi
    total_scaling = ft(1) / (ft(nsym) * beta)
    lse_re, lse_im = lse_re * total_scaling, lse_im * total_scaling
    epre_sum = ft(0)
    for s, t in enumerate(terms["epre"]):
        e = seq_sum(t, ft) / fn * fn
        epre_sum = e if s == 0 else epre_sum + e
    dot_re = dot_im = ft(0)
    terms["dot"] = (np.zeros(n, ft), np.zeros(n, ft))
    if nsym > 1:
        (a, b), (c, d) = prods[1], prods[0]
        terms["dot"] = (a * c - b * (-d), a * (-d) + b * c)
        dot_re, dot_im = seq_sum(terms["dot"][0], ft), seq_sum(terms["dot"][1], ft)
    f_re, f_im = smooth(lse_re, lse_im, nof_rb, strategy, m) if filtered is None else (filtered[0].astype(ft),
                                                                                        filtered[1].astype(ft))
    terms["power"] = f_re * f_re - f_im * (-f_im)
    power = seq_sum(terms["power"], ft)
    # sc_prod by cf_t(-beta, 0), then prod with the pilots, add the received, average_power times size
    s_re, s_im = f_re * (-beta) - f_im * ft(0), f_re * ft(0) + f_im * (-beta)
    noise_sum = ft(0)
    for s, ((a, b), (c, d)) in enumerate(zip(rx, x)):
        p_re, p_im = (s_re * c - s_im * d) + a, (s_re * d + s_im * c) + b
        t = p_re * p_re - p_im * (-p_im)
        terms["noise"].append(t)
        e = seq_sum(t, ft) / fn * fn
        noise_sum = e if s == 0 else noise_sum + e
    i_re, i_im = interpolate(f_re, f_im, layer, ft)
    return dict(filtered=(f_re, f_im), interp=(i_re, i_im), terms=terms,
                sums=(epre_sum, power, noise_sum, dot_re, dot_im, n))


# ---- cases ------------------------------------------------------------------------------------------------------------
def _case(seed, strategy, L, nports, nrb, rbs, symbols, first=0, nsymb=14, scaling=1.0, slot=0, sid=0, n_scid=0,
          snr_db=20, rx_ports=None, grid_ports=None, numerology=0, kind="rand"):
    rx_ports = list(range(nports)) if rx_ports is None else list(rx_ports)
    return dict(strategy=strategy, layers=L, ports=nports, nrb=nrb, rbs=[list(x) for x in rbs], symbols=list(symbols),
                first=first, nsymb=nsymb, scaling=float(np.float32(scaling)), slot=slot, id=sid, n_scid=n_scid,
                snr_db=snr_db, rx_ports=rx_ports, grid_ports=max(rx_ports) + 1 if grid_ports is None else grid_ports,
                numerology=numerology, kind=kind, seed=seed)


SQRT2 = float(np.float32(math.sqrt(2.0)))


def cases():
    c = []
    for st in (NONE, FILTER):
        s = 96000 + 100 * st
        c += [
            _case(s + 0, st, 1, 1, 11, [[4, 5]], [2], sid=41),                                  # one RB
            _case(s + 1, st, 1, 2, 11, [[3, 5]], [2, 11], slot=7, sid=1000, n_scid=1, scaling=SQRT2, numerology=1),
            _case(s + 2, st, 2, 1, 11, [[0, 3]], [2, 3], first=2, nsymb=12, slot=3, sid=77),    # three RBs
            _case(s + 3, st, 3, 1, 25, [[5, 14]], [2, 7, 11], slot=9, sid=513, snr_db=30),      # nine RBs
            _case(s + 4, st, 4, 4, 11, [[1, 3]], [2, 11], slot=4, sid=300, scaling=SQRT2, snr_db=25),
            _case(s + 5, st, 1, 1, 52, [[2, 45]], [2, 11], slot=11, sid=29, snr_db=15, numerology=1),         # 43 RBs: 258 pilots
            # a non-contiguous 25-RB mask; rx ports that are not 0 .. P - 1
            _case(s + 6, st, 1, 2, 52, [[1, 9], [12, 13], [20, 36]], [2, 11], first=2, nsymb=12, slot=1, sid=5,
                  rx_ports=[2, 0], grid_ports=4),
            # RBs 270-272 of 273: a sequence jump of two digits; the c_init wrap
            _case(s + 7, st, 2, 1, 273, [[270, 273]], [13], first=11, nsymb=3, slot=159, sid=65535, n_scid=1,
                  numerology=4),
            # a phase that wraps across +-pi inside the edge pilots
            _case(s + 8, st, 1, 1, 11, [[0, 6]], [2, 11], slot=2, sid=1, snr_db=40, kind="wrap"),
            # a plane of all-zero received REs (port 1)
            _case(s + 9, st, 1, 2, 11, [[2, 6]], [2, 11], slot=6, sid=10, kind="zero_port"),
        ]
    # one 273-RB plane at 1 layer on 1 port
    c.append(_case(96300, FILTER, 1, 1, 273, [[0, 273]], [2, 11], slot=13, sid=123, snr_db=25, numerology=1))
    return c


def case_rb_mask(c) -> np.ndarray:
    m = np.zeros(c["nrb"], bool)
    for b, e in c["rbs"]:
        m[b:e] = True
    return m


def _channel(c, k):
    """complex128 [ports, layers, len(k)]: per plane and component a sign times 1 + a quadratic in t = k / (12 nrb) - 1/2
    of at most 0.625, so that no component comes near zero (where a cf32 value is always close to a bf16 midpoint on the
    scale of the plane's largest value: tests/test_gpu_chest.py's cbf16 check)"""
    nports, L = c["ports"], c["layers"]
    u = sm_unit(c["seed"], 8 * nports * L).reshape(nports, L, 2, 4) - 0.5
    sign = np.where(u[..., 0] < 0.0, -1.0, 1.0)
    t = np.asarray(k, np.float64) / float(NRE * c["nrb"]) - 0.5
    comp = sign[..., None] * (1.0 + 0.5 * u[..., 1, None] + u[..., 2, None] * t + u[..., 3, None] * (t * t))
    h = comp[:, :, 0, :] + 1j * comp[:, :, 1, :]
    if c["kind"] == "wrap":
        # on the negative real axis' side, the imaginary part changing sign between the second and third pilot of
        # either end: -0.25, -0.05, 0.15, ... up to 0.55
        kk = np.asarray(k, np.float64)
        d = np.minimum(kk - kk[0], kk[-1] - kk)
        h = np.broadcast_to((-1.0 + 1j * np.minimum(0.1 * d - 0.25, 0.55))[None, None, :], h.shape).copy()
    return h


def case_input(c) -> np.ndarray:
    """the received grid uint32 [grid_ports, NSYMB, 12 nrb] (cbf16), guard outside the DM-RS REs"""
    nsubc = NRE * c["nrb"]
    rbs = np.flatnonzero(case_rb_mask(c))
    grid = np.full((c["grid_ports"], NSYMB, nsubc), GUARD, np.uint32)
    sigma = 10.0 ** (-c["snr_db"] / 20.0) / math.sqrt(2.0) * math.sqrt(3.0)   # unit variance: 4 uniforms have 1 / 3
    for cdm in range((c["layers"] + 1) // 2):
        k = pilot_subcarriers(rbs, 2 * cdm)
        h = _channel(c, k)
        for si, l in enumerate(c["symbols"]):
            tot = np.zeros((c["ports"], k.size), np.complex128)
            for layer in range(2 * cdm, min(2 * cdm + 2, c["layers"])):
                xr, xi = pilots(rbs, layer, l, c["slot"], c["id"], c["n_scid"])
                tot += h[:, layer, :] * (xr.astype(np.float64) + 1j * xi.astype(np.float64))[None, :] * c["scaling"]
            u = sm_unit(c["seed"] + 1000 * (1 + cdm) + si, 8 * c["ports"] * k.size).reshape(2, c["ports"], k.size, 4)
            w = (u.sum(axis=-1) - 2.0) * sigma
            tot = tot + (w[0] + 1j * w[1])
            for p in range(c["ports"]):
                if c["kind"] == "zero_port" and p == 1:
                    tot[p] = 0.0
                grid[c["rx_ports"][p], l, k] = P.to_cbf16(tot[p].real.astype(np.float32), tot[p].imag.astype(np.float32))
    return grid


def grid_pilots(grid, c, p, layer):
    """the received pilots of plane (p, layer) per DM-RS symbol, widened exactly: a list of (re, im) float32"""
    k = pilot_subcarriers(np.flatnonzero(case_rb_mask(c)), layer)
    out = []
    for l in c["symbols"]:
        g = grid[c["rx_ports"][p], l, k]
        out.append((P.f32(g << np.uint32(16)), P.f32(g & np.uint32(0xFFFF0000))))
    return out


def run_case(c, grid, ft=np.float32, filtered=None):
    """The restatement on a case: per plane (layer-major: plane = layer ports + p) estimate_plane's dict with
    `metrics` (finals) added. filtered: per plane (re, im) to take in place of the smoothing's result."""
    rbs = np.flatnonzero(case_rb_mask(c))
    m = _Math(ft)
    out = []
    for layer in range(c["layers"]):
        x = [pilots(rbs, layer, l, c["slot"], c["id"], c["n_scid"]) for l in c["symbols"]]
        for p in range(c["ports"]):
            r = estimate_plane(grid_pilots(grid, c, p, layer), x, c["scaling"], c["strategy"], layer, rbs.size, ft,
                               None if filtered is None else filtered[layer * c["ports"] + p])
            r["metrics"] = finals(r["sums"], c["scaling"], c["symbols"], c["numerology"], m)
            out.append(r)
    return out


def plane_record(r):
    """a plane's recorded words (uint32): filtered pilots (re, im interleaved), interpolated values (interleaved), the
    cbf16 estimates of one symbol, the five metrics (cfo nan: none), the five raw sums"""
    f = np.stack(r["filtered"], axis=-1).astype(np.float32).reshape(-1)
    i = np.stack(r["interp"], axis=-1).astype(np.float32).reshape(-1)
    c16 = P.to_cbf16(r["interp"][0].astype(np.float32), r["interp"][1].astype(np.float32))
    return np.concatenate([P.bits_of(f), P.bits_of(i), c16, P.bits_of(r["metrics"].astype(np.float32)),
                           P.bits_of(np.array(r["sums"][:5], np.float32))])


def split_record(words, n_pilots):
    """plane_record's parts: filtered [n, 2], interp [2 n, 2], cbf16 [2 n], metrics [5], sums [5] (uint32 bits)"""
    n = n_pilots
    at = np.cumsum([0, 2 * n, 4 * n, 2 * n, 5, 5])
    assert words.size == at[-1]
    parts = [words[a:b] for a, b in zip(at[:-1], at[1:])]
    return dict(filtered=parts[0].reshape(n, 2), interp=parts[1].reshape(2 * n, 2), cbf16=parts[2], metrics=parts[3],
                sums=parts[4])


def midpoint_share(interp_bits, bound) -> float:
    """The share of the cf32 components (uint32 bits [n, 2] of one plane) that lie within bound x max |component| of the
    midpoint between two bf16 values: where a deviation of that size may move the cbf16 rounding by one step."""
    bits = np.ascontiguousarray(interp_bits, np.uint32).reshape(-1)
    v = bits.view(np.float32).astype(np.float64)
    top = np.abs(v).max()
    if top == 0.0:
        return 0.0
    expo = ((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    ulp = np.ldexp(1.0, np.maximum(expo, 1) - 127 - 23)
    dist = np.abs((bits & np.uint32(0xFFFF)).astype(np.int64) - 0x8000) * ulp
    return float(np.count_nonzero(dist <= bound * top)) / bits.size


def fixture_classes(cs) -> dict:
    """The classes the fixture must hold: name -> present."""
    def nalloc(c):
        return sum(e - b for b, e in c["rbs"])

    def has(pred):
        return any(pred(c) for c in cs)

    return {
        "both strategies": {c["strategy"] for c in cs} == {NONE, FILTER},
        "1, 2, 3 and 4 layers": {c["layers"] for c in cs} == {1, 2, 3, 4},
        "1, 2 and 4 ports": {c["ports"] for c in cs} >= {1, 2, 4},
        "1, 2, 3, 9 and 43 RBs in both strategies": all(
            {nalloc(c) for c in cs if c["strategy"] == st} >= {1, 2, 3, 9, 43} for st in (NONE, FILTER)),
        "a non-contiguous 25-RB mask": has(lambda c: len(c["rbs"]) > 1 and nalloc(c) == 25),
        "RBs 270-272 of 273": has(lambda c: c["nrb"] == 273 and c["rbs"] == [[270, 273]] and 12 * 270 // 32 > 32),
        "one 273-RB plane at 1 layer on 1 port": has(lambda c: nalloc(c) == 273 and c["layers"] == c["ports"] == 1),
        "DM-RS symbols {2}": has(lambda c: c["symbols"] == [2]),
        "DM-RS symbols {2, 11}": has(lambda c: c["symbols"] == [2, 11]),
        "DM-RS symbols {2, 7, 11}": has(lambda c: c["symbols"] == [2, 7, 11]),
        "DM-RS symbols {2, 3}": has(lambda c: c["symbols"] == [2, 3]),
        "symbols 0/14": has(lambda c: (c["first"], c["nsymb"]) == (0, 14)),
        "symbols 2/12": has(lambda c: (c["first"], c["nsymb"]) == (2, 12)),
        "scaling 1 and sqrt 2": {c["scaling"] for c in cs} >= {1.0, SQRT2},
        "n_scid 1": has(lambda c: c["n_scid"] == 1),
        "the c_init wrap": has(lambda c: (c["slot"], c["id"]) == (159, 65535) and
                               (14 * 159 + max(c["symbols"]) + 1) * (2 * 65535 + 1) * (1 << 17) >= 1 << 32),
        "an rx port list that is not 0 .. P - 1": has(lambda c: c["rx_ports"] != list(range(c["ports"]))),
        "a phase wrap inside the edge pilots": has(lambda c: c["kind"] == "wrap" and c["strategy"] == FILTER),
        "a plane of all-zero received REs": has(lambda c: c["kind"] == "zero_port"),
        "an odd layer": has(lambda c: c["layers"] >= 2),
        "a CDM group of offset 1": has(lambda c: c["layers"] >= 3),
    }


def load_fixture():
    """(cases, per case a list of split_record dicts per plane, regenerated grids). Every grid's SHA-256 must equal the
    recorded one."""
    d = np.load(GOLDEN, allow_pickle=False)
    cs = json.loads(str(d["index"]))
    off, out = d["off"], d["out"]
    outs, grids = [], []
    for i, c in enumerate(cs):
        g = case_input(c)
        assert digest(g) == c["sha"], f"ref_chest.npz: the regenerated grid of case {i} has another digest"
        grids.append(g)
        n = DPR * int(case_rb_mask(c).sum())
        words = out[int(off[i]):int(off[i + 1])].reshape(c["layers"] * c["ports"], -1)
        outs.append([split_record(w, n) for w in words])
    return cs, outs, grids
