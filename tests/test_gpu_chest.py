"""GPU tests of the PUSCH DM-RS channel estimator (ldpc_chest_kernel through ldpc_hip_dmrs_pusch_estimate_launch) against
the compiled reference's recorded outputs (tests/golden/ref_chest.npz) and the NumPy restatement (tests/chest_ref.py):
bit for bit with smoothing `none` and wherever the `filter` path does not pass through the device's hypotf, atan2f and
sincosf; within chest_ref.FILTER_BOUND (profiles/r17/chest_tolerance.json) where it does."""
import ctypes
import functools

import numpy as np
import pytest

from tests import chest_ref as R
from tests import equalizer_ref as E

pytestmark = pytest.mark.gpu

GUARD = R.GUARD
SUM_BOUND = 2.0 ** -19   # a tree over at most 4 x 1,638 non-negative terms is depth 13, plus the term's three
#                          roundings: 16 x 2^-24 = 2^-20; then a factor 2


@functools.lru_cache(maxsize=1)
def _fixture():
    return R.load_fixture()


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.int8, 4: np.int32}[a.dtype.itemsize])).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _config(c):
    from srsran_projectvtlmo_amd import signal_processors as sp
    sym = np.zeros(R.NSYMB, bool)
    sym[c["symbols"]] = True
    return sp.pusch_config_t(c["slot"], c["numerology"], 1, c["id"], bool(c["n_scid"]), c["scaling"], sym,
                             R.case_rb_mask(c), c["first"], c["nsymb"], c["layers"], c["rx_ports"])


def _strategy(c):
    return "filter" if c["strategy"] == R.FILTER else "none"


def _geometry(c):
    nsubc = c["nrb"] * R.NRE
    k = (R.NRE * np.flatnonzero(R.case_rb_mask(c))[:, None] + np.arange(R.NRE)[None, :]).reshape(-1)
    mask = np.zeros((R.NSYMB, nsubc), bool)
    mask[c["first"]:c["first"] + c["nsymb"]][:, k] = True
    return nsubc, k, mask


_DEVICE = {}


def _device(hip_ctx):
    """Every case as its own launch (dmrs_pusch_estimator_hip.estimate), cbf16 and cf32, into guard-filled buffers:
    per case a dict est16 [L, P, 14, nsubc], est32 [L, P, 14, nsubc, 2], pilots [planes, n, 2], records [planes, 8]
    (uint32), computed once for the module."""
    if _DEVICE:
        return _DEVICE["outs"]
    import torch
    from srsran_projectvtlmo_amd import signal_processors as sp
    cases, _, grids = _fixture()
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for c, grid in zip(cases, grids):
        nsubc, _, _ = _geometry(c)
        L, P, n = c["layers"], c["ports"], R.DPR * int(R.case_rb_mask(c).sum())
        shape = (L, P, R.NSYMB, nsubc)
        est = sp.create_dmrs_pusch_estimator_hip_factory(_strategy(c), False, hip_ctx, stream).create()
        d_grid = _cuda(grid)
        d16 = _cuda(np.full(shape, GUARD, np.uint32))
        d32 = _cuda(np.full(shape + (2,), GUARD, np.uint32))
        d_pil = _cuda(np.full((L * P * n + 2, 2), GUARD, np.uint32))
        d_pil32 = _cuda(np.full((L * P * n + 2, 2), GUARD, np.uint32))
        d_rec = _cuda(np.full((L * P + 2, 8), GUARD, np.uint32))
        d_rec32 = _cuda(np.full((L * P + 2, 8), GUARD, np.uint32))
        g = sp.device_grid(d_grid.data_ptr(), (c["grid_ports"], R.NSYMB, nsubc))
        est.estimate(sp.device_channel_estimate(d16.data_ptr(), shape, d_rec.data_ptr(), result_offset=1,
                                                filtered_ptr=d_pil.data_ptr(), pilots_offset=1), g, _config(c))
        est.estimate(sp.device_channel_estimate(d32.data_ptr(), shape, d_rec32.data_ptr(), cf32=True, result_offset=1,
                                                filtered_ptr=d_pil32.data_ptr(), pilots_offset=1), g, _config(c))
        torch.cuda.synchronize()
        pil, rec = _host(d_pil), _host(d_rec)
        # both forms give the same pilots and sums; the guard around them is intact
        assert np.array_equal(pil, _host(d_pil32)) and np.array_equal(rec, _host(d_rec32))
        assert np.all(pil[[0, -1]] == GUARD) and np.all(rec[[0, -1]] == GUARD)
        outs.append(dict(est16=_host(d16).reshape(shape), est32=_host(d32).reshape(shape + (2,)),
                         pilots=pil[1:-1].reshape(L * P, n, 2).copy(), records=rec[1:-1].copy()))
    _DEVICE["outs"] = outs
    return outs


def _guard_kept(c, o):
    _, _, mask = _geometry(c)
    return bool(np.all(o["est16"][:, :, ~mask] == GUARD) and np.all(o["est32"][:, :, ~mask] == GUARD))


def test_strategy_none_equals_the_reference_bit_for_bit(hip_ctx):
    """Estimates in both output forms and the filtered pilots of every `none` case equal the file; every symbol of the
    range holds the same row; nothing else is touched."""
    cases, outs, _ = _fixture()
    bad = []
    for i, (c, planes, o) in enumerate(zip(cases, outs, _device(hip_ctx))):
        if c["strategy"] != R.NONE:
            continue
        _, k, _ = _geometry(c)
        ok = _guard_kept(c, o)
        for pl, rec in enumerate(planes):
            layer, p = divmod(pl, c["ports"])
            for l in range(c["first"], c["first"] + c["nsymb"]):
                ok = ok and np.array_equal(o["est16"][layer, p, l, k], rec["cbf16"])
                ok = ok and np.array_equal(o["est32"][layer, p, l, k], rec["interp"])
            ok = ok and np.array_equal(o["pilots"][pl], rec["filtered"])
        if not ok:
            bad.append(i)
    assert not bad, f"cases that differ from the reference: {bad}"


def _deviation(got_bits, want_bits):
    """max |got - want| / max |want| of two uint32 float32-bit arrays"""
    g, w = got_bits.view(np.float32).astype(np.float64), want_bits.view(np.float32).astype(np.float64)
    top = np.abs(w).max()
    if top == 0.0:
        return 0.0 if np.array_equal(g, w) else float("inf")
    return float(np.abs(g - w).max() / top)


def test_strategy_filter_pilots_and_interpolated_values(hip_ctx):
    """The filtered pilots farther than (taps - 1) / 2 positions from either end are the file's bit for bit; the edge
    pilots and all interpolated cf32 values are within FILTER_BOUND of it, relative to the plane's largest value; each
    cbf16 component is the bf16 rounding of the kernel's own cf32 output."""
    cases, outs, _ = _fixture()
    worst, bad = 0.0, []
    for i, (c, planes, o) in enumerate(zip(cases, outs, _device(hip_ctx))):
        if c["strategy"] != R.FILTER:
            continue
        _, k, _ = _geometry(c)
        half = (R.filter_taps(int(R.case_rb_mask(c).sum())).size - 1) // 2
        ok = _guard_kept(c, o)
        for pl, rec in enumerate(planes):
            layer, p = divmod(pl, c["ports"])
            n = rec["filtered"].shape[0]
            ok = ok and np.array_equal(o["pilots"][pl][half:n - half], rec["filtered"][half:n - half])
            dev = max(_deviation(o["pilots"][pl], rec["filtered"]),
                      _deviation(o["est32"][layer, p, c["first"], k], rec["interp"]))
            worst = max(worst, dev)
            ok = ok and dev <= R.FILTER_BOUND
            own = o["est32"][layer, p, c["first"], k].view(np.float32)
            for l in range(c["first"], c["first"] + c["nsymb"]):
                ok = ok and np.array_equal(o["est32"][layer, p, l, k], o["est32"][layer, p, c["first"], k])
                ok = ok and np.array_equal(o["est16"][layer, p, l, k], R.P.to_cbf16(own[:, 0], own[:, 1]))
        if not ok:
            bad.append(i)
    print(f"chest filter: largest deviation {worst:.3e} = 2^{np.log2(max(worst, 1e-300)):.2f}, bound {R.FILTER_BOUND:.3e}")
    assert not bad, f"cases outside the bound: {bad} (largest deviation {worst:.3e})"


def test_strategy_filter_cbf16(hip_ctx):
    """A cbf16 component differs from the file's only by one bf16 step, and only where the file's cf32 component lies
    within FILTER_BOUND (times the plane's largest value) of the midpoint between two bf16 values; the share of
    components where that is possible is below 1 % in every case."""
    cases, outs, _ = _fixture()
    differing = total = 0
    for c, planes, o in zip(cases, outs, _device(hip_ctx)):
        if c["strategy"] != R.FILTER:
            continue
        _, k, _ = _geometry(c)
        sizes = [rec["interp"].size for rec in planes]
        share = sum(R.midpoint_share(rec["interp"], R.FILTER_BOUND) * n for rec, n in zip(planes, sizes)) / sum(sizes)
        assert share < 0.01, (share, c)
        for pl, rec in enumerate(planes):
            layer, p = divmod(pl, c["ports"])
            got = o["est16"][layer, p, c["first"], k]
            for sh in (0, 16):
                g = ((got >> np.uint32(sh)) & np.uint32(0xFFFF)).astype(np.int64)
                w = ((rec["cbf16"] >> np.uint32(sh)) & np.uint32(0xFFFF)).astype(np.int64)
                diff = g != w
                total += g.size
                if not diff.any():
                    continue
                differing += int(diff.sum())
                # one step of the sign-magnitude code (across zero: 0x0000 and 0x8000 are the same value)
                def code(v):
                    return np.where(v & 0x8000, -(v & 0x7FFF), v & 0x7FFF)
                assert np.all(np.abs(code(g[diff]) - code(w[diff])) <= 1), c
                comp = rec["interp"][:, sh // 16]
                v = comp.view(np.float32).astype(np.float64)
                top = np.abs(rec["interp"].view(np.float32).astype(np.float64)).max()
                expo = ((comp >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
                dist = np.abs((comp & np.uint32(0xFFFF)).astype(np.int64) - 0x8000) * np.ldexp(1.0, np.maximum(expo, 1) - 150)
                assert np.all(dist[diff] <= R.FILTER_BOUND * top), (c, v[diff])
    print(f"chest filter: {differing} of {total} cbf16 components differ from the file")


def _placement(cases):
    """every case as a row of one launch: (rows, per case its offsets and strides, the four buffers' sizes)"""
    from srsran_projectvtlmo_amd import signal_processors as sp
    n = len(cases)
    order = [(5 * j + 2) % n for j in range(n)]
    assert sorted(order) == list(range(n))
    rows, place = sp.chest_rows(), []
    go, eo, po, ro = 1, 2, 3, 1
    for j, i in enumerate(order):
        c = cases[i]
        nsubc, _, _ = _geometry(c)
        L, P, npil = c["layers"], c["ports"], R.DPR * int(R.case_rb_mask(c).sum())
        gss, ess = nsubc + j % 3, nsubc + (j % 4 if j % 2 else 4 * (j % 3))
        gps, eps = R.NSYMB * gss + j % 5, R.NSYMB * ess + (j % 7 if j % 2 else 0)
        eo += (j % 4 - eo) % 4                                                # every residue; 0 takes the 16-byte stores
        rows.add((c["grid_ports"], R.NSYMB, nsubc), (L, P, R.NSYMB, nsubc), _config(c), _strategy(c), grid_offset=go,
                 grid_symbol_stride=gss, grid_port_stride=gps, est_offset=eo, symbol_stride=ess, plane_stride=eps,
                 pilots_offset=po, result_offset=ro)
        place.append((i, go, gss, gps, eo, ess, eps, po, ro))
        go += c["grid_ports"] * gps + 1 + j % 3
        eo += L * P * eps + 1 + j % 4
        po += L * P * npil + 1
        ro += L * P + 1
    assert {e % 4 for _, _, _, _, e, _, _, _, _ in place} == {0, 1, 2, 3}
    assert any(r["est_offset"] % 4 == 0 and r["symbol_stride"] % 4 == 0 and r["plane_stride"] % 4 == 0
               for r in rows.rows), "a row that takes the 16-byte stores"
    return rows, place, (go, eo, po, ro)


@pytest.mark.parametrize("cf32", [False, True])
def test_all_cases_in_one_launch(hip_ctx, cf32):
    """Every case as rows of one launch: topologies and strategies mixed, grid and estimate offsets of every residue
    mod 4, strides above the width, into guard-filled estimate, pilot and result buffers. Every element equals what the
    case's own launch gave and the guard everywhere else; an equal second call reuses the table and changes nothing."""
    import torch
    from srsran_projectvtlmo_amd import signal_processors as sp
    cases, _, grids = _fixture()
    single = _device(hip_ctx)
    rows, place, (go, eo, po, ro) = _placement(cases)
    h_grid = np.full(go + 4, GUARD, np.uint32)
    want = np.full((eo + 8, 2) if cf32 else eo + 8, GUARD, np.uint32)
    want_pil = np.full((po + 4, 2), GUARD, np.uint32)
    want_rec = np.full((ro + 2, 8), GUARD, np.uint32)
    for i, g0, gss, gps, e0, ess, eps, p0, r0 in place:
        c, o = cases[i], single[i]
        nsubc, k, mask = _geometry(c)
        for p in range(c["grid_ports"]):
            for l in range(R.NSYMB):
                at = g0 + p * gps + l * gss
                h_grid[at:at + nsubc] = grids[i][p, l]
        l_idx, k_idx = np.nonzero(mask)
        for pl in range(c["layers"] * c["ports"]):
            layer, p = divmod(pl, c["ports"])
            src = o["est32"] if cf32 else o["est16"]
            want[e0 + pl * eps + l_idx * ess + k_idx] = src[layer, p, l_idx, k_idx]
        npil = o["pilots"].shape[1]
        want_pil[p0:p0 + o["pilots"].shape[0] * npil] = o["pilots"].reshape(-1, 2)
        want_rec[r0:r0 + o["records"].shape[0]] = o["records"]
    d_grid = _cuda(h_grid)
    d_est = _cuda(np.full(want.shape, GUARD, np.uint32))
    d_pil = _cuda(np.full(want_pil.shape, GUARD, np.uint32))
    d_rec = _cuda(np.full(want_rec.shape, GUARD, np.uint32))
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        sp.dmrs_pusch_estimate_launch(hip_ctx, rows, d_grid.data_ptr(), d_est.data_ptr(), d_rec.data_ptr(), stream, cf32,
                                      d_pil.data_ptr())
        torch.cuda.synchronize()
        got = _host(d_est).reshape(want.shape)
        bad = np.flatnonzero((got != want).reshape(want.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{bad.size} estimate elements differ, the first at {bad[:4]}"
        assert np.array_equal(_host(d_pil).reshape(want_pil.shape), want_pil)
        assert np.array_equal(_host(d_rec).reshape(want_rec.shape), want_rec)
        assert np.array_equal(_host(d_grid), h_grid)


def test_raw_sums_against_float64_sums_of_the_float32_terms(hip_ctx):
    """Each raw sum of each plane against the float64 sum of the restatement's float32 terms, the terms computed from
    the kernel's own filtered pilots (the file's, with `none`): the three non-negative sums within 2^-19 relative, the
    CFO dot within 2^-19 x sum |term| per component."""
    cases, _, grids = _fixture()
    dev = _device(hip_ctx)
    worst = 0.0
    for c, grid, o in zip(cases, grids, dev):
        filt = [(pl[:, 0].view(np.float32), pl[:, 1].view(np.float32)) for pl in o["pilots"]]
        for pl, r in enumerate(R.run_case(c, grid, np.float32, filt)):
            rec = o["records"][pl]
            got = rec[:5].view(np.float32).astype(np.float64)
            assert rec[5] == r["sums"][5] and np.all(rec[6:] == 0)
            t = r["terms"]
            want = [sum(float(np.sum(e, dtype=np.float64)) for e in t["epre"]), float(np.sum(t["power"], dtype=np.float64)),
                    sum(float(np.sum(e, dtype=np.float64)) for e in t["noise"])]
            for name, g, w in zip(("epre", "power", "noise"), got[:3], want):
                worst = max(worst, abs(g - w) / w if w > 0.0 else 0.0)
                assert abs(g - w) <= SUM_BOUND * w, (name, g, w, c)
            for q in (0, 1):
                w = float(np.sum(t["dot"][q], dtype=np.float64))
                room = SUM_BOUND * float(np.sum(np.abs(t["dot"][q]), dtype=np.float64))
                assert abs(got[3 + q] - w) <= room, (q, got[3 + q], w, c)
    print(f"chest sums: largest relative deviation of a non-negative sum {worst:.3e} = 2^{np.log2(max(worst, 1e-300)):.2f}")


def test_contract_violations_launch_nothing(hip_ctx):
    """Each LDPC_HIP_EINVAL case returns it and the buffers keep their guard pattern; afterwards a good launch on the
    same buffers succeeds."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import signal_processors as sp
    L = _lib.load()
    cases, outs, grids = _fixture()
    i = next(j for j, c in enumerate(cases) if c["strategy"] == R.NONE and c["layers"] == 4)
    c, grid = cases[i], grids[i]
    nsubc, k, mask = _geometry(c)
    shape = (c["layers"], c["ports"], R.NSYMB, nsubc)
    d_grid = _cuda(grid)
    d_est = _cuda(np.full(shape, GUARD, np.uint32))
    d_pil = _cuda(np.full((16 * 12 + 1, 2), GUARD, np.uint32))
    d_rec = _cuda(np.full((17, 8), GUARD, np.uint32))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or _lib.STREAM_LEGACY)

    def rows(**change):
        r = sp.chest_rows()
        r.add((c["grid_ports"], R.NSYMB, nsubc), shape, _config(c), "none")
        r.rows[0].update(change)
        return r

    def rc(r=None, grid=True, est=True, rec=True, descs=True, mask=True, nm=None, fmt=_lib.SYM_CBF16):
        arr, m = (r or rows()).descriptors()
        return L.ldpc_hip_dmrs_pusch_estimate_launch(
            hip_ctx.handle, 1, arr if descs else None, m.ctypes.data if mask else None, m.size if nm is None else nm,
            ctypes.c_void_p(d_grid.data_ptr()) if grid else None, ctypes.c_void_p(d_est.data_ptr()) if est else None,
            fmt, ctypes.c_void_p(d_pil.data_ptr()), ctypes.c_void_p(d_rec.data_ptr()) if rec else None, stream)

    for t in (0, 2, 255):                                                     # type 2 and anything else
        assert rc(rows(type=t)) == _lib.EINVAL, t
    for ly, po in [(0, 1), (1, 0), (5, 1), (1, 5)]:
        assert rc(rows(nof_layers=ly, nof_rx_ports=po)) == _lib.EINVAL, (ly, po)
    assert rc(rows(strategy=2)) == _lib.EINVAL                                # `mean`
    assert rc(rows(compensate_cfo=1)) == _lib.EINVAL
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert rc(rows(scaling=v)) == _lib.EINVAL, v
    assert rc(rows(symbols_mask=0)) == _lib.EINVAL
    assert rc(rows(symbols_mask=1 << 14)) == _lib.EINVAL                      # outside the slot
    assert rc(rows(first_symbol=3, nof_symbols=11)) == _lib.EINVAL            # DM-RS symbol 2 before the range
    assert rc(rows(nof_symbols=9)) == _lib.EINVAL                             # DM-RS symbol 11 after the range
    assert rc(rows(nof_symbols=0)) == _lib.EINVAL and rc(rows(first_symbol=1)) == _lib.EINVAL  # empty; past symbol 14
    assert rc(rows(symbols_mask=0b111110)) == _lib.EINVAL                     # five DM-RS symbols
    assert rc(rows(width=nsubc - 1)) == _lib.EINVAL                           # 12 nof_rb above the width
    assert rc(rows(symbol_stride=nsubc - 1)) == _lib.EINVAL and rc(rows(grid_symbol_stride=nsubc - 1)) == _lib.EINVAL
    assert rc(rows(grid_port_stride=11 * nsubc + nsubc - 1)) == _lib.EINVAL   # symbol 11's row past the port stride
    assert rc(rows(plane_stride=13 * nsubc + nsubc - 1)) == _lib.EINVAL       # symbol 13's row past the plane stride
    assert rc(rows(est_offset=1 << 48)) == _lib.EINVAL and rc(rows(plane_stride=1 << 62)) == _lib.EINVAL  # a wrap
    assert rc(rows(mask_offset=1)) == _lib.EINVAL and rc(nm=0) == _lib.EINVAL  # the RB mask outside the array
    assert rc(rows(nof_rb=2, width=nsubc)) == _lib.EINVAL                     # RB 2 is set: a bit past nof_rb
    assert rc(rows(scrambling_id=65536)) == _lib.EINVAL and rc(rows(n_scid=2)) == _lib.EINVAL
    assert rc(rows(rx_ports=(0, 1, 2, 4))) == _lib.EINVAL and rc(rows(grid_ports=3)) == _lib.EINVAL
    assert rc(fmt=_lib.SYM_CI8) == _lib.EINVAL and rc(fmt=3) == _lib.EINVAL   # an output format that is neither
    assert rc(grid=False) == _lib.EINVAL and rc(est=False) == _lib.EINVAL and rc(rec=False) == _lib.EINVAL
    assert rc(descs=False) == _lib.EINVAL and rc(mask=False) == _lib.EINVAL
    arr, m = rows().descriptors()
    assert L.ldpc_hip_dmrs_pusch_estimate_launch(None, 1, arr, m.ctypes.data, m.size, ctypes.c_void_p(d_grid.data_ptr()),
                                                 ctypes.c_void_p(d_est.data_ptr()), _lib.SYM_CBF16, None,
                                                 ctypes.c_void_p(d_rec.data_ptr()), None) == _lib.EINVAL
    with pytest.raises(_lib.LdpcHipError):
        sp.dmrs_pusch_estimate_launch(hip_ctx, rows(type=2), d_grid.data_ptr(), d_est.data_ptr(), d_rec.data_ptr(),
                                      stream.value)
    # a transmission with an empty RB mask is skipped
    empty = rows()
    empty.masks[:] = 0
    assert rc(empty) == _lib.OK
    torch.cuda.synchronize()
    assert np.all(_host(d_est) == GUARD) and np.all(_host(d_pil) == GUARD) and np.all(_host(d_rec) == GUARD)
    # the same buffers then take a good launch, here without the filtered pilots
    arr, m = rows().descriptors()
    assert L.ldpc_hip_dmrs_pusch_estimate_launch(hip_ctx.handle, 1, arr, m.ctypes.data, m.size,
                                                 ctypes.c_void_p(d_grid.data_ptr()), ctypes.c_void_p(d_est.data_ptr()),
                                                 _lib.SYM_CBF16, None, ctypes.c_void_p(d_rec.data_ptr()),
                                                 stream) == _lib.OK
    torch.cuda.synchronize()
    got = _host(d_est).reshape(shape)
    for pl, rec in enumerate(outs[i]):
        layer, p = divmod(pl, c["ports"])
        assert np.array_equal(got[layer, p, 5, k], rec["cbf16"])
    assert np.all(got[:, :, ~mask] == GUARD) and np.all(_host(d_pil) == GUARD)
    recs = _host(d_rec).reshape(17, 8)
    assert np.all(recs[16:] == GUARD) and np.all(recs[:16, 5] == 12) and np.all(recs[:16, 6:] == 0)


def test_capture_with_the_equalizer_in_one_graph(hip_ctx):
    """dmrs_pusch_estimate_launch and equalize_launch on one stream, eager, then captured in one graph and replayed
    twice with a changed received grid: the estimates follow the grid, and the equalizer reads them in place through
    est_offset / est_stride on a one-symbol, all-data-RE segment. Smoothing `none`, so every value is the
    restatements' bit for bit."""
    import torch
    from srsran_projectvtlmo_amd import equalization as eq
    from srsran_projectvtlmo_amd import signal_processors as sp
    base = dict(R.cases()[4], strategy=R.NONE, layers=2, ports=2, rx_ports=[0, 1], grid_ports=2, nrb=11,
                rbs=[[2, 7]], kind="rand")
    nsubc, k, _ = _geometry(base)
    L, P, l_data = 2, 2, 5
    shape = (L, P, R.NSYMB, nsubc)
    grids = []
    for seed in (97001, 97002, 97003):
        c = dict(base, seed=seed)
        g = R.case_input(c)
        # data REs on symbol l_data: bf16 patterns of moderate size
        b = E._bf16(seed, (P, nsubc, 2), 120, 130).astype(np.uint32)
        g[:, l_data, :] = b[..., 0] | (b[..., 1] << np.uint32(16))
        grids.append(g)
    nv = [0.01, 0.02]
    rows = sp.chest_rows()
    rows.add((P, R.NSYMB, nsubc), shape, _config(base), "none")
    seg = eq.eq_segment(k.size, P, L, nv, eq.channel_equalizer_algorithm_type.zf, 1.0, sym_offset=l_data * nsubc + k[0],
                        est_offset=l_data * nsubc + k[0], sym_stride=R.NSYMB * nsubc, est_stride=R.NSYMB * nsubc)
    d_grid = _cuda(grids[0])
    d_est = _cuda(np.full(shape, GUARD, np.uint32))
    d_rec = _cuda(np.zeros((L * P, 8), np.uint32))
    d_sym = torch.zeros((k.size * L, 2), dtype=torch.float32, device="cuda")
    d_var = torch.zeros(k.size * L, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def launch():
        sp.dmrs_pusch_estimate_launch(hip_ctx, rows, d_grid.data_ptr(), d_est.data_ptr(), d_rec.data_ptr(),
                                      st.cuda_stream)
        eq.equalize_launch(hip_ctx, [seg], d_grid.data_ptr(), d_est.data_ptr(), d_sym.data_ptr(), d_var.data_ptr(),
                           st.cuda_stream)

    def expect(g):
        r = R.run_case(base, g)
        est = np.stack([R.P.to_cbf16(*pl["interp"]) for pl in r]).reshape(L, P, -1)
        est16 = np.stack([est & np.uint32(0xFFFF), est >> np.uint32(16)], axis=-1).astype(np.uint16)
        sym = g[:, l_data, k]
        sym16 = np.stack([sym & np.uint32(0xFFFF), sym >> np.uint32(16)], axis=-1).astype(np.uint16)
        s, v = E.equalize(0, sym16, est16, np.array(nv, np.float32), np.float32(1.0))
        return est, np.ascontiguousarray(s, np.complex64).view(np.uint32), E.bits_of(v)

    def check(g, what):
        est, s, v = expect(g)
        got = _host(d_est).reshape(shape)
        assert np.array_equal(got[:, :, l_data, k], est), what
        assert np.array_equal(_host(d_sym).reshape(-1), s) and np.array_equal(_host(d_var), v), what

    launch()
    st.synchronize()
    check(grids[0], "eager")
    lib, graph = hip_ctx.lib, ctypes.c_void_p()
    assert lib.ldpc_hip_capture_begin(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream)) == 0
    launch()
    assert lib.ldpc_hip_capture_end(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream), ctypes.byref(graph)) == 0
    for j in (1, 2):
        d_grid.copy_(_cuda(grids[j]))
        torch.cuda.synchronize()
        assert lib.ldpc_hip_graph_launch(graph, ctypes.c_void_p(st.cuda_stream)) == 0
        st.synchronize()
        check(grids[j], f"replay {j}")
    lib.ldpc_hip_graph_destroy(graph)


def test_275_rbs_against_the_restatement(hip_ctx):
    """The widest RB mask the launch accepts, every RB allocated (the fixture's widest case has 273): smoothing `none`
    against the restatement bit for bit, estimates, filtered pilots and pilot count; the guard elsewhere."""
    import torch
    from srsran_projectvtlmo_amd import signal_processors as sp
    c = dict(R.cases()[0], strategy=R.NONE, nrb=275, rbs=[[0, 275]], symbols=[2, 11], seed=97100)
    grid = R.case_input(c)
    nsubc, k, mask = _geometry(c)
    shape, n = (1, 1, R.NSYMB, nsubc), R.DPR * 275
    d_grid = _cuda(grid)
    d_est = _cuda(np.full(shape + (2,), GUARD, np.uint32))
    d_pil = _cuda(np.full((n + 2, 2), GUARD, np.uint32))
    d_rec = _cuda(np.full((3, 8), GUARD, np.uint32))
    est = sp.create_dmrs_pusch_estimator_hip_factory("none", False, hip_ctx,
                                                     torch.cuda.current_stream().cuda_stream).create()
    est.estimate(sp.device_channel_estimate(d_est.data_ptr(), shape, d_rec.data_ptr(), cf32=True, result_offset=1,
                                            filtered_ptr=d_pil.data_ptr(), pilots_offset=1),
                 sp.device_grid(d_grid.data_ptr(), (1, R.NSYMB, nsubc)), _config(c))
    torch.cuda.synchronize()
    want = R.split_record(R.plane_record(R.run_case(c, grid)[0]), n)
    got, pil, rec = _host(d_est).reshape(shape + (2,)), _host(d_pil), _host(d_rec)
    for l in range(R.NSYMB):
        assert np.array_equal(got[0, 0, l, k], want["interp"]), l
    assert np.array_equal(pil[1:-1], want["filtered"]) and np.all(pil[[0, -1]] == GUARD)
    assert rec[1, 5] == n and np.all(rec[[0, 2]] == GUARD) and np.all(got[:, :, ~mask] == GUARD)
