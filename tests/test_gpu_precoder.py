"""GPU tests of the precoder (ldpc_precode_kernel through ldpc_hip_precode_sync / ldpc_hip_precode_map_launch): bit for
bit against the compiled reference's recorded outputs (tests/golden/ref_precode.npz) and against the NumPy restatement
(tests/precoder_ref.py)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
from tests import modulation_ref as M
from tests import precoder_ref as R
from tests import scrambling_ref as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _fixture():
    return R.load_fixture()


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.int8, 4: np.int32}[a.dtype.itemsize])).cuda()


def _launch(ctx, rows, d_sym, d_grid):
    import torch
    from srsran_projectvtlmo_amd import precoding as pc
    pc.precode_map_launch(ctx, rows, d_sym.data_ptr(), d_grid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_grid.cpu().numpy().view(np.uint32)


def test_every_fixture_case_sync(hip_ctx):
    """The compact cases through both channel_precoder methods; the grid cases PRG by PRG through
    apply_layer_map_and_precoding, converted to cbf16 here."""
    from srsran_projectvtlmo_amd import precoding as pc
    cases, outs, inputs = _fixture()
    prec = pc.create_channel_precoder_hip_factory(hip_ctx).create()
    bad = []
    for i, (c, o, inp) in enumerate(zip(cases, outs, inputs)):
        L, P = c["layers"], c["ports"]
        if c["form"] == "compact":
            a, b = np.empty((P, c["n"]), np.complex64), np.empty((P, c["n"]), np.complex64)
            prec.apply_layer_map_and_precoding(a, inp[0], inp[2])
            prec.apply_precoding(b, inp[1], inp[2])
            ok = np.array_equal(a.view(np.uint32).reshape(-1), o[0]) and \
                np.array_equal(b.view(np.uint32).reshape(-1), o[1])
        else:
            _, k_idx = np.nonzero(R.case_masks(c))
            prg = k_idx // (R.NRE * c["prg_size"])
            sym = inp[0].reshape(-1, L, 2)
            got = np.empty((P, k_idx.size), np.uint32)
            for g in np.unique(prg):
                sel = prg == g
                out = np.empty((P, int(sel.sum())), np.complex64)
                prec.apply_layer_map_and_precoding(out, sym[sel].reshape(-1, 2), inp[1][g])
                got[:, sel] = R.to_cbf16(np.ascontiguousarray(out.real), np.ascontiguousarray(out.imag))
            ok = np.array_equal(got.reshape(-1), o)
        if not ok:
            bad.append(i)
    assert not bad, f"cases that differ from the reference: {bad}"


def test_every_fixture_case_grid(hip_ctx):
    """Each grid case as its own launch into a guard-filled grid; each compact case's ci8 input as one all-masked row
    of n subcarriers, against the recorded cf32 outputs converted to cbf16."""
    from srsran_projectvtlmo_amd import precoding as pc
    cases, outs, inputs = _fixture()
    bad = []
    for i, (c, o, inp) in enumerate(zip(cases, outs, inputs)):
        P = c["ports"]
        rows = pc.precode_rows()
        if c["form"] == "grid":
            masks, shape = R.case_masks(c), (P, R.NSYMB, c["nrb"] * R.NRE)
            rows.add(shape, masks, c["prg_size"], inp[1])
            want = o
        else:
            masks, shape = np.ones((1, c["n"]), bool), (P, 1, c["n"])
            rows.add(shape, masks, R.WIDEBAND, inp[2][None])
            f = o[0].view(np.float32).reshape(P, c["n"], 2)
            want = R.to_cbf16(f[:, :, 0], f[:, :, 1]).reshape(-1)
        grid = _launch(hip_ctx, rows, _cuda(inp[0]), _cuda(np.full(shape, R.GUARD, np.uint32))).reshape(shape)
        if not (np.array_equal(grid[:, masks].reshape(-1), want) and np.all(grid[:, ~masks] == R.GUARD)):
            bad.append(i)
    assert not bad, f"cases that differ from the reference: {bad}"


def test_all_grid_cases_in_one_launch(hip_ctx):
    """Every grid case as rows of one launch into one buffer: topologies mixed, odd symbol offsets (misaligned ci8
    loads), grid offsets of every residue, symbol and port strides above the width, and a guard pattern that must
    survive everywhere outside the masks."""
    from srsran_projectvtlmo_amd import precoding as pc
    cases, outs, inputs = _fixture()
    idx = [i for i, c in enumerate(cases) if c["form"] == "grid"]
    order = [idx[(5 * k + 3) % len(idx)] for k in range(len(idx))]            # 5 and 13 are coprime
    assert sorted(order) == idx
    rows, place = pc.precode_rows(), []
    so, go = 1, 3
    for k, i in enumerate(order):
        c = cases[i]
        P, nsubc = c["ports"], c["nrb"] * R.NRE
        sstride = nsubc + 1 + k % 4
        pstride = R.NSYMB * sstride + 1 + k % 3
        n = rows.add((P, R.NSYMB, nsubc), R.case_masks(c), c["prg_size"], inputs[i][1], sym_offset=so, grid_offset=go,
                     symbol_stride=sstride, port_stride=pstride)
        place.append((i, so, go, sstride, pstride))
        so += n * c["layers"] + 1 + 2 * (k % 2)                               # odd and even gaps: every 4-byte phase
        go += P * pstride + 1 + k % 5
    h_sym = np.full((so + 8, 2), 85, np.int8)
    for i, s, *_ in place:
        h_sym[s:s + inputs[i][0].shape[0]] = inputs[i][0]
    want = np.full(go + 8, R.GUARD, np.uint32)
    for i, _, g, sstride, pstride in place:
        c, masks = cases[i], R.case_masks(cases[i])
        l_idx, k_idx = np.nonzero(masks)
        o = outs[i].reshape(c["ports"], -1)
        for p in range(c["ports"]):
            want[g + p * pstride + l_idx * sstride + k_idx] = o[p]
    d_sym = _cuda(h_sym)
    got = _launch(hip_ctx, rows, d_sym, _cuda(np.full(go + 8, R.GUARD, np.uint32)))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} grid elements differ, the first at {bad[:4]}"
    assert np.array_equal(d_sym.cpu().numpy(), h_sym)


def test_contract_violations_launch_nothing(hip_ctx):
    """Each LDPC_HIP_EINVAL case returns it; the grid keeps its guard pattern."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import precoding as pc
    L = _lib.load()
    nsubc = 132
    d_sym = torch.ones(4 * nsubc * 2, dtype=torch.int8, device="cuda")
    d_grid = _cuda(np.full(4 * nsubc, R.GUARD, np.uint32))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream or _lib.STREAM_LEGACY)
    masks = np.zeros((1, nsubc), bool)
    masks[0, 12:60] = True                                                    # PRBs 1 to 4: PRGs 0 and 1 of size 4

    def rows(w=None, **change):
        r = pc.precode_rows()
        r.add((4, 1, nsubc), masks, 4, np.ones((2, 4, 2), np.complex64) if w is None else w)
        r.rows[0].update(change)
        return r

    def rc(r=None, ptrs=(0, 1), descs=True, weights=True, mask=True, nw=None, nm=None):
        arr, w, m = (r or rows()).descriptors()
        p = [ctypes.c_void_p(q) if i in ptrs else None for i, q in enumerate((d_sym.data_ptr(), d_grid.data_ptr()))]
        return L.ldpc_hip_precode_map_launch(hip_ctx.handle, 1, arr if descs else None,
                                             w.ctypes.data if weights else None, w.size // 2 if nw is None else nw,
                                             m.ctypes.data if mask else None, m.size if nm is None else nm, *p, stream)

    for ly, po in [(0, 1), (1, 0), (2, 1), (3, 2), (4, 3), (1, 5), (5, 5), (0, 0)]:  # outside the ten
        assert rc(rows(nof_layers=ly, nof_ports=po)) == _lib.EINVAL, (ly, po)
    for v in (float("inf"), float("-inf"), float("nan"), 2.0 ** 64, -2.0 ** 64):      # a refused weight, re or im
        for z in (complex(v, 0), complex(0, v)):
            w = np.ones((2, 4, 2), np.complex64)
            w[1, 3, 1] = z
            assert rc(rows(w)) == _lib.EINVAL, z
    assert rc(rows(nof_prg=1)) == _lib.EINVAL                                 # subcarrier 48 is PRG 1
    assert rc(nw=15) == _lib.EINVAL                                           # the weight block ends past the array
    assert rc(rows(weight_offset=1)) == _lib.EINVAL
    assert rc(rows(port_stride=nsubc - 1)) == _lib.EINVAL                     # a row wider than its port stride
    assert rc(rows(width=50)) == _lib.EINVAL                                  # mask bits at and past the width
    assert rc(rows(mask_offset=1)) == _lib.EINVAL and rc(nm=2) == _lib.EINVAL  # the mask outside the array
    assert rc(rows(prg_size=0)) == _lib.EINVAL
    for missing in (0, 1):
        assert rc(ptrs=(1 - missing,)) == _lib.EINVAL
    assert rc(descs=False) == _lib.EINVAL and rc(weights=False) == _lib.EINVAL and rc(mask=False) == _lib.EINVAL
    arr, w, m = rows().descriptors()
    assert L.ldpc_hip_precode_map_launch(None, 1, arr, w.ctypes.data, w.size // 2, m.ctypes.data, m.size, None, None,
                                         None) == _lib.EINVAL
    # the sync form: topology, format, weight, nof_re * nof_layers >= 2^31, null
    x, out, w1 = np.zeros((8, 2), np.int8), np.zeros(16, np.complex64), np.ones(2, np.complex64)

    def sync(n=4, ly=2, po=1, inp=x, fmt=_lib.SYM_CI8, w=w1, o=out):
        return L.ldpc_hip_precode_sync(hip_ctx.handle, n, ly, po, inp.ctypes.data if inp is not None else None, fmt,
                                       w.ctypes.data if w is not None else None,
                                       o.ctypes.data if o is not None else None)
    w2 = np.ones(4, np.complex64)
    assert sync() == _lib.EINVAL and sync(po=2, fmt=2, w=w2) == _lib.EINVAL
    assert sync(n=1 << 30, po=2, w=w2) == _lib.EINVAL
    assert sync(po=2, w=np.array([1, 1, 1, np.inf], np.complex64)) == _lib.EINVAL
    assert sync(po=2, w=None) == _lib.EINVAL and sync(po=2, w=w2, inp=None) == _lib.EINVAL
    assert sync(po=2, w=w2, o=None) == _lib.EINVAL
    assert L.ldpc_hip_precode_sync(None, 4, 2, 2, x.ctypes.data, 1, w2.ctypes.data, out.ctypes.data) == _lib.EINVAL
    with pytest.raises(_lib.LdpcHipError):
        pc.channel_precoder_hip(hip_ctx).apply_precoding(np.zeros((1, 4), np.complex64), np.zeros((2, 4), np.complex64),
                                                         np.ones((1, 2), np.complex64))
    torch.cuda.synchronize()
    assert np.all(d_grid.cpu().numpy().view(np.uint32) == R.GUARD)
    # a row with no masked RE is skipped (whatever its weights' reach), and the same buffers then take a good launch
    empty = pc.precode_rows()
    empty.add((4, 1, nsubc), masks, 4, np.ones((2, 4, 2), np.complex64))
    empty.masks[:] = 0
    assert rc(empty) == _lib.OK
    torch.cuda.synchronize()
    assert np.all(d_grid.cpu().numpy().view(np.uint32) == R.GUARD)
    assert rc() == _lib.OK and sync(po=2, w=w2) == _lib.OK and sync(n=0, po=2, w=w2) == _lib.OK
    torch.cuda.synchronize()
    grid = d_grid.cpu().numpy().view(np.uint32).reshape(4, nsubc)
    assert np.all(grid[:, ~masks[0]] == R.GUARD) and np.all(grid[:, masks[0]] == 0x40004000)  # two layers of (1 + j) 1 = 2 + 2j


def test_capture_and_replay_with_new_symbols(hip_ctx):
    """Launch, capture, then replay with other symbols at the same addresses: equal to an eager launch of them."""
    import torch
    from srsran_projectvtlmo_amd import precoding as pc
    cases, _, inputs = _fixture()
    i = next(i for i, c in enumerate(cases) if c["form"] == "grid" and (c["layers"], c["ports"]) == (2, 2))
    c, (sym, w) = cases[i], inputs[i]
    masks, shape = R.case_masks(c), (c["ports"], R.NSYMB, c["nrb"] * R.NRE)
    rows = pc.precode_rows()
    rows.add(shape, masks, c["prg_size"], w)
    other = np.ascontiguousarray(sym[::-1])
    d_sym = _cuda(sym)
    d_grid = _cuda(np.full(shape, R.GUARD, np.uint32))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def launch():
        pc.precode_map_launch(hip_ctx, rows, d_sym.data_ptr(), d_grid.data_ptr(), st.cuda_stream)
    launch()
    st.synchronize()
    L, graph = hip_ctx.lib, ctypes.c_void_p()
    assert L.ldpc_hip_capture_begin(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream)) == 0
    launch()
    assert L.ldpc_hip_capture_end(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream), ctypes.byref(graph)) == 0
    d_sym.copy_(_cuda(other))
    d_grid.fill_(0)
    torch.cuda.synchronize()
    assert L.ldpc_hip_graph_launch(graph, ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    replay = d_grid.cpu().numpy().view(np.uint32).copy()
    L.ldpc_hip_graph_destroy(graph)
    d_grid.fill_(0)
    torch.cuda.synchronize()
    launch()
    st.synchronize()
    eager = d_grid.cpu().numpy().view(np.uint32)
    want = np.zeros(shape, np.uint32)
    R.map_grid(want, masks, c["prg_size"], w, other)
    assert np.array_equal(eager.reshape(shape), want)
    assert np.array_equal(replay, eager)


def test_rate_match_modulate_feeds_the_precoder(hip_ctx):
    """One chain on one stream: rate_match_modulate_launch (ci8) then precode_map_launch, for one BG2 Z = 36 QPSK
    codeblock and one BG1 Z = 36 256-QAM codeblock, each at 2 layers on 4 ports of a 25-RB grid, against the
    restatement applied to the levels tests/modulation_ref.py expects of the scrambled rate-matched bits."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import precoding as pc
    rng = np.random.default_rng(77)
    c_init, nrb, Ly, P = 0x091A0155, 25, 2, 4
    shape = (P, R.NSYMB, nrb * R.NRE)
    # (bg, Z, Qm, E, PRBs, symbols, prg_size): E / Qm / 2 REs = PRBs x 12 x symbols
    tbs = [(2, 36, 2, 1152, (3, 15), (2, 3), 4), (1, 36, 8, 2304, (15, 21), (5, 6), R.WIDEBAND)]
    cws, rm, mods, levels, rows, want = [], [], [], [], pc.precode_rows(), np.full(shape, R.GUARD, np.uint32)
    co = so = 0
    for t, (bg, Z, Qm, E, (b, e), symbols, prg_size) in enumerate(tbs):
        K, N = O.BG_K[bg], O.BG_N_SHORT[bg] * Z
        cw = O.ldpc_encode(bg, Z, rng.integers(0, 2, K * Z).astype(np.uint8))
        bits = O.rate_match(cw, E, 0, Qm, 0, bg, Z)
        bits = bits ^ S.sequence(c_init + t, 0, bits.size)
        cws.append((co, np.packbits(cw.astype(np.uint8))))
        rm.append(cc.cb_rate_match_spec(N, E, Qm, 0, 0, 0, co, 0))
        mods.append(cm.mod_segment(E // Qm, Qm, 0, so, True, c_init + t, 0))
        lv = M.levels(bits, Qm)
        masks = np.zeros(shape[1:], bool)
        masks[list(symbols), b * R.NRE:e * R.NRE] = True
        assert int(masks.sum()) * Ly == E // Qm
        nprg = 1 if prg_size == R.WIDEBAND else -(-nrb // prg_size)
        w = R._weights(5000 + t, (nprg, P, Ly), 2)
        sc = float(R.modulation_scaling(Qm))
        assert np.float32(sc).view(np.uint32) == np.float32(_lib.load().ldpc_hip_modulation_scaling(Qm)).view(np.uint32)
        rows.add(shape, masks, prg_size, w, sc, sym_offset=so)
        R.map_grid(want, masks, prg_size, R.scaled(w, sc), lv)
        co += ((N + 7) // 8 + 15) // 16 * 16
        so += E // Qm + 3                                                     # the second TB's symbols off the 4-byte grid
    h = np.zeros(co, np.uint8)
    for off, p in cws:
        h[off:off + p.size] = p
    d_cw = torch.from_numpy(h).cuda()
    d_sym = torch.full((so, 2), 85, dtype=torch.int8, device="cuda")
    d_grid = _cuda(np.full(shape, R.GUARD, np.uint32))
    s = torch.cuda.current_stream().cuda_stream
    cm.rate_match_modulate_launch(hip_ctx, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), _lib.SYM_CI8, s)
    pc.precode_map_launch(hip_ctx, rows, d_sym.data_ptr(), d_grid.data_ptr(), s)
    torch.cuda.synchronize()
    assert np.array_equal(d_grid.cpu().numpy().view(np.uint32).reshape(shape), want)
