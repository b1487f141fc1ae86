"""GPU tests of PUSCH descrambling (pusch_demodulator_impl.cpp:289-293 on the device): the stand-alone descrambler and
packed-bit scrambler (ldpc_hip_descramble_launch / _sync, ldpc_hip_scramble_bits_launch), descrambling fused into the
rate dematcher (ldpc_hip_rate_dematch_scr_launch, from LLRs and from symbols) and the device-resident slot with a
scrambled codeword per UE. The reference is the brute-force walk of the TS 38.211 5.2.1 recurrences
(tests/scrambling_ref.py); every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
from tests import scrambling_ref as R
from tests.tb_chain import SwFlow, TransportBlock
from tests.vectors import modulate

pytestmark = pytest.mark.gpu
C_INIT = 0x091A0155  # rnti 0x1234, n_id 0x155
# (sequence offset, size): the reference test's grid (pseudo_random_generator_test.cpp), the word-boundary sizes, a far
# offset and a full-size codeblock's worth (4 x 25344)
GRID = [(o, n) for o in (0, 2, 3, 5, 7) for n in (255, 512, 768)] + [(0, n) for n in (1, 31, 32, 33)] + \
    [(100000, 1000), (0, 4 * 25344)]


def _llrs(rng, n):
    return rng.integers(-127, 128, n).astype(np.int8)


def test_descramble_grid(hip_ctx):
    """out = c ? -in : in through ldpc_hip_descramble_sync (the generator object) and ldpc_hip_descramble_launch."""
    import torch
    from srsran_projectvtlmo_amd import sequence_generators as sg
    rng = np.random.default_rng(5)
    gen = sg.create_pseudo_random_generator_hip_factory(hip_ctx).create()
    for off, n in GRID:
        llr = _llrs(rng, n)
        exp = R.descramble(llr, C_INIT, off)
        gen.init(C_INIT)
        gen.advance(off)
        assert np.array_equal(gen.apply_xor(llr), exp), f"sync offset {off} size {n}"
        assert gen.offset == off + n
        d_in = torch.from_numpy(llr).cuda()
        d_out = torch.full((n + 32,), 99, dtype=torch.int8, device="cuda")
        sg.descramble_launch(hip_ctx, [sg.prs_segment(n, C_INIT, off)], d_in.data_ptr(), d_out.data_ptr())
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:n], exp), f"launch offset {off} size {n}"
        assert np.all(got[n:] == 99)


def test_descramble_multi_segment_launch(hip_ctx):
    """One launch: mixed lengths, unaligned input / output byte offsets (byte path), aligned ones (vector path), more
    than one workgroup, and one segment in place. Bytes outside the segments' outputs keep their values."""
    import torch
    from srsran_projectvtlmo_amd import sequence_generators as sg
    rng = np.random.default_rng(6)
    # (length, c_init, sequence offset, in place)
    shapes = [(40000, C_INIT, 17, False), (5, 1, 0, False), (777, 0x7FFFFFFF, 33, True), (1001, 0, 100000, False),
              (32, C_INIT, 31, False), (4096, 3, 5, True), (33, 2, 1, False)]
    pos, segs, parts = 16, [], []
    for k, (n, c, so, inplace) in enumerate(shapes):
        a = pos + (0 if k in (0, 5) else k % 3)      # segments 0 and 5 start 16-byte aligned
        pos = (a + n + 15) // 16 * 16 + 16
        b = a
        if not inplace:
            b = pos + (0 if k == 0 else (k + 1) % 3)
            pos = (b + n + 15) // 16 * 16 + 16
        segs.append(sg.prs_segment(n, c, so, a, b))
        parts.append((a, b, _llrs(rng, n)))
    buf = np.full(pos + 64, 99, np.int8)
    for a, _, llr in parts:
        buf[a:a + llr.size] = llr
    exp = buf.copy()
    for (a, b, llr), s in zip(parts, segs):
        exp[b:b + llr.size] = R.descramble(llr, s.c_init, s.seq_offset)
    d = torch.from_numpy(buf).cuda()
    sg.descramble_launch(hip_ctx, segs, d.data_ptr(), d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"first difference at byte {bad[:1]}"


def test_minus_128_is_kept(hip_ctx):
    """-128 is outside the LLR range; the documented behaviour is that it comes out as -128 on both code paths."""
    import torch
    from srsran_projectvtlmo_amd import sequence_generators as sg
    llr = np.full(100, -128, np.int8)
    d_in = torch.from_numpy(llr).cuda()
    d_out = torch.zeros(116, dtype=torch.int8, device="cuda")
    sg.descramble_launch(hip_ctx, [sg.prs_segment(100, C_INIT, 0, 0, 0), sg.prs_segment(13, C_INIT, 0, 0, 101)],
                         d_in.data_ptr(), d_out.data_ptr())
    got = d_out.cpu().numpy()
    assert np.all(got[:100] == -128) and np.all(got[101:114] == -128)


def test_packed_bits_grid(hip_ctx):
    """generate (NULL input) and apply_xor on packed bits, MSB first; bits of the last byte beyond the length keep the
    input's value (generate: zero), bytes beyond it are untouched."""
    import torch
    from srsran_projectvtlmo_amd import sequence_generators as sg
    rng = np.random.default_rng(7)
    for off, n in GRID:
        nb = (n + 7) // 8
        seq = R.packed(C_INIT, off, n)
        d_out = torch.full((nb + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        sg.scramble_bits_launch(hip_ctx, [sg.prs_segment(n, C_INIT, off)], 0, d_out.data_ptr())
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:nb], seq), f"generate offset {off} size {n}"
        assert np.all(got[nb:] == 0xA5)
        data = rng.integers(0, 256, nb).astype(np.uint8)
        d_in = torch.from_numpy(data).cuda()
        d_out.fill_(0xA5)
        sg.scramble_bits_launch(hip_ctx, [sg.prs_segment(n, C_INIT, off, 0, 1)], d_in.data_ptr(), d_out.data_ptr())
        got = d_out.cpu().numpy()
        exp = R.xor_packed(data, C_INIT, off, n)
        assert np.array_equal(got[1:1 + nb], exp), f"xor offset {off} size {n}"
        if n % 8:
            keep = 0xFF >> (n % 8)
            assert (got[nb] & keep) == (data[-1] & keep), "trailing bits of the last byte changed"
        assert got[0] == 0xA5 and np.all(got[1 + nb:] == 0xA5)


def test_generator_object_packed(hip_ctx):
    """pseudo_random_generator mirror: generate / apply_xor consume the sequence as the reference's do."""
    from srsran_projectvtlmo_amd import sequence_generators as sg
    gen = sg.pseudo_random_generator_hip(hip_ctx)
    gen.init(C_INIT)
    a = gen.generate(255)
    st = gen.get_state()
    assert (st.x1, st.x2) == R.state(C_INIT, 255)
    b = gen.generate(64)
    assert np.array_equal(a, R.packed(C_INIT, 0, 255)) and np.array_equal(b, R.packed(C_INIT, 255, 64))
    data = np.arange(10, dtype=np.uint8)
    gen.init(st)
    assert np.array_equal(gen.apply_xor(data, 77), R.xor_packed(data, C_INIT, 255, 77))
    assert gen.offset == 255 + 77


# ---- fused into the dematcher --------------------------------------------------------------------------------------
# (bg, Z, Qm, E): the staging limit; a small BG2 codeblock; a 64-QAM one whose E is no multiple of 32 or 16
FUSED_SHAPES = [(1, 384, 8, 32768), (2, 36, 2, 156 * 4), (2, 36, 6, 1002)]


def _dematch_scr(hip_ctx, dm, scr, d_soft, soft_off, d_llr=None, llr_off=None, demod=None, d_sym=None, d_nv=None):
    from srsran_projectvtlmo_amd import _lib
    n = len(soft_off)
    u64 = ctypes.c_uint64 * n
    return hip_ctx.lib.ldpc_hip_rate_dematch_scr_launch(
        hip_ctx.handle, n, dm, d_llr.data_ptr() if d_llr is not None else None,
        u64(*llr_off) if llr_off is not None else None, demod, d_sym.data_ptr() if d_sym is not None else None,
        d_nv.data_ptr() if d_nv is not None else None, scr, d_soft.data_ptr(), u64(*soft_off), _lib.stream_arg(0))


def _dematch_descs(bg, Z, Qm, E, rv, new_data, n=2):
    from srsran_projectvtlmo_amd import _lib
    dm = (_lib.DematchDesc * n)()
    for d in dm:
        d.modulation_order, d.rv, d.new_data = Qm, rv, int(new_data)
        d.cb_length, d.rm_length, d.Nref, d.nof_filler_bits = O.BG_N_SHORT[bg] * Z, E, 0, 0
    return dm


@pytest.mark.parametrize("bg,Z,Qm,E", FUSED_SHAPES)
@pytest.mark.parametrize("from_symbols", [False, True])
def test_fused_dematch_descrambles(hip_ctx, bg, Z, Qm, E, from_symbols):
    """Descrambling fused into the stand-alone dematch kernel (ldpc_hip_rate_dematch_scr_launch, 512 threads): not the
    dematcher fused into the decode kernels, whose soft buffers tests/test_gpu_dematch_grid.py compares.
    Two CBs of one codeword (the second one's sequence offset is the first one's E), rv 0 with new data and then rv 2
    combining: the soft buffers equal the oracle dematcher fed the reference-descrambled LLRs; the LLRs come from
    d_llr, or are demodulated from symbols in the dematcher (oracle demodulator)."""
    import torch
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import sequence_generators as sg
    rng = np.random.default_rng(1000 * bg + E + int(from_symbols))
    N = O.BG_N_SHORT[bg] * Z
    Ea = (E + 15) // 16 * 16 + 16
    Na = (N + 15) // 16 * 16
    scr = sg.scramble_descriptors([(C_INIT, 0), (C_INIT, E)])
    d_soft = torch.zeros(2 * Na, dtype=torch.int8, device="cuda")
    soft = [np.zeros(N, np.int8), np.zeros(N, np.int8)]
    for rv, new_data in ((0, True), (2, False)):
        dm = _dematch_descs(bg, Z, Qm, E, rv, new_data)
        if from_symbols:
            nsym = E // Qm
            bits = rng.integers(0, 2, 2 * E).astype(np.uint8)
            z = modulate(bits, Qm)
            w = (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size)) * np.sqrt(0.05)
            sym = (z + w).astype(np.complex64)
            nv = (0.1 * rng.uniform(0.5, 2.0, z.size)).astype(np.float32)
            llr = [O.demodulate_soft(Qm, sym[k * nsym:(k + 1) * nsym], nv[k * nsym:(k + 1) * nsym]) for k in (0, 1)]
            demod = cm.demod_descriptors([cm.demod_segment(nsym, Qm, k * nsym, k * nsym, 0) for k in (0, 1)])
            d_sym = torch.from_numpy(sym.view(np.float32)).cuda()
            d_nv = torch.from_numpy(nv).cuda()
            rc = _dematch_scr(hip_ctx, dm, scr, d_soft, [0, Na], demod=demod, d_sym=d_sym, d_nv=d_nv)
        else:
            llr = [_llrs(rng, E), _llrs(rng, E)]
            buf = np.zeros(2 * Ea, np.int8)
            buf[3:3 + E] = llr[0]           # unaligned: the byte staging path
            buf[Ea:Ea + E] = llr[1]         # aligned: 16-byte loads
            d_llr = torch.from_numpy(buf).cuda()
            rc = _dematch_scr(hip_ctx, dm, scr, d_soft, [0, Na], d_llr=d_llr, llr_off=[3, Ea])
        assert rc == 0
        torch.cuda.synchronize()
        got = d_soft.cpu().numpy()
        for k in (0, 1):
            O.rate_dematch(soft[k], R.descramble(llr[k], C_INIT, k * E), new_data, rv, Qm, 0, 0)
            assert np.array_equal(got[k * Na:k * Na + N], soft[k]), f"rv {rv} cb {k}"


def test_fused_dematch_limits_and_null(hip_ctx):
    """A scrambled CB longer than the LDS staging is refused (and the message names the stand-alone call); scr == NULL
    and a disabled descriptor give exactly what ldpc_hip_rate_dematch_launch gives."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import sequence_generators as sg
    rng = np.random.default_rng(9)
    bg, Z, Qm, E = 1, 384, 4, 32772
    N = O.BG_N_SHORT[bg] * Z
    llr = _llrs(rng, E)
    d_llr = torch.from_numpy(llr).cuda()
    dm = _dematch_descs(bg, Z, Qm, E, 0, True, n=1)
    d_soft = torch.full((N,), 5, dtype=torch.int8, device="cuda")
    rc = _dematch_scr(hip_ctx, dm, sg.scramble_descriptors([(C_INIT, 0)]), d_soft, [0], d_llr=d_llr, llr_off=[0])
    assert rc == _lib.EINVAL
    assert b"ldpc_hip_descramble_launch" in hip_ctx.lib.ldpc_hip_last_error(hip_ctx.handle)
    torch.cuda.synchronize()
    assert np.all(d_soft.cpu().numpy() == 5), "a refused launch wrote the soft buffer"
    outs = []
    for scr in (None, sg.scramble_descriptors([None]), "plain"):
        d_soft.fill_(5)
        if scr == "plain":
            rc = hip_ctx.lib.ldpc_hip_rate_dematch_launch(hip_ctx.handle, 1, dm, d_llr.data_ptr(),
                                                          (ctypes.c_uint64 * 1)(0), d_soft.data_ptr(),
                                                          (ctypes.c_uint64 * 1)(0), _lib.stream_arg(0))
        else:
            rc = _dematch_scr(hip_ctx, dm, scr, d_soft, [0], d_llr=d_llr, llr_off=[0])
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(d_soft.cpu().numpy())
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[2])
    assert np.array_equal(outs[2], O.rate_dematch(np.zeros(N, np.int8), llr, True, 0, Qm, 0, 0))


# ---- the slot ------------------------------------------------------------------------------------------------------
SLOT_SEED = 41
SLOT_UES = [(40000, 1, 14000, "QAM256", 4), (256, 2, 156 * 4, "QPSK", 4), (3000, 2, 1500, "QAM16", 2),
            (9000, 1, 3000, "QAM64", 2)]
SLOT_IDS = [(0x1234, 0x155), (1, 0), (65535, 1023), (0x4601, 7)]  # (rnti, n_id) per TB
MODS = {"QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}


@functools.lru_cache(maxsize=1)
def _slot():
    """The four-UE slot of test_gpu_demod.py::test_slot_from_symbols with a scrambled codeword per UE: the transmit
    side XORs the rate-matched bits with the reference sequence before modulation. Returns the TBs, their symbols and
    noise variances, and the oracle flow's results on the reference-descrambled oracle LLRs (computed once)."""
    from srsran_projectvtlmo_amd.sequence_generators import pusch_c_init
    rng = np.random.default_rng(SLOT_SEED)
    tbs = [TransportBlock(rng, tbs_, bg, syms, mod, layers) for (tbs_, bg, syms, mod, layers) in SLOT_UES]
    sym_tb, nv_tb, flows = [], [], []
    for tb, (_, _, _, mod, _), (rnti, n_id) in zip(tbs, SLOT_UES, SLOT_IDS):
        c_init = pusch_c_init(rnti, n_id)
        bits = np.concatenate([O.rate_match(tb.cws[r], m["rm_length"], 0, tb.Qm, 0, tb.bg, tb.Z)
                               for r, m in enumerate(tb.metas)])
        z = modulate(bits ^ R.sequence(c_init, 0, bits.size), MODS[mod])
        nvar = {2: 0.5, 4: 0.1, 6: 0.03, 8: 0.008}[tb.Qm]
        w = (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size)) * np.sqrt(nvar / 2)
        sym = (z + w).astype(np.complex64)
        nv = np.full(z.size, nvar, np.float32)
        llr = R.descramble(O.demodulate_soft(MODS[mod], sym, nv), c_init, 0)
        f = SwFlow(tb, nof_iters=6, early_stop=True)
        ok, _ = f.transmission(np.split(llr, np.cumsum([m["rm_length"] for m in tb.metas])[:-1]), 0, True)
        sym_tb.append(sym)
        nv_tb.append(nv)
        flows.append((f, ok))
    return tbs, sym_tb, nv_tb, flows


def _specs(tbs, ids):
    from srsran_projectvtlmo_amd import pusch
    return [pusch.tb_slot_spec(tb.tbs, tb.bg, tb.Z, tb.F, [m["rm_length"] for m in tb.metas], tb.Qm, 0, True, 0, 6,
                               True, rnti=rnti, n_id=n_id) for tb, (rnti, n_id) in zip(tbs, ids)]


def _check_slot(pipe, tbs, flows, what):
    got, cbres = pipe.results()
    i = 0
    for t, (tb, (f, ok), (tb_bytes, g_ok, _)) in enumerate(zip(tbs, flows, got)):
        for r in range(tb.C):
            assert bool(cbres[i + r, 0]) == f.crc_ok[r], f"{what}: tb {t} cb {r} crc"
            if f.crc_ok[r]:
                assert cbres[i + r, 1] == f.iters_used[r], f"{what}: tb {t} cb {r} iterations"
        i += tb.C
        assert g_ok == ok, f"{what}: tb {t} crc"
        assert np.array_equal(np.unpackbits(tb_bytes)[: tb.tbs], tb.data), f"{what}: tb {t} bytes"


def _clear(pipe):
    pipe.d_res.zero_()
    pipe.d_tbres.zero_()
    pipe.d_tb.zero_()
    pipe.d_out.zero_()


def test_slot_scrambled(hip_ctx):
    """The device slot from scrambled symbols, descrambling inside the fused dematcher, then with demodulation and
    descrambling as their own kernels (fuse_demod = False), then as one captured graph replayed: every CB flag,
    iteration count, TB CRC and TB byte equals the oracle flow on the reference-descrambled oracle LLRs."""
    import torch
    from srsran_projectvtlmo_amd import pusch
    tbs, sym_tb, nv_tb, flows = _slot()
    assert all(ok for _, ok in flows), "the oracle flow must decode all four TBs at this seed"
    pipe = pusch.SlotPipeline(hip_ctx, _specs(tbs, SLOT_IDS))
    assert pipe.scrambled and pipe.fuse_demod
    pipe.upload_symbols(sym_tb, nv_tb)
    s = torch.cuda.Stream()
    pipe.launch(s.cuda_stream)
    s.synchronize()
    _check_slot(pipe, tbs, flows, "fused")
    _clear(pipe)
    pipe.fuse_demod = False
    pipe.launch(s.cuda_stream)
    s.synchronize()
    _check_slot(pipe, tbs, flows, "separate kernels")
    for fuse in (True, False):
        pipe.fuse_demod = fuse
        pipe.capture(s.cuda_stream)
        s.synchronize()
        _clear(pipe)
        pipe.launch_graph(s.cuda_stream)
        s.synchronize()
        _check_slot(pipe, tbs, flows, f"graph replay (fuse_demod={fuse})")
    pipe.release_graph()


def test_slot_scrambled_from_llrs(hip_ctx):
    """upload() of LLRs with rnti >= 0: the LLRs are still scrambled; the fused dematcher descrambles them."""
    import torch
    from srsran_projectvtlmo_amd import pusch
    tbs, sym_tb, nv_tb, flows = _slot()
    llr_tb = [np.split(O.demodulate_soft(MODS[u[3]], sym, nv), np.cumsum([m["rm_length"] for m in tb.metas])[:-1])
              for tb, u, sym, nv in zip(tbs, SLOT_UES, sym_tb, nv_tb)]
    for fuse_dematch in (True, False):
        pipe = pusch.SlotPipeline(hip_ctx, _specs(tbs, SLOT_IDS), fuse_dematch=fuse_dematch)
        pipe.upload(llr_tb)
        pipe.launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _check_slot(pipe, tbs, flows, f"from LLRs (fuse_dematch={fuse_dematch})")


def test_slot_descrambling_off_fails(hip_ctx):
    """The same symbols with rnti = -1 (no descrambling) fail every TB CRC: the slot test can fail."""
    import torch
    from srsran_projectvtlmo_amd import pusch
    tbs, sym_tb, nv_tb, _ = _slot()
    pipe = pusch.SlotPipeline(hip_ctx, _specs(tbs, [(-1, 0)] * len(tbs)))
    assert not pipe.scrambled
    pipe.upload_symbols(sym_tb, nv_tb)
    pipe.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, _ = pipe.results()
    assert not any(ok for _, ok, _ in got)
