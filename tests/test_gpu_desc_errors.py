"""Rejected descriptors through every public entry point that shares a descriptor translation
(csrc/ldpc_hip_descs.cpp): the call returns EINVAL with the entry point's error text and launches nothing, and the
same entry point then serves one valid BG2 Z=36 codeblock bit-exactly against the oracle (a rejection leaves the
context usable). The texts are those of the entry points before the translations were gathered in one unit; the
demodulator mismatch has one wording now, prefixed with the entry point's name."""
import ctypes

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

BG, Z, QM, E, ITERS = 2, 36, 2, 1248, 6
N = O.BG_N_SHORT[BG] * Z
MB = (O.BG_K[BG] * Z + 7) // 8
NA = (N + 15) // 16 * 16


def _err(ctx):
    return ctx.lib.ldpc_hip_last_error(ctx.handle).decode()


def _rejected(ctx, rc, text):
    from srsran_projectvtlmo_amd import _lib
    assert rc == _lib.EINVAL
    assert _err(ctx) == text


@pytest.fixture(scope="module")
def cb():
    """One codeblock: rate-matched LLRs of a random codeword (rv 0), the oracle's soft buffer and decoded message."""
    rng = np.random.default_rng(77)
    msg = rng.integers(0, 2, O.BG_K[BG] * Z).astype(np.uint8)
    tx = O.rate_match(O.ldpc_encode(BG, Z, msg), E, 0, QM, 0, BG, Z)
    llr = O.quantize_array(2.0 * (1.0 - 2.0 * tx) + rng.standard_normal(E), 8.0)
    soft = O.rate_dematch(np.zeros(N, np.int8), llr, True, 0, QM, 0, 0)
    out, _ = O.ldpc_decode(BG, Z, soft, ITERS)
    soft.setflags(write=False), llr.setflags(write=False), out.setflags(write=False)
    return {"llr": llr, "soft": soft, "msg": out}


def _dec_desc(**kw):
    from srsran_projectvtlmo_amd import _lib
    d = _lib.DecDesc(base_graph=BG, max_iterations=ITERS, crc_mode=_lib.CRC_MODE_NONE, crc_poly=0, lifting_size=Z,
                     nof_filler_bits=0, llr_length=N, scaling_factor=0.0, llr_offset=0, out_offset=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _dm_desc(**kw):
    from srsran_projectvtlmo_amd import _lib
    d = _lib.DematchDesc(modulation_order=QM, rv=0, new_data=1, reserved=0, cb_length=N, rm_length=E, Nref=0,
                         nof_filler_bits=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _arr(ctype, items):
    return (ctype * len(items))(*items)


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def test_decode_plan_create(hip_ctx, cb):
    import torch
    from srsran_projectvtlmo_amd import _lib
    plan = ctypes.c_void_p()
    rc = hip_ctx.lib.ldpc_hip_decode_plan_create(hip_ctx.handle, 1, _arr(_lib.DecDesc, [_dec_desc(max_iterations=0)]),
                                                 ctypes.byref(plan))
    _rejected(hip_ctx, rc, "Max iterations must be different to 0")
    assert not plan.value
    assert hip_ctx.lib.ldpc_hip_decode_plan_create(hip_ctx.handle, 1, _arr(_lib.DecDesc, [_dec_desc()]),
                                                   ctypes.byref(plan)) == 0
    d_llr = torch.from_numpy(np.array(cb["soft"])).cuda()
    d_out = torch.zeros(MB, dtype=torch.uint8, device="cuda")
    assert hip_ctx.lib.ldpc_hip_decode_launch(plan, d_llr.data_ptr(), d_out.data_ptr(), None, _lib.stream_arg(0)) == 0
    torch.cuda.synchronize()
    hip_ctx.lib.ldpc_hip_decode_plan_destroy(plan)
    assert np.array_equal(d_out.cpu().numpy(), cb["msg"])


@pytest.mark.parametrize("n", [1, 2])
def test_decode_sync(hip_ctx, cb, n):
    from srsran_projectvtlmo_amd import _lib
    soft = [np.array(cb["soft"]) for _ in range(n)]
    outs = [np.zeros(MB, np.uint8) for _ in range(n)]
    bad = [_dec_desc() for _ in range(n)]
    if n == 1:
        bad[0].llr_length, text = 12 * Z - 1, "input length out of range [(K+2)Z, N_short Z]"
    else:
        bad[1].scaling_factor, text = 1.0, "Scaling factor must be between 0 and 1 exclusively"
    rc = hip_ctx.lib.ldpc_hip_decode_sync(hip_ctx.handle, n, _arr(_lib.DecDesc, bad), _ptrs(soft), _ptrs(outs), None)
    _rejected(hip_ctx, rc, text)
    assert not any(o.any() for o in outs)
    res = (_lib.CbResult * n)()
    assert hip_ctx.lib.ldpc_hip_decode_sync(hip_ctx.handle, n, _arr(_lib.DecDesc, [_dec_desc() for _ in range(n)]),
                                            _ptrs(soft), _ptrs(outs), res) == 0
    for o in outs:
        assert np.array_equal(o, cb["msg"])


@pytest.mark.parametrize("n", [1, 2])
def test_rate_dematch_sync(hip_ctx, cb, n):
    from srsran_projectvtlmo_amd import _lib
    llrs = [np.array(cb["llr"]) for _ in range(n)]
    softs = [np.zeros(N, np.int8) for _ in range(n)]
    bad = [_dm_desc() for _ in range(n)]
    if n == 1:
        bad[0].nof_filler_bits, text = 8 * Z, "LDPC rate dematching: invalid number of filler bits."
    else:
        bad[1].cb_length, text = N + 1, "LDPC rate dematching: invalid input length."
    rc = hip_ctx.lib.ldpc_hip_rate_dematch_sync(hip_ctx.handle, n, _arr(_lib.DematchDesc, bad), _ptrs(softs),
                                                _ptrs(llrs))
    _rejected(hip_ctx, rc, text)
    assert not any(s.any() for s in softs)
    assert hip_ctx.lib.ldpc_hip_rate_dematch_sync(hip_ctx.handle, n, _arr(_lib.DematchDesc, [_dm_desc()] * n),
                                                  _ptrs(softs), _ptrs(llrs)) == 0
    for s in softs:
        assert np.array_equal(s, cb["soft"])


def test_rate_dematch_launch(hip_ctx, cb):
    import torch
    from srsran_projectvtlmo_amd import _lib
    d_llr = torch.from_numpy(np.array(cb["llr"])).cuda()
    d_soft = torch.zeros(N, dtype=torch.int8, device="cuda")
    zero = (ctypes.c_uint64 * 1)(0)

    def launch(desc):
        return hip_ctx.lib.ldpc_hip_rate_dematch_launch(hip_ctx.handle, 1, _arr(_lib.DematchDesc, [desc]),
                                                        d_llr.data_ptr(), zero, d_soft.data_ptr(), zero,
                                                        _lib.stream_arg(0))
    _rejected(hip_ctx, launch(_dm_desc(rv=4)), "invalid rv / modulation / rm_length")
    assert launch(_dm_desc()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_soft.cpu().numpy(), cb["soft"])


def test_demod_dematch_launch(hip_ctx):
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_modulation as cm
    rng = np.random.default_rng(5)
    nsym = E // QM
    sym = ((rng.standard_normal(nsym) + 1j * rng.standard_normal(nsym)) * 0.8).astype(np.complex64)
    nv = (0.1 * rng.uniform(0.5, 2.0, nsym)).astype(np.float32)
    d_sym, d_nv = torch.from_numpy(sym.view(np.float32)).cuda(), torch.from_numpy(nv).cuda()
    d_soft = torch.zeros(N, dtype=torch.int8, device="cuda")
    zero = (ctypes.c_uint64 * 1)(0)

    def launch(symbols):
        demod = cm.demod_descriptors([cm.demod_segment(symbols, QM, 0, 0, 0)])
        return hip_ctx.lib.ldpc_hip_demod_dematch_launch(hip_ctx.handle, 1, _arr(_lib.DematchDesc, [_dm_desc()]),
                                                         demod, d_sym.data_ptr(), d_nv.data_ptr(), d_soft.data_ptr(),
                                                         zero, _lib.stream_arg(0))
    # was "demod_dematch_launch: symbols x bits per symbol must equal rm_length"
    _rejected(hip_ctx, launch(nsym - 1),
              "demod_dematch_launch: symbols x bits per symbol must equal rm_length <= 32768")
    assert launch(nsym) == 0
    torch.cuda.synchronize()
    want = O.rate_dematch(np.zeros(N, np.int8), O.demodulate_soft(QM, sym, nv), True, 0, QM, 0, 0)
    assert np.array_equal(d_soft.cpu().numpy(), want)


def test_dematch_decode_scr_launch(hip_ctx, cb):
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import sequence_generators as sg
    from tests import scrambling_ref as R
    c_init = 0x2468ace
    # the sign flips are their own inverse
    scrambled = np.ascontiguousarray(R.descramble(np.array(cb["llr"]), c_init, 0), dtype=np.int8)
    d_llr = torch.from_numpy(scrambled).cuda()
    d_soft = torch.zeros(NA, dtype=torch.int8, device="cuda")
    d_out = torch.zeros(MB, dtype=torch.uint8, device="cuda")
    plan = ctypes.c_void_p()
    assert hip_ctx.lib.ldpc_hip_decode_plan_create(hip_ctx.handle, 1, _arr(_lib.DecDesc, [_dec_desc()]),
                                                   ctypes.byref(plan)) == 0
    zero = (ctypes.c_uint64 * 1)(0)
    scr = sg.scramble_descriptors([(c_init, 0)])

    def launch(desc):
        return hip_ctx.lib.ldpc_hip_dematch_decode_scr_launch(plan, _arr(_lib.DematchDesc, [desc]), d_llr.data_ptr(),
                                                              zero, None, None, None, scr, d_soft.data_ptr(),
                                                              d_out.data_ptr(), None, _lib.stream_arg(0))
    _rejected(hip_ctx, launch(_dm_desc(nof_filler_bits=1)),
              "dematch_decode_launch: dematch descriptor does not match its codeblock (cb_length != llr_length or "
              "filler bits differ)")
    assert launch(_dm_desc()) == 0
    torch.cuda.synchronize()
    hip_ctx.lib.ldpc_hip_decode_plan_destroy(plan)
    assert np.array_equal(d_soft.cpu().numpy()[:N], cb["soft"])
    assert np.array_equal(d_out.cpu().numpy(), cb["msg"])


def test_enqueue(hip_ctx, cb):
    from srsran_projectvtlmo_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle

    def cfg(**kw):
        c = _lib.HwConfig(base_graph=BG, modulation_order=QM, rv=0, new_data=1, nof_segments=1, cw_length=E,
                          lifting_size=Z, Ncb=N, Nref=0, nof_segment_bits=O.BG_K[BG] * Z, nof_filler_bits=0,
                          max_nof_ldpc_iterations=ITERS, use_early_stop=0, cb_crc_type=_lib.CRC24B, cb_crc_len=24,
                          absolute_cb_id=0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    llr = np.array(cb["llr"])
    assert lib.ldpc_hip_queue_reserve(h) == 0
    try:
        rc = lib.ldpc_hip_enqueue(h, 0, ctypes.byref(cfg(rv=4)), llr.ctypes.data, llr.size, None, 0)
        _rejected(hip_ctx, rc, "invalid HAL operation configuration")
        assert lib.ldpc_hip_enqueue(h, 0, ctypes.byref(cfg()), llr.ctypes.data, llr.size, None, 0) == 0
        out, soft = np.zeros(MB, np.uint8), np.zeros(N, np.int8)
        while True:
            rc = lib.ldpc_hip_dequeue(h, 0, out.ctypes.data, out.size, soft.ctypes.data, soft.size)
            if rc != _lib.NOT_READY:
                break
        assert rc == 0
    finally:
        lib.ldpc_hip_queue_free(h)
    assert np.array_equal(soft, cb["soft"])
    assert np.array_equal(out, cb["msg"])


NCB_TEXT = "LDPC rate dematching: limited buffer shorter than the systematic bits."
NSYS = (O.BG_K[BG] - 2) * Z


@pytest.mark.parametrize("entry", ["rate_dematch_sync_1", "rate_dematch_sync_2", "rate_dematch_launch",
                                   "rate_dematch_scr_launch", "demod_dematch_launch", "dematch_decode_launch",
                                   "dematch_decode_scr_launch", "enqueue"])
def test_limited_buffer_below_systematic_bits(hip_ctx, cb, entry):
    """Nref = (K - 2) Z - 1 through every entry point that takes dematch descriptors: EINVAL with the reason, nothing
    launched (the sentinel-filled soft buffer and output keep their bytes). With such a buffer the allot loop's parity
    range would wrap and write up to E soft bits past the codeblock; the case is refused, never run."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import sequence_generators as sg
    lib, h = hip_ctx.lib, hip_ctx.handle
    bad = _dm_desc(Nref=NSYS - 1)
    llr = np.array(cb["llr"])
    zero = (ctypes.c_uint64 * 1)(0)
    if entry.startswith("rate_dematch_sync"):
        n = int(entry[-1])
        softs = [np.full(N, 55, np.int8) for _ in range(n)]
        descs = [_dm_desc() for _ in range(n - 1)] + [bad]
        rc = lib.ldpc_hip_rate_dematch_sync(h, n, _arr(_lib.DematchDesc, descs), _ptrs(softs), _ptrs([llr] * n))
        _rejected(hip_ctx, rc, NCB_TEXT)
        assert all(np.all(s == 55) for s in softs)
        return
    if entry == "enqueue":
        cfg = _lib.HwConfig(base_graph=BG, modulation_order=QM, rv=0, new_data=1, nof_segments=1, cw_length=E,
                            lifting_size=Z, Ncb=N, Nref=NSYS - 1, nof_segment_bits=O.BG_K[BG] * Z, nof_filler_bits=0,
                            max_nof_ldpc_iterations=ITERS, use_early_stop=0, cb_crc_type=_lib.CRC24B, cb_crc_len=24,
                            absolute_cb_id=0)
        assert lib.ldpc_hip_queue_reserve(h) == 0
        try:
            rc = lib.ldpc_hip_enqueue(h, 0, ctypes.byref(cfg), llr.ctypes.data, llr.size, None, 0)
            _rejected(hip_ctx, rc, "invalid HAL operation configuration")  # the HAL has one text for its configuration
        finally:
            lib.ldpc_hip_queue_free(h)
        return
    d_llr = torch.from_numpy(llr).cuda()
    d_soft = torch.full((NA + 64,), 55, dtype=torch.int8, device="cuda")
    d_out = torch.full((MB + 16,), 55, dtype=torch.uint8, device="cuda")
    nsym = E // QM
    d_sym = torch.zeros(2 * nsym, dtype=torch.float32, device="cuda")
    d_nv = torch.ones(nsym, dtype=torch.float32, device="cuda")
    demod = cm.demod_descriptors([cm.demod_segment(nsym, QM, 0, 0, 0)])
    scr = sg.scramble_descriptors([(0x2468ace, 0)])
    descs = _arr(_lib.DematchDesc, [bad])
    st = _lib.stream_arg(0)
    plan = ctypes.c_void_p()
    try:
        if entry == "rate_dematch_launch":
            rc = lib.ldpc_hip_rate_dematch_launch(h, 1, descs, d_llr.data_ptr(), zero, d_soft.data_ptr(), zero, st)
        elif entry == "rate_dematch_scr_launch":
            rc = lib.ldpc_hip_rate_dematch_scr_launch(h, 1, descs, d_llr.data_ptr(), zero, None, None, None, scr,
                                                      d_soft.data_ptr(), zero, st)
        elif entry == "demod_dematch_launch":
            rc = lib.ldpc_hip_demod_dematch_launch(h, 1, descs, demod, d_sym.data_ptr(), d_nv.data_ptr(),
                                                   d_soft.data_ptr(), zero, st)
        else:
            assert lib.ldpc_hip_decode_plan_create(h, 1, _arr(_lib.DecDesc, [_dec_desc()]), ctypes.byref(plan)) == 0
            if entry == "dematch_decode_launch":
                rc = lib.ldpc_hip_dematch_decode_launch(plan, descs, d_llr.data_ptr(), zero, None, None, None,
                                                        d_soft.data_ptr(), d_out.data_ptr(), None, st)
            else:
                rc = lib.ldpc_hip_dematch_decode_scr_launch(plan, descs, None, None, demod, d_sym.data_ptr(),
                                                            d_nv.data_ptr(), scr, d_soft.data_ptr(), d_out.data_ptr(),
                                                            None, st)
        _rejected(hip_ctx, rc, NCB_TEXT)
        torch.cuda.synchronize()
        assert bool((d_soft == 55).all()) and bool((d_out == 55).all())
    finally:
        if plan.value:
            lib.ldpc_hip_decode_plan_destroy(plan)
