"""GPU test of the host round trip the five stage *_sync entry points share (ldpc_hip_ctx::sync_round_trip: scratch
reserved, copies in, the stage's segments, copies out, one synchronise): ldpc_hip_modulate_sync, _equalize_sync,
_precode_sync, _demodulate_sync and _descramble_sync in turn on one fresh context, each in the scratch the one before
it sized, then in the reverse order at sizes that make every scratch buffer grow, then small again. Every output bit
for bit against the references the stages' own tests use."""
import functools

import numpy as np
import pytest

import oracle as O
from tests import equalizer_ref as E
from tests import modulation_ref as M
from tests import precoder_ref as R
from tests import scrambling_ref as S
from tests.vectors import noisy_symbols

pytestmark = pytest.mark.gpu
C_INIT, SEQ_OFFSET = 0x091A0155, 7
NOISE_VARS, TX_SCALING = np.array([0.01, 0.03], np.float32), 0.7071
# symbols to cf32, symbols to ci8, REs to equalise (not a multiple of EQ_RES 4: the estimates lie 8 n bytes behind the
# symbols), REs to precode, symbols to demodulate, LLRs to descramble (one past a 32-bit sequence word)
SMALL = dict(qpsk=3, qam256=5, eq=5, pc=7, dm=3, ds=33)
LARGE = dict(qpsk=4097, qam256=4097, eq=4097, pc=4097, dm=4097, ds=4097)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


@functools.lru_cache(maxsize=2)
def _vectors(large):
    """Per stage (inputs, expected output as integers), computed once per size set"""
    n, seed = (LARGE, 900) if large else (SMALL, 800)
    rng = np.random.default_rng(seed)
    v = {}
    for name, mod, levels in (("qpsk", 2, False), ("qam256", 8, True)):
        bits = rng.integers(0, 2, n[name] * mod).astype(np.uint8)
        v[name] = (np.packbits(bits), M.levels(bits, mod) if levels else _u32(M.modulate(bits, mod)))
    sym, est = E.case_input(dict(ports=2, layers=2, n=n["eq"], seed=seed))
    eq_sym, eq_var = E.equalize(E.ZF, sym, est, NOISE_VARS, np.float32(TX_SCALING))
    v["eq"] = ((np.ascontiguousarray(sym), np.ascontiguousarray(est)), (_u32(eq_sym), E.bits_of(eq_var).reshape(-1)))
    ci8, _, w = R.case_input(dict(form="compact", layers=2, ports=2, n=n["pc"], seed=seed, qm=4))
    v["pc"] = ((np.ascontiguousarray(ci8), np.ascontiguousarray(w)), _u32(R.apply_layer_map_and_precoding(ci8, w)))
    _, dsym, dnv = noisy_symbols(rng, n["dm"], 4, noise_var=0.1)
    v["dm"] = ((dsym, dnv), O.demodulate_soft(4, dsym, dnv))
    llr = rng.integers(-127, 128, n["ds"]).astype(np.int8)
    v["ds"] = (llr, S.descramble(llr, C_INIT, SEQ_OFFSET))
    return n, v


def _stages(ctx, large):
    """name -> a call of the stage's *_sync entry point on the size set: (return code, output, expected)"""
    from srsran_projectvtlmo_amd import _lib
    L, h = _lib.load(), ctx.handle
    n, v = _vectors(large)

    def modulate(name, mod, fmt, dtype):
        out = np.zeros((n[name], 2), dtype)
        rc = L.ldpc_hip_modulate_sync(h, n[name], mod, v[name][0].ctypes.data, out.ctypes.data, fmt)
        return rc, [(out if dtype == np.int8 else _u32(out), v[name][1])]

    def equalize():
        (sym, est), (want_sym, want_var) = v["eq"]
        out, var = np.zeros(2 * n["eq"], np.complex64), np.zeros(2 * n["eq"], np.float32)
        rc = L.ldpc_hip_equalize_sync(h, E.ZF, n["eq"], 2, 2, sym.ctypes.data, est.ctypes.data, NOISE_VARS.ctypes.data,
                                      TX_SCALING, out.ctypes.data, var.ctypes.data)
        return rc, [(_u32(out), want_sym), (_u32(var), want_var)]

    def precode():
        (ci8, w), want = v["pc"]
        out = np.zeros((2, n["pc"]), np.complex64)
        rc = L.ldpc_hip_precode_sync(h, n["pc"], 2, 2, ci8.ctypes.data, _lib.SYM_CI8, w.ctypes.data, out.ctypes.data)
        return rc, [(_u32(out), want)]

    def demodulate():
        (sym, nv), want = v["dm"]
        out = np.zeros(4 * n["dm"], np.int8)
        rc = L.ldpc_hip_demodulate_sync(h, n["dm"], 4, sym.ctypes.data, nv.ctypes.data, out.ctypes.data)
        return rc, [(out, want)]

    def descramble():
        llr, want = v["ds"]
        out = np.zeros(n["ds"], np.int8)
        rc = L.ldpc_hip_descramble_sync(h, C_INIT, SEQ_OFFSET, n["ds"], llr.ctypes.data, out.ctypes.data)
        return rc, [(out, want)]

    return {"modulate qpsk cf32": lambda: modulate("qpsk", 2, _lib.SYM_CF32, np.float32),
            "modulate 256-QAM ci8": lambda: modulate("qam256", 8, _lib.SYM_CI8, np.int8),
            "equalize": equalize, "precode": precode, "demodulate": demodulate, "descramble": descramble}


def test_stage_sync_calls_share_one_round_trip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srsran_projectvtlmo_amd import _lib
    ctx = _lib.Context(0)
    try:
        L, h, bad = _lib.load(), ctx.handle, []
        for pas, large, reverse in (("first", False, False), ("grown", True, True), ("again", False, False)):
            stages = list(_stages(ctx, large).items())
            for name, call in (reversed(stages) if reverse else stages):
                rc, pairs = call()
                assert rc == _lib.OK, f"{pas} pass, {name}: {rc} {L.ldpc_hip_last_error(h)}"
                if not all(got.shape == want.shape and np.array_equal(got, want) for got, want in pairs):
                    bad.append((pas, name))
        assert not bad, f"outputs that differ from their reference: {bad}"
        # nothing to do is OK before any pointer is looked at (the precoder validates its weights first)
        w = np.ones(4, np.complex64)
        assert L.ldpc_hip_modulate_sync(h, 0, 2, None, None, _lib.SYM_CF32) == _lib.OK
        assert L.ldpc_hip_equalize_sync(h, E.ZF, 0, 2, 2, None, None, None, TX_SCALING, None, None) == _lib.OK
        assert L.ldpc_hip_precode_sync(h, 0, 2, 2, None, _lib.SYM_CI8, w.ctypes.data, None) == _lib.OK
        assert L.ldpc_hip_demodulate_sync(h, 0, 4, None, None, None) == _lib.OK
        assert L.ldpc_hip_descramble_sync(h, C_INIT, SEQ_OFFSET, 0, None, None) == _lib.OK
    finally:
        ctx.close()
