"""The compiled reference (oracle/_ref/libsrsran_ref.so, built by `make -C oracle ref`) -- TEST INFRASTRUCTURE ONLY.

Same call shapes as the oracle's Python functions (oracle/__init__.py), so a test can swap one for the other. The
library is the reference tree's own generic (non-SIMD) classes behind oracle/ref_shim.cpp. It asserts its contracts:
LLRs outside [-120, 120] and +-127, illegal lengths or a scaling factor outside (0, 1) end the process.

The reference's encoder and rate matcher work on packed bits with fillers as zeros; the wrappers translate the
oracle's convention (one bit per byte, fillers marked FILLER_BIT) both ways.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

from . import BG_K, BG_N_SHORT, FILLER_BIT, NO_CRC, bits_per_symbol

LIB_PATH = Path(__file__).resolve().parent / "_ref" / "libsrsran_ref.so"

_lib = None


def available() -> bool:
    return LIB_PATH.exists()


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(str(LIB_PATH))
        i8p = ctypes.POINTER(ctypes.c_int8)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        fp = ctypes.POINTER(ctypes.c_float)
        U = ctypes.c_uint
        I = ctypes.c_int
        sig = {
            "ref_ldpc_decode": (I, [I, U, U, i8p, U, U, ctypes.c_float, I, u8p]),
            "ref_rate_dematch": (I, [i8p, U, i8p, U, I, U, U, U, U]),
            "ref_ldpc_encode": (I, [I, U, u8p, u8p, U]),
            "ref_rate_match": (I, [u8p, U, u8p, U, U, U, U, I, U]),
            "ref_demodulate_soft": (I, [I, U, fp, fp, i8p]),
            "ref_descramble": (I, [U, U, U, i8p, i8p]),
            "ref_scramble_packed": (I, [U, U, U, u8p, u8p]),
            "ref_crc_bits": (ctypes.c_uint32, [I, u8p, U]),
            "ref_crc_packed": (ctypes.c_uint32, [I, u8p, U]),
            "ref_llr_add": (ctypes.c_int8, [ctypes.c_int8, ctypes.c_int8]),
            "ref_llr_promotion_sum": (ctypes.c_int8, [ctypes.c_int8, ctypes.c_int8]),
            "ref_llr_quantize": (ctypes.c_int8, [ctypes.c_float, ctypes.c_float]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _p(a: np.ndarray, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def llr_add(a: int, b: int) -> int:
    return int(lib().ref_llr_add(a, b))


def llr_promotion_sum(a: int, b: int) -> int:
    return int(lib().ref_llr_promotion_sum(a, b))


def llr_quantize(x: float, r: float) -> int:
    return int(lib().ref_llr_quantize(x, r))


def crc_bits(poly: int, bits: np.ndarray) -> int:
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    return int(lib().ref_crc_bits(poly, _p(bits, ctypes.c_uint8), bits.size))


def crc_packed(poly: int, packed: np.ndarray, nbits: int) -> int:
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    return int(lib().ref_crc_packed(poly, _p(packed, ctypes.c_uint8), nbits))


def ldpc_decode(bg: int, Z: int, llr: np.ndarray, max_iterations: int, crc_poly: int = NO_CRC,
                nof_filler_bits: int = 0, scaling_factor: float = 0.8, out: np.ndarray | None = None):
    """ldpc_decoder_generic::decode on a fresh object. Returns (packed message bytes, iterations-or-None)."""
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    if out is None:
        out = np.zeros((BG_K[bg] * Z + 7) // 8, dtype=np.uint8)
    r = lib().ref_ldpc_decode(bg, Z, nof_filler_bits, _p(llr, ctypes.c_int8), llr.size, max_iterations,
                              scaling_factor, crc_poly, _p(out, ctypes.c_uint8))
    return out, (r if r > 0 else None)


def rate_dematch(out: np.ndarray, llr_e: np.ndarray, new_data: bool, rv: int, Qm: int, Nref: int,
                 nof_filler_bits: int) -> np.ndarray:
    """ldpc_rate_dematcher_impl::rate_dematch, in place on `out` (the soft buffer, N LLRs)."""
    assert out.dtype == np.int8 and out.flags.c_contiguous
    llr_e = np.ascontiguousarray(llr_e, dtype=np.int8)
    lib().ref_rate_dematch(_p(out, ctypes.c_int8), out.size, _p(llr_e, ctypes.c_int8), llr_e.size, int(new_data), rv,
                           Qm, Nref, nof_filler_bits)
    return out


def ldpc_encode(bg: int, Z: int, msg_bits: np.ndarray, cb_len: int | None = None) -> np.ndarray:
    """ldpc_encoder_generic::encode. msg_bits and the result in the oracle's convention (fillers FILLER_BIT)."""
    msg_bits = np.ascontiguousarray(msg_bits, dtype=np.uint8)
    assert msg_bits.size == BG_K[bg] * Z
    if cb_len is None:
        cb_len = BG_N_SHORT[bg] * Z
    filler = msg_bits == FILLER_BIT
    packed = np.packbits(np.where(filler, 0, msg_bits).astype(np.uint8))
    cw = np.zeros((cb_len + 7) // 8, dtype=np.uint8)
    lib().ref_ldpc_encode(bg, Z, _p(packed, ctypes.c_uint8), _p(cw, ctypes.c_uint8), cb_len)
    bits = np.unpackbits(cw)[:cb_len].copy()
    f = filler[2 * Z:][:cb_len]
    bits[:f.size][f] = FILLER_BIT
    return bits


def rate_match(cw_bits: np.ndarray, E: int, rv: int, Qm: int, Nref: int, bg: int, Z: int) -> np.ndarray:
    """ldpc_rate_matcher_impl::rate_match. cw_bits in the oracle's convention; E output bits, one per byte."""
    cw_bits = np.ascontiguousarray(cw_bits, dtype=np.uint8)
    filler = cw_bits == FILLER_BIT
    packed = np.packbits(np.where(filler, 0, cw_bits).astype(np.uint8))
    out = np.zeros((E + 7) // 8, dtype=np.uint8)
    lib().ref_rate_match(_p(out, ctypes.c_uint8), E, _p(packed, ctypes.c_uint8), cw_bits.size, rv, Qm, Nref, bg,
                         int(filler.sum()))
    return np.unpackbits(out)[:E].copy()


def demodulate_soft(mod: int, symbols: np.ndarray, noise_vars: np.ndarray) -> np.ndarray:
    """demodulation_mapper_impl::demodulate_soft."""
    sym = np.ascontiguousarray(symbols, dtype=np.complex64)
    nv = np.ascontiguousarray(noise_vars, dtype=np.float32)
    assert sym.size == nv.size
    out = np.zeros(sym.size * bits_per_symbol(mod), dtype=np.int8)
    fp = ctypes.POINTER(ctypes.c_float)
    lib().ref_demodulate_soft(mod, sym.size, sym.view(np.float32).ctypes.data_as(fp), nv.ctypes.data_as(fp),
                              _p(out, ctypes.c_int8))
    return out


def descramble(llr: np.ndarray, c_init: int, offset: int = 0) -> np.ndarray:
    """pseudo_random_generator_impl: init(c_init), advance(offset), apply_xor on int8 LLRs."""
    llr = np.ascontiguousarray(llr, dtype=np.int8)
    out = np.zeros_like(llr)
    lib().ref_descramble(c_init, offset, llr.size, _p(llr, ctypes.c_int8), _p(out, ctypes.c_int8))
    return out


def xor_packed(data: np.ndarray, c_init: int, offset: int, nbits: int) -> np.ndarray:
    """The same generator's apply_xor on packed bits (MSB first)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros((nbits + 7) // 8, dtype=np.uint8)
    lib().ref_scramble_packed(c_init, offset, nbits, _p(data, ctypes.c_uint8), _p(out, ctypes.c_uint8))
    return out
