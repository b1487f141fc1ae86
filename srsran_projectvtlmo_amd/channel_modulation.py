"""Modulation and soft demodulation mappers on the MI355X: the Python mirror of srsRAN's
`modulation_mapper` and `demodulation_mapper` interfaces (include/srsran/phy/upper/channel_modulation/
modulation_mapper.h, demodulation_mapper.h:46-70) and of `channel_modulation_factory::create_modulation_mapper` /
`create_demodulation_mapper` (channel_modulation_factories.h:32-39), on top of the C ABI (`ldpc_hip_modulate_sync` /
`ldpc_hip_modulate_launch` / `ldpc_hip_rate_match_modulate_launch`, `ldpc_hip_demodulate_sync` /
`ldpc_hip_demodulate_launch`, include/srsran_ldpc_hip.h).

The symbols are the reference's float32 table (modulation_mapper_lut_impl.cpp) bit for bit; the LLRs are those of the
reference's portable per-symbol functions (demodulation_mapper_impl.cpp:33-76,
demodulation_mapper_{qpsk,qam16,qam64,qam256}.cpp scalar loops) bit for bit. There is no CPU fallback: without the HIP
library or a GPU the calls raise."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from enum import IntEnum
from typing import Optional, Sequence

import numpy as np

from . import _lib


class modulation_scheme(IntEnum):
    """include/srsran/ran/sch/modulation_scheme.h:39-52."""
    PI_2_BPSK = 0
    BPSK = 1
    QPSK = 2
    QAM16 = 4
    QAM64 = 6
    QAM256 = 8


def get_bits_per_symbol(mod: int) -> int:
    """modulation_scheme.h get_bits_per_symbol: 1 for (pi/2-)BPSK, else the scheme's value."""
    return 1 if int(mod) in (0, 1) else int(mod)


class demodulation_mapper:
    """demodulation_mapper.h:46-70."""

    def demodulate_soft(self, llrs: np.ndarray, symbols: np.ndarray, noise_vars: np.ndarray,
                        mod: modulation_scheme) -> None:
        raise NotImplementedError


class demodulation_mapper_hip(demodulation_mapper):
    """demodulate_soft on the GPU: host spans in, host LLRs out (one HIP round trip)."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx if ctx is not None else _lib.default_context()

    def demodulate_soft(self, llrs, symbols, noise_vars, mod):
        sym = np.ascontiguousarray(symbols, dtype=np.complex64)
        nv = np.ascontiguousarray(noise_vars, dtype=np.float32)
        # demodulation_mapper_impl.cpp:82-83 (srsran_assert)
        if sym.size != nv.size:
            raise ValueError("Inputs symbols and noise_vars must have the same length.")
        if sym.size * get_bits_per_symbol(mod) != llrs.size or llrs.dtype != np.int8:
            raise ValueError("Input and output lengths are incompatible.")
        out = llrs if llrs.flags.c_contiguous else np.empty_like(llrs)
        _lib.check(self.ctx.handle,
                   _lib.load().ldpc_hip_demodulate_sync(self.ctx.handle, sym.size, int(mod), sym.ctypes.data,
                                                         nv.ctypes.data, out.ctypes.data),
                   "ldpc_hip_demodulate_sync")
        if out is not llrs:
            llrs[...] = out


def get_modulation_scaling(mod: int) -> np.float32:
    """modulation_mapper::get_modulation_scaling (ldpc_hip_modulation_scaling, host only): the factor that takes the
    ci8 levels to unit mean power; 0.0 for a value that is no scheme."""
    return np.float32(_lib.load().ldpc_hip_modulation_scaling(int(mod)))


class modulation_mapper:
    """modulation_mapper.h: modulate(span<cf_t> | span<ci8_t>, bit_buffer, scheme) and get_modulation_scaling."""

    def modulate(self, symbols: np.ndarray, bits_packed: np.ndarray, mod: modulation_scheme, nof_bits: int = -1):
        raise NotImplementedError

    @staticmethod
    def get_modulation_scaling(mod: modulation_scheme) -> np.float32:
        return get_modulation_scaling(mod)


class modulation_mapper_hip(modulation_mapper):
    """modulate on the GPU: packed host bits in, host symbols out (one HIP round trip). `symbols` is a complex64 array
    (nothing is returned) or an int8 array of shape (n, 2) holding (re, im) levels (the scaling is returned, as the
    reference's ci8 overload returns it). The packed bytes must hold exactly the symbols' Qm x n bits; `nof_bits`,
    when given, is the bit buffer's size and must equal that."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx if ctx is not None else _lib.default_context()

    def modulate(self, symbols, bits_packed, mod, nof_bits=-1):
        ci8 = symbols.dtype == np.int8
        if ci8:
            if symbols.ndim != 2 or symbols.shape[1] != 2:
                raise ValueError("int8 symbols must have shape (n, 2).")
            n = symbols.shape[0]
        elif symbols.dtype == np.complex64:
            n = symbols.size
        else:
            raise ValueError("symbols must be complex64 or int8 (n, 2).")
        bits = np.ascontiguousarray(bits_packed, dtype=np.uint8)
        need = get_bits_per_symbol(mod) * n
        # modulation_mapper_lut_impl.cpp (srsran_assert): the bit buffer holds Qm bits per symbol
        if bits.size != (need + 7) // 8 or (nof_bits >= 0 and nof_bits != need):
            raise ValueError("The number of bits must be equal to the number of symbols times the bits per symbol.")
        out = symbols if symbols.flags.c_contiguous else np.empty_like(symbols)
        _lib.check(self.ctx.handle,
                   _lib.load().ldpc_hip_modulate_sync(self.ctx.handle, n, int(mod), bits.ctypes.data, out.ctypes.data,
                                                       _lib.SYM_CI8 if ci8 else _lib.SYM_CF32),
                   "ldpc_hip_modulate_sync")
        if out is not symbols:
            symbols[...] = out
        return get_modulation_scaling(mod) if ci8 else None


class channel_modulation_factory:
    """channel_modulation_factories.h:32-39: the modulation mapper and the demodulation mapper."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx

    def create_modulation_mapper(self) -> modulation_mapper:
        return modulation_mapper_hip(self.ctx)

    def create_demodulation_mapper(self) -> demodulation_mapper:
        return demodulation_mapper_hip(self.ctx)


def create_channel_modulation_hip_factory(ctx: Optional[_lib.Context] = None) -> channel_modulation_factory:
    return channel_modulation_factory(ctx)


@dataclass
class demod_segment:
    """One ldpc_hip_demod_desc: offsets in symbols / floats / bytes from the launch's base pointers."""
    nof_symbols: int
    modulation: int
    symbol_offset: int = 0
    noise_offset: int = 0
    llr_offset: int = 0


def demod_descriptors(segments: Sequence[demod_segment]):
    """The ldpc_hip_demod_desc array of `segments` (build once, launch many times)."""
    arr = (_lib.DemodDesc * max(len(segments), 1))()
    for i, s in enumerate(segments):
        arr[i].symbol_offset = s.symbol_offset
        arr[i].noise_offset = s.noise_offset
        arr[i].llr_offset = s.llr_offset
        arr[i].nof_symbols = s.nof_symbols
        arr[i].modulation = int(s.modulation)
    return arr


def demodulate_launch(ctx: _lib.Context, segments, d_symbols: int, d_noise_vars: int, d_llrs: int,
                      stream: int = 0, n: int = -1) -> None:
    """ldpc_hip_demodulate_launch on device pointers (asynchronous on `stream`). `segments`: a sequence of
    demod_segment, or a prebuilt demod_descriptors() array with its length n."""
    if n < 0:
        n = len(segments)
        arr = demod_descriptors(segments)
    else:
        arr = segments
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_demodulate_launch(ctx.handle, n, arr, ctypes.c_void_p(d_symbols),
                                                      ctypes.c_void_p(d_noise_vars), ctypes.c_void_p(d_llrs),
                                                      ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_demodulate_launch")


@dataclass
class mod_segment:
    """One ldpc_hip_mod_desc: nof_symbols symbols of one scheme; bit_offset in bytes and symbol_offset in symbols from
    the launch's base pointers. scramble: the bits meet c(seq_offset ..) of c_init before they are mapped."""
    nof_symbols: int
    modulation: int
    bit_offset: int = 0
    symbol_offset: int = 0
    scramble: bool = False
    c_init: int = 0
    seq_offset: int = 0


def mod_descriptors(segments: Sequence[mod_segment]):
    """The ldpc_hip_mod_desc array of `segments` (build once, launch many times)."""
    arr = (_lib.ModDesc * max(len(segments), 1))()
    for i, s in enumerate(segments):
        arr[i].bit_offset, arr[i].symbol_offset, arr[i].seq_offset = s.bit_offset, s.symbol_offset, s.seq_offset
        arr[i].nof_symbols, arr[i].c_init = s.nof_symbols, s.c_init
        arr[i].modulation, arr[i].scramble = int(s.modulation), int(bool(s.scramble))
    return arr


def modulate_launch(ctx: _lib.Context, segments, d_bits: int, d_symbols: int, fmt: int = _lib.SYM_CF32,
                    stream: int = 0, n: int = -1) -> None:
    """ldpc_hip_modulate_launch on device pointers (asynchronous on `stream`). `segments`: a sequence of mod_segment,
    or a prebuilt mod_descriptors() array with its length n. fmt: _lib.SYM_CF32 or _lib.SYM_CI8."""
    if n < 0:
        n = len(segments)
        arr = mod_descriptors(segments)
    else:
        arr = segments
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_modulate_launch(ctx.handle, n, arr, ctypes.c_void_p(d_bits),
                                                    ctypes.c_void_p(d_symbols), fmt,
                                                    ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_modulate_launch")


def rate_match_modulate_launch(ctx: _lib.Context, rm_specs, segments: Sequence[mod_segment], d_cws: int,
                               d_symbols: int, fmt: int = _lib.SYM_CF32, stream: int = 0) -> None:
    """ldpc_hip_rate_match_modulate_launch: codeblock i is rate-matched as channel_coding.cb_rate_match_spec
    rm_specs[i] says (its out_offset is unused), scrambled and mapped as segments[i] says (its bit_offset is unused),
    in one launch with no packed-bit round trip."""
    if len(rm_specs) != len(segments):
        raise ValueError("one mod_segment per rate-match spec")
    rm = (_lib.RmDesc * max(1, len(rm_specs)))()
    for a, sp in zip(rm, rm_specs):
        a.cw_offset, a.out_offset, a.cb_length, a.rm_length = sp.cw_offset, sp.out_offset, sp.cb_length, sp.rm_length
        a.Nref, a.nof_filler_bits, a.modulation_order, a.rv = sp.Nref, sp.nof_filler_bits, sp.modulation_order, sp.rv
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_rate_match_modulate_launch(ctx.handle, len(rm_specs), rm,
                                                               mod_descriptors(segments), ctypes.c_void_p(d_cws),
                                                               ctypes.c_void_p(d_symbols), fmt,
                                                               ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_rate_match_modulate_launch")
