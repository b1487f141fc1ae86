"""The channel equalizer on the MI355X: the Python mirror of srsRAN's `channel_equalizer` interface
(include/srsran/phy/upper/equalization/channel_equalizer.h:37-102), of `channel_equalizer_algorithm_type` and of
`create_channel_equalizer_generic_factory` (equalization_factories.h:35-50), on top of the C ABI
(`ldpc_hip_equalize_sync` / `ldpc_hip_equalize_launch`, include/srsran_ldpc_hip.h).

The equalised symbols and the post-equalisation noise variances are those of the reference's scalar loops
(equalize_zf_1xn.h:136-178, equalize_mmse_1xn.h:56-96, equalize_zf_2xn.h:182-252) bit for bit. Topologies: ZF and MMSE
with one layer on 1 to 4 receive ports, ZF with two layers on 2 or 4 ports; anything else raises. There is no CPU
fallback: without the HIP library or a GPU the calls raise.

cbf16 arrays are uint16[..., 2] (bf16 re, bf16 im): ch_symbols [port, re], ch_estimates [layer, port, re]."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Optional, Sequence

import numpy as np

from . import _lib


class channel_equalizer_algorithm_type(IntEnum):
    """channel_equalizer_algorithm_type.h; the values are LDPC_HIP_EQ_ZF / LDPC_HIP_EQ_MMSE."""
    zf = 0
    mmse = 1


def to_cbf16(z) -> np.ndarray:
    """complex -> uint16[..., 2], each component rounded to nearest, ties to even (bf16.h:38-55)."""
    z = np.asarray(z, np.complex64)
    u = np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def from_cbf16(a) -> np.ndarray:
    """uint16[..., 2] -> complex64: bits << 16 (bf16.h:58-72)."""
    f = (np.asarray(a, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    z = np.empty(f.shape[:-1], np.complex64)      # component by component: 1j * inf would make a NaN
    z.real, z.imag = f[..., 0], f[..., 1]
    return z


def equalize_supported(algorithm: int, nof_rx_ports: int, nof_tx_layers: int) -> bool:
    """ldpc_hip_equalize_supported (host only)."""
    return bool(_lib.load().ldpc_hip_equalize_supported(int(algorithm), nof_rx_ports, nof_tx_layers))


class channel_equalizer:
    """channel_equalizer.h:37-102."""

    def equalize(self, eq_symbols: np.ndarray, eq_noise_vars: np.ndarray, ch_symbols: np.ndarray,
                 ch_estimates: np.ndarray, noise_var_estimates, tx_scaling: float) -> None:
        raise NotImplementedError


def _cbf16_planes(a, ndim: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint16 or a.ndim != ndim + 1 or a.shape[-1] != 2:
        raise ValueError(f"{what} must be cbf16: uint16 of shape ({'layer, ' if ndim == 3 else ''}port, re, 2).")
    return a


class channel_equalizer_hip(channel_equalizer):
    """equalize on the GPU: host arrays in, host arrays out (one HIP round trip). eq_symbols is complex64 and
    eq_noise_vars float32, both of nof_re x layers elements, two layers interleaved per RE."""

    def __init__(self, type: channel_equalizer_algorithm_type = channel_equalizer_algorithm_type.zf,
                 ctx: Optional[_lib.Context] = None):
        self.type = channel_equalizer_algorithm_type(type)
        self.ctx = ctx if ctx is not None else _lib.default_context()

    def equalize(self, eq_symbols, eq_noise_vars, ch_symbols, ch_estimates, noise_var_estimates, tx_scaling):
        sym = _cbf16_planes(ch_symbols, 2, "ch_symbols")
        est = _cbf16_planes(ch_estimates, 3, "ch_estimates")
        nv = np.ascontiguousarray(noise_var_estimates, dtype=np.float32)
        L, P, n = est.shape[:3]
        # channel_equalizer_generic_impl.cpp assert_sizes (srsran_assert)
        if sym.shape[:2] != (P, n) or nv.size != P:
            raise ValueError("Number of Rx ports or of REs does not match.")
        if eq_symbols.size != n * L or eq_noise_vars.size != n * L:
            raise ValueError("The number of channel estimates and layers is not consistent with the equalized REs.")
        if eq_symbols.dtype != np.complex64 or eq_noise_vars.dtype != np.float32:
            raise ValueError("eq_symbols must be complex64 and eq_noise_vars float32.")
        out = eq_symbols if eq_symbols.flags.c_contiguous else np.empty(eq_symbols.shape, np.complex64)
        var = eq_noise_vars if eq_noise_vars.flags.c_contiguous else np.empty(eq_noise_vars.shape, np.float32)
        _lib.check(self.ctx.handle,
                   _lib.load().ldpc_hip_equalize_sync(self.ctx.handle, int(self.type), n, P, L, sym.ctypes.data,
                                                      est.ctypes.data, nv.ctypes.data, float(tx_scaling),
                                                      out.ctypes.data, var.ctypes.data),
                   "ldpc_hip_equalize_sync")
        if out is not eq_symbols:
            eq_symbols[...] = out
        if var is not eq_noise_vars:
            eq_noise_vars[...] = var


class channel_equalizer_factory:
    """equalization_factories.h:35-44."""

    def __init__(self, type=channel_equalizer_algorithm_type.zf, ctx: Optional[_lib.Context] = None):
        self.type, self.ctx = channel_equalizer_algorithm_type(type), ctx

    def create(self) -> channel_equalizer:
        return channel_equalizer_hip(self.type, self.ctx)


def create_channel_equalizer_hip_factory(type=channel_equalizer_algorithm_type.zf,
                                         ctx: Optional[_lib.Context] = None) -> channel_equalizer_factory:
    return channel_equalizer_factory(type, ctx)


@dataclass
class eq_segment:
    """One ldpc_hip_eq_desc: nof_re REs of one topology. Offsets and strides in cbf16 elements from the launch's
    d_ch_symbols / d_ch_estimates (port p's symbols at sym_offset + p sym_stride, plane (port p, layer l) at est_offset
    + (l nof_rx_ports + p) est_stride; a stride of 0 means nof_re); out_offset in symbols / floats from d_eq_symbols /
    d_eq_noise_vars."""
    nof_re: int
    nof_rx_ports: int
    nof_tx_layers: int
    noise_vars: Sequence[float] = field(default_factory=list)
    algorithm: int = 0
    tx_scaling: float = 1.0
    sym_offset: int = 0
    est_offset: int = 0
    out_offset: int = 0
    sym_stride: int = 0
    est_stride: int = 0


def eq_descriptors(segments: Sequence[eq_segment]):
    """The ldpc_hip_eq_desc array of `segments` (build once, launch many times)."""
    arr = (_lib.EqDesc * max(len(segments), 1))()
    for a, s in zip(arr, segments):
        a.sym_offset, a.est_offset, a.out_offset = s.sym_offset, s.est_offset, s.out_offset
        a.sym_stride, a.est_stride = s.sym_stride or s.nof_re, s.est_stride or s.nof_re
        a.nof_re, a.tx_scaling = s.nof_re, s.tx_scaling
        if not 0 <= s.nof_rx_ports < 256 or not 0 <= s.nof_tx_layers < 256 or not 0 <= int(s.algorithm) < 256:
            raise ValueError("algorithm, ports and layers are 8-bit fields")
        if len(s.noise_vars) > 4:
            raise ValueError("at most 4 receive ports")
        for p, v in enumerate(s.noise_vars):
            a.noise_var[p] = v
        a.algorithm, a.nof_rx_ports, a.nof_tx_layers = int(s.algorithm), s.nof_rx_ports, s.nof_tx_layers
    return arr


def equalize_launch(ctx: _lib.Context, segments, d_ch_symbols: int, d_ch_estimates: int, d_eq_symbols: int,
                    d_eq_noise_vars: int, stream: int = 0, n: int = -1) -> None:
    """ldpc_hip_equalize_launch on device pointers (asynchronous on `stream`). `segments`: a sequence of eq_segment, or
    a prebuilt eq_descriptors() array with its length n."""
    if n < 0:
        n = len(segments)
        arr = eq_descriptors(segments)
    else:
        arr = segments
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_equalize_launch(ctx.handle, n, arr, ctypes.c_void_p(d_ch_symbols),
                                                    ctypes.c_void_p(d_ch_estimates), ctypes.c_void_p(d_eq_symbols),
                                                    ctypes.c_void_p(d_eq_noise_vars),
                                                    ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_equalize_launch")
