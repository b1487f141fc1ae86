"""Layer mapping and precoding on the MI355X: the Python mirror of srsRAN's `channel_precoder` interface
(include/srsran/phy/generic_functions/precoding/channel_precoder.h) and of `create_channel_precoder_factory("generic")`
(precoding_factories.h), and the row form of `resource_grid_mapper_impl::map(symbol_buffer&, ...)` with re_skip == 0,
on top of the C ABI (`ldpc_hip_precode_sync` / `ldpc_hip_precode_map_launch`, include/srsran_ldpc_hip.h).

The outputs are those of the reference's scalar loops (channel_precoder_generic.cpp:27-70) bit for bit, and the grid's
cbf16 REs those of resource_grid_writer_impl.cpp:44-81. Topologies: every 1 <= layers <= ports <= 4; anything else
raises. A weight component must be finite and below 2^64 in magnitude. There is no CPU fallback: without the HIP
library or a GPU the calls raise.

ci8 arrays are int8[..., 2] (re, im); the grid is cbf16, uint16[port, symbol, subcarrier, 2] (bf16 re, bf16 im)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib

NRE = 12


def precode_supported(nof_layers: int, nof_ports: int) -> bool:
    """ldpc_hip_precode_supported (host only)."""
    return bool(_lib.load().ldpc_hip_precode_supported(nof_layers, nof_ports))


def scaled_weights(weights, scaling: float = 1.0) -> np.ndarray:
    """complex64 weights times a real scaling as srsvec::sc_prod does it: (re * s, im * s) in float32."""
    w = np.ascontiguousarray(weights, np.complex64)
    f = w.view(np.float32) * np.float32(scaling)
    return f.astype(np.float32).view(np.complex64).reshape(w.shape)


class channel_precoder:
    """channel_precoder.h."""

    def apply_precoding(self, output: np.ndarray, input: np.ndarray, precoding: np.ndarray) -> None:
        raise NotImplementedError

    def apply_layer_map_and_precoding(self, output: np.ndarray, input: np.ndarray, precoding: np.ndarray) -> None:
        raise NotImplementedError


class channel_precoder_hip(channel_precoder):
    """One PRG on the GPU: host arrays in, host arrays out (one HIP round trip). output is complex64 [port, re],
    precoding complex64 [port, layer] (precoding_weight_matrix)."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx if ctx is not None else _lib.default_context()

    def _run(self, output, inp, fmt, nof_re, precoding):
        w = np.ascontiguousarray(precoding, np.complex64)
        if w.ndim != 2 or output.ndim != 2 or output.dtype != np.complex64:
            raise ValueError("output must be complex64 [port, re] and precoding [port, layer].")
        P, L = w.shape
        # channel_precoder_impl.cpp:36-57 (srsran_assert)
        if output.shape != (P, nof_re):
            raise ValueError("The output's ports or REs do not match the input and the precoding matrix.")
        out = output if output.flags.c_contiguous else np.empty(output.shape, np.complex64)
        _lib.check(self.ctx.handle,
                   _lib.load().ldpc_hip_precode_sync(self.ctx.handle, nof_re, L, P, inp.ctypes.data, fmt,
                                                     w.ctypes.data, out.ctypes.data),
                   "ldpc_hip_precode_sync")
        if out is not output:
            output[...] = out

    def apply_precoding(self, output, input, precoding):
        """input: complex64 [layer, re]."""
        x = np.ascontiguousarray(input, np.complex64)
        if x.ndim != 2 or x.shape[0] != np.shape(precoding)[1]:
            raise ValueError("The input's layers do not match the precoding matrix.")
        self._run(output, x, _lib.SYM_CF32, x.shape[1], precoding)

    def apply_layer_map_and_precoding(self, output, input, precoding):
        """input: int8 [re * layers, 2], RE r's layer i at r * layers + i."""
        x = np.ascontiguousarray(input)
        L = np.shape(precoding)[1]
        if x.dtype != np.int8 or x.ndim != 2 or x.shape[1] != 2 or x.shape[0] % L != 0:
            raise ValueError("input must be ci8: int8 of shape (re * layers, 2).")
        self._run(output, x, _lib.SYM_CI8, x.shape[0] // L, precoding)


class channel_precoder_factory:
    """precoding_factories.h."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx

    def create(self) -> channel_precoder:
        return channel_precoder_hip(self.ctx)


def create_channel_precoder_hip_factory(ctx: Optional[_lib.Context] = None) -> channel_precoder_factory:
    """Stands for create_channel_precoder_factory("generic")."""
    return channel_precoder_factory(ctx)


def mask_words(mask) -> np.ndarray:
    """A row's subcarrier mask (bool[width]) as 64-bit words: bit k % 64 of word k / 64."""
    m = np.asarray(mask, bool)
    bits = np.zeros((m.size + 63) // 64 * 64, np.uint8)
    bits[:m.size] = m
    return np.packbits(bits, bitorder="little").view("<u8")


def word_prefix(words) -> np.ndarray:
    """Per word, the set bits of the earlier words (what the library computes for the kernel's rank)."""
    cnt = np.array([bin(int(w)).count("1") for w in words], np.uint32)
    return (np.cumsum(cnt, dtype=np.uint64) - cnt).astype(np.uint32)


class precode_rows:
    """The host side of one ldpc_hip_precode_map_launch: rows (ldpc_hip_precode_desc), mask words with their prefix
    counts, and weights. add() turns one transmission into rows; equal masks share their words."""

    def __init__(self):
        self.rows = []          # dicts of the ldpc_hip_precode_desc fields
        self.masks = np.zeros(0, np.uint64)
        self.prefix = np.zeros(0, np.uint32)
        self.weights = np.zeros(0, np.complex64)
        self._known = {}
        self._arrays = None

    def add(self, grid_shape, masks, prg_size: int, weights, scaling: float = 1.0, *, sym_offset: int = 0,
            grid_offset: int = 0, symbol_stride: Optional[int] = None, port_stride: Optional[int] = None) -> int:
        """One transmission on a grid of grid_shape = (ports, symbols, subcarriers): masks bool[symbols, subcarriers]
        (the allocation minus the reserved REs, per OFDM symbol), weights complex[prg, port, layer] for PRGs of
        prg_size RBs counted from subcarrier 0, times `scaling`. Its ci8 symbols start at element sym_offset of the
        launch's d_symbols; its grid starts at cbf16 element grid_offset of d_grid, symbols symbol_stride apart
        (default: subcarriers) and ports port_stride apart (default: symbols * symbol_stride). Returns the number of
        masked REs: the transmission reads that many times `layers` symbols."""
        nports, nsym, nsubc = grid_shape
        masks = np.asarray(masks, bool)
        w = scaled_weights(weights, scaling)
        if masks.shape != (nsym, nsubc) or w.ndim != 3:
            raise ValueError("masks must be bool[symbols, subcarriers] and weights complex[prg, port, layer].")
        nprg, P, L = w.shape
        if P > nports:
            raise ValueError("The precoding number of ports exceeds the grid number of ports.")
        symbol_stride = nsubc if symbol_stride is None else symbol_stride
        port_stride = nsym * symbol_stride if port_stride is None else port_stride
        weight_offset = self.weights.size
        self.weights = np.concatenate([self.weights, w.reshape(-1)])
        count = 0
        for l in range(nsym):
            n = int(masks[l].sum())
            if n == 0:
                continue
            words = mask_words(masks[l])
            key = words.tobytes()
            if key not in self._known:
                self._known[key] = self.masks.size
                self.masks = np.concatenate([self.masks, words])
                self.prefix = np.concatenate([self.prefix, word_prefix(words)])
            self.rows.append(dict(sym_offset=sym_offset + L * count, grid_offset=grid_offset + l * symbol_stride,
                                  port_stride=port_stride, mask_offset=self._known[key], weight_offset=weight_offset,
                                  nof_prg=nprg, width=nsubc, prg_size=prg_size, nof_layers=L, nof_ports=P))
            count += n
        self._arrays = None
        return count

    def descriptors(self):
        """(ldpc_hip_precode_desc array, float32 weights, uint64 masks), built once."""
        if self._arrays is None:
            arr = (_lib.PrecodeDesc * max(len(self.rows), 1))()
            for a, r in zip(arr, self.rows):
                for k, v in r.items():
                    setattr(a, k, v)
            self._arrays = (arr, np.ascontiguousarray(self.weights).view(np.float32),
                            np.ascontiguousarray(self.masks, np.uint64))
        return self._arrays


def precode_map_launch(ctx: _lib.Context, rows: precode_rows, d_symbols: int, d_grid: int, stream: int = 0) -> None:
    """ldpc_hip_precode_map_launch on device pointers (asynchronous on `stream`): d_symbols ci8, d_grid cbf16."""
    arr, w, m = rows.descriptors()
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_precode_map_launch(ctx.handle, len(rows.rows), arr, w.ctypes.data, w.size // 2,
                                                       m.ctypes.data, m.size, ctypes.c_void_p(d_symbols),
                                                       ctypes.c_void_p(d_grid),
                                                       ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_precode_map_launch")
