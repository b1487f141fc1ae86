"""PDSCH DM-RS generation and mapping, and (further down) PUSCH DM-RS channel estimation, on the MI355X. The first
part is the Python mirror of srsRAN's `dmrs_pdsch_processor` interface
(include/srsran/phy/upper/signal_processors/dmrs_pdsch_processor.h) and of `create_dmrs_pdsch_processor_factory_sw`
(signal_processor_factories.h), on top of the C ABI (`ldpc_hip_dmrs_pdsch_map_launch`, include/srsran_ldpc_hip.h).

The grid REs are those of dmrs_pdsch_processor_impl.cpp:84-262 over resource_grid_mapper_impl::map(const
re_buffer_reader&, ...) bit for bit. DM-RS types 1 and 2 at every 1 <= layers <= ports <= 4 and one PRG; anything else
raises. There is no CPU fallback: without the HIP library or a GPU the launch raises.

The grid is on the device: cbf16, uint16[port, symbol, subcarrier, 2] (bf16 re, bf16 im), or, for the values before the
bf16 rounding, cf32 of the same geometry counted in elements."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

NRE = 12
NSYMB = 14
TYPE1, TYPE2 = 1, 2   # dmrs_type::TYPE1 / TYPE2


def dmrs_pdsch_supported(type: int, nof_layers: int, nof_ports: int) -> bool:
    """ldpc_hip_dmrs_pdsch_supported (host only)."""
    return bool(_lib.load().ldpc_hip_dmrs_pdsch_supported(type, nof_layers, nof_ports))


def dmrs_pdsch_c_init(slot_index: int, symbol: int, scrambling_id: int, n_scid: int) -> int:
    """ldpc_hip_dmrs_pdsch_c_init (host only): the sequence's c_init on DM-RS symbol `symbol`."""
    return int(_lib.load().ldpc_hip_dmrs_pdsch_c_init(slot_index, symbol, scrambling_id, n_scid))


def rb_mask_words(rb_mask) -> np.ndarray:
    """An RB mask (bool[nof_rb]) as 64-bit words: bit n % 64 of word n / 64."""
    m = np.asarray(rb_mask, bool)
    bits = np.zeros((m.size + 63) // 64 * 64, np.uint8)
    bits[:m.size] = m
    return np.packbits(bits, bitorder="little").view("<u8")


@dataclass
class config_t:
    """dmrs_pdsch_processor::config_t, with slot_index (slot_point::slot_index()) in place of the slot_point."""
    slot_index: int
    reference_point_k_rb: int
    type: int                  # TYPE1 or TYPE2
    scrambling_id: int
    n_scid: bool
    amplitude: float
    symbols_mask: Sequence     # bool[14]: the OFDM symbols that carry DM-RS
    rb_mask: Sequence          # bool[nof_rb]: the allocation
    precoding: np.ndarray      # complex [port, layer]: one PRG (or [1, port, layer])


@dataclass
class device_grid:
    """A resource grid in device memory: element 0 of (port 0, symbol 0, subcarrier 0) at ptr + offset elements,
    symbols symbol_stride elements apart (default: subcarriers), ports port_stride apart (default: symbols x
    symbol_stride). Elements are cbf16 (4 bytes), or cf32 (8 bytes) with cf32 set."""
    ptr: int
    shape: Tuple[int, int, int]   # (ports, symbols, subcarriers)
    offset: int = 0
    symbol_stride: Optional[int] = None
    port_stride: Optional[int] = None
    cf32: bool = False


class dmrs_rows:
    """The host side of one ldpc_hip_dmrs_pdsch_map_launch: transmissions (ldpc_hip_dmrs_pdsch_desc), RB-mask words
    and weights. add() takes one config_t; equal RB masks share their words."""

    def __init__(self):
        self.rows = []          # dicts of the ldpc_hip_dmrs_pdsch_desc fields
        self.masks = np.zeros(0, np.uint64)
        self.weights = np.zeros(0, np.complex64)
        self._known = {}
        self._arrays = None

    def add(self, grid_shape, config: config_t, *, grid_offset: int = 0, symbol_stride: Optional[int] = None,
            port_stride: Optional[int] = None) -> int:
        """One transmission on a grid of grid_shape = (ports, symbols, subcarriers) that starts at element grid_offset
        of the launch's d_grid, its symbols symbol_stride apart (default: subcarriers) and its ports port_stride apart
        (default: symbols * symbol_stride). Returns the DM-RS REs it writes per antenna port."""
        nports, nsym, nsubc = grid_shape
        w = np.ascontiguousarray(config.precoding, np.complex64)
        if w.ndim == 3:
            if w.shape[0] != 1:
                # dmrs_pdsch_processor_impl.cpp:177 builds each CDM group's precoding with one PRG
                raise ValueError("The DM-RS processor takes one PRG: precoding must be complex[port, layer].")
            w = w[0]
        if w.ndim != 2:
            raise ValueError("precoding must be complex[port, layer].")
        P, L = w.shape
        if P > nports:
            raise ValueError("The precoding number of ports exceeds the grid number of ports.")
        rb = np.asarray(config.rb_mask, bool).reshape(-1)
        sym = np.asarray(config.symbols_mask, bool).reshape(-1)
        if sym.size > nsym or rb.size * NRE > nsubc:
            raise ValueError("The symbol mask or the RB mask exceeds the grid.")
        symbol_stride = nsubc if symbol_stride is None else symbol_stride
        port_stride = nsym * symbol_stride if port_stride is None else port_stride
        words = rb_mask_words(rb)
        key = (rb.size, words.tobytes())
        if key not in self._known:
            self._known[key] = self.masks.size
            self.masks = np.concatenate([self.masks, words])
        weight_offset = self.weights.size
        self.weights = np.concatenate([self.weights, w.reshape(-1)])
        self.rows.append(dict(grid_offset=grid_offset, symbol_stride=symbol_stride, port_stride=port_stride,
                              mask_offset=self._known[key], weight_offset=weight_offset, nof_rb=rb.size, width=nsubc,
                              slot_index=config.slot_index, scrambling_id=config.scrambling_id,
                              reference_point_k_rb=config.reference_point_k_rb, amplitude=float(config.amplitude),
                              symbols_mask=sum(1 << int(l) for l in np.flatnonzero(sym)), type=int(config.type),
                              nof_layers=L, nof_ports=P, n_scid=int(config.n_scid)))
        self._arrays = None
        ncdm = (L + 1) // 2
        return int(rb.sum()) * int(sym.sum()) * ncdm * (6 if config.type == TYPE1 else 4)

    def descriptors(self):
        """(ldpc_hip_dmrs_pdsch_desc array, float32 weights, uint64 RB-mask words), built once."""
        if self._arrays is None:
            arr = (_lib.DmrsPdschDesc * max(len(self.rows), 1))()
            for a, r in zip(arr, self.rows):
                for k, v in r.items():
                    setattr(a, k, v)
            self._arrays = (arr, np.ascontiguousarray(self.weights).view(np.float32),
                            np.ascontiguousarray(self.masks, np.uint64))
        return self._arrays


def dmrs_pdsch_map_launch(ctx: _lib.Context, rows: dmrs_rows, d_grid: int, stream: int = 0,
                          cf32: bool = False) -> None:
    """ldpc_hip_dmrs_pdsch_map_launch on a device pointer (asynchronous on `stream`): d_grid cbf16, or cf32 with cf32
    set (the values before the bf16 rounding, same element offsets and strides)."""
    arr, w, m = rows.descriptors()
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_dmrs_pdsch_map_launch(ctx.handle, len(rows.rows), arr, w.ctypes.data, w.size // 2,
                                                          m.ctypes.data, m.size, ctypes.c_void_p(d_grid),
                                                          _lib.SYM_CF32 if cf32 else _lib.SYM_CBF16,
                                                          ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_dmrs_pdsch_map_launch")


class dmrs_pdsch_processor:
    """dmrs_pdsch_processor.h."""

    def map(self, grid: device_grid, config: config_t) -> None:
        raise NotImplementedError


class dmrs_pdsch_processor_hip(dmrs_pdsch_processor):
    """Generates and maps one transmission's DM-RS into a device grid: one launch, asynchronous on `stream` (default:
    torch's current stream when torch has the GPU open, else the context's)."""

    def __init__(self, ctx: Optional[_lib.Context] = None, stream: int = 0):
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.stream = stream

    def map(self, grid: device_grid, config: config_t) -> None:
        rows = dmrs_rows()
        rows.add(grid.shape, config, grid_offset=grid.offset, symbol_stride=grid.symbol_stride,
                 port_stride=grid.port_stride)
        dmrs_pdsch_map_launch(self.ctx, rows, grid.ptr, self.stream, grid.cf32)


class dmrs_pdsch_processor_factory:
    """signal_processor_factories.h."""

    def __init__(self, ctx: Optional[_lib.Context] = None, stream: int = 0):
        self.ctx, self.stream = ctx, stream

    def create(self) -> dmrs_pdsch_processor:
        return dmrs_pdsch_processor_hip(self.ctx, self.stream)


def create_dmrs_pdsch_processor_hip_factory(ctx: Optional[_lib.Context] = None,
                                            stream: int = 0) -> dmrs_pdsch_processor_factory:
    """Stands for create_dmrs_pdsch_processor_factory_sw(prg_factory)."""
    return dmrs_pdsch_processor_factory(ctx, stream)


# ---- PUSCH DM-RS channel estimation ----------------------------------------------------------------------------------
# The mirror of `dmrs_pusch_estimator` (include/srsran/phy/upper/signal_processors/dmrs_pusch_estimator.h) and of
# `dmrs_pusch_estimator_factory_sw`, on ldpc_hip_dmrs_pusch_estimate_launch: the estimates are those of
# dmrs_pusch_estimator_impl.cpp:71-212 over port_channel_estimator_average_impl.cpp (include/srsran_ldpc_hip.h says
# which values are the reference's bit for bit). DM-RS type 1, 1 to 4 layers on 1 to 4 receive ports, smoothing `none`
# or `filter`, no CFO compensation; anything else raises NotImplementedError.
STRATEGIES = {"none": _lib.CHEST_NONE, "filter": _lib.CHEST_FILTER}


def dmrs_pusch_supported(type: int, nof_layers: int, nof_rx_ports: int, strategy: int = _lib.CHEST_FILTER,
                         compensate_cfo: bool = False) -> bool:
    """ldpc_hip_dmrs_pusch_supported (host only)."""
    return bool(_lib.load().ldpc_hip_dmrs_pusch_supported(type, nof_layers, nof_rx_ports, strategy,
                                                          int(bool(compensate_cfo))))


@dataclass
class pusch_config_t:
    """dmrs_pusch_estimator::configuration, with slot_index (slot_point::slot_index()) and numerology in place of the
    slot_point."""
    slot_index: int
    numerology: int
    type: int                  # TYPE1
    scrambling_id: int
    n_scid: bool
    scaling: float
    symbols_mask: Sequence     # bool[14]: the OFDM symbols that carry DM-RS
    rb_mask: Sequence          # bool[nof_rb]: the allocation
    first_symbol: int
    nof_symbols: int
    nof_tx_layers: int
    rx_ports: Sequence         # the grid ports of the receive ports


@dataclass
class device_channel_estimate:
    """A channel estimate in device memory: element 0 of plane (layer 0, port 0), symbol 0, subcarrier 0 at ptr + offset
    elements, symbols symbol_stride apart (default: subcarriers), planes (layer i, port p) = i ports + p plane_stride
    apart (default: symbols x symbol_stride). Elements are cbf16 (4 bytes), or cf32 (8 bytes) with cf32 set.
    results_ptr takes one ldpc_hip_chest_result per plane from record result_offset; filtered_ptr, when given, the
    filtered pilots (cf32, 6 per allocated RB and plane) from element pilots_offset."""
    ptr: int
    shape: Tuple[int, int, int, int]   # (layers, ports, symbols, subcarriers)
    results_ptr: int
    offset: int = 0
    symbol_stride: Optional[int] = None
    plane_stride: Optional[int] = None
    cf32: bool = False
    result_offset: int = 0
    filtered_ptr: Optional[int] = None
    pilots_offset: int = 0


class chest_rows:
    """The host side of one ldpc_hip_dmrs_pusch_estimate_launch: transmissions (ldpc_hip_dmrs_pusch_desc) and RB-mask
    words. add() takes one pusch_config_t; equal RB masks share their words."""

    def __init__(self):
        self.rows = []          # dicts of the ldpc_hip_dmrs_pusch_desc fields
        self.masks = np.zeros(0, np.uint64)
        self._known = {}
        self._arrays = None

    def add(self, grid_shape, est_shape, config: pusch_config_t, strategy="filter", compensate_cfo=False, *,
            grid_offset: int = 0, grid_symbol_stride: Optional[int] = None, grid_port_stride: Optional[int] = None,
            est_offset: int = 0, symbol_stride: Optional[int] = None, plane_stride: Optional[int] = None,
            pilots_offset: int = 0, result_offset: int = 0) -> int:
        """One transmission: a received grid of grid_shape = (ports, symbols, subcarriers) at element grid_offset of the
        launch's d_grid, and an estimate of est_shape = (layers, ports, symbols, subcarriers) at element est_offset of
        its d_estimates. Returns the transmission's planes."""
        if isinstance(strategy, str):
            if strategy not in STRATEGIES:
                raise NotImplementedError(f"fd_smoothing_strategy {strategy!r}: only 'none' and 'filter'")
            strategy = STRATEGIES[strategy]
        rxp = [int(p) for p in config.rx_ports]
        L, P = int(config.nof_tx_layers), len(rxp)
        if not dmrs_pusch_supported(int(config.type), L, P, int(strategy), compensate_cfo):
            raise NotImplementedError("The PUSCH DM-RS estimator takes DM-RS type 1, 1 to 4 layers on 1 to 4 receive "
                                      "ports, smoothing none or filter, and no CFO compensation.")
        gports, gsym, nsubc = grid_shape
        eL, eP, esym, esubc = est_shape
        rb = np.asarray(config.rb_mask, bool).reshape(-1)
        sym = np.asarray(config.symbols_mask, bool).reshape(-1)
        if L > eL or P > eP or esubc != nsubc or config.first_symbol + config.nof_symbols > esym:
            raise ValueError("The channel estimate is smaller than the transmission.")
        if sym.size > gsym or rb.size * NRE > nsubc or max(rxp) >= gports:
            raise ValueError("The symbol mask, the RB mask or a receive port exceeds the grid.")
        grid_symbol_stride = nsubc if grid_symbol_stride is None else grid_symbol_stride
        grid_port_stride = gsym * grid_symbol_stride if grid_port_stride is None else grid_port_stride
        symbol_stride = nsubc if symbol_stride is None else symbol_stride
        plane_stride = esym * symbol_stride if plane_stride is None else plane_stride
        words = rb_mask_words(rb)
        key = (rb.size, words.tobytes())
        if key not in self._known:
            self._known[key] = self.masks.size
            self.masks = np.concatenate([self.masks, words])
        self.rows.append(dict(grid_offset=grid_offset, grid_symbol_stride=grid_symbol_stride,
                              grid_port_stride=grid_port_stride, est_offset=est_offset, symbol_stride=symbol_stride,
                              plane_stride=plane_stride, pilots_offset=pilots_offset, result_offset=result_offset,
                              mask_offset=self._known[key], nof_rb=rb.size, width=nsubc, grid_ports=gports,
                              slot_index=config.slot_index, scrambling_id=config.scrambling_id,
                              scaling=float(config.scaling),
                              symbols_mask=sum(1 << int(l) for l in np.flatnonzero(sym)), type=int(config.type),
                              nof_layers=L, nof_rx_ports=P, n_scid=int(config.n_scid),
                              first_symbol=int(config.first_symbol), nof_symbols=int(config.nof_symbols),
                              strategy=int(strategy), compensate_cfo=int(bool(compensate_cfo)),
                              rx_ports=tuple(rxp + [0] * (4 - P))))
        self._arrays = None
        return L * P

    def descriptors(self):
        """(ldpc_hip_dmrs_pusch_desc array, uint64 RB-mask words), built once."""
        if self._arrays is None:
            arr = (_lib.DmrsPuschDesc * max(len(self.rows), 1))()
            for a, r in zip(arr, self.rows):
                for k, v in r.items():
                    if k == "rx_ports":
                        a.rx_ports[:] = v
                    else:
                        setattr(a, k, v)
            self._arrays = (arr, np.ascontiguousarray(self.masks, np.uint64))
        return self._arrays


def dmrs_pusch_estimate_launch(ctx: _lib.Context, rows: chest_rows, d_grid: int, d_est: int, d_results: int,
                               stream: int = 0, cf32: bool = False, d_filtered: Optional[int] = None) -> None:
    """ldpc_hip_dmrs_pusch_estimate_launch on device pointers (asynchronous on `stream`): d_grid cbf16; d_est cbf16, or
    cf32 with cf32 set; d_results one ldpc_hip_chest_result per plane; d_filtered, when given, the filtered pilots."""
    arr, m = rows.descriptors()
    _lib.check(ctx.handle,
               _lib.load().ldpc_hip_dmrs_pusch_estimate_launch(
                   ctx.handle, len(rows.rows), arr, m.ctypes.data, m.size, ctypes.c_void_p(d_grid),
                   ctypes.c_void_p(d_est), _lib.SYM_CF32 if cf32 else _lib.SYM_CBF16,
                   ctypes.c_void_p(d_filtered) if d_filtered else None, ctypes.c_void_p(d_results),
                   ctypes.c_void_p(_lib.stream_arg(stream))),
               "ldpc_hip_dmrs_pusch_estimate_launch")


def chest_results(records, scaling: float, symbols_mask, numerology: int = 0):
    """ldpc_hip_dmrs_pusch_finalize (host only) on the records of one transmission's planes: `records` uint32 or bytes
    [planes, 8] as the device wrote them. Returns a list of dicts (epre, rsrp, noise_var, snr, cfo_Hz or None)."""
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)
    sym = np.flatnonzero(np.asarray(symbols_mask, bool))
    l0, l1 = int(sym[0]), int(sym[1]) if sym.size > 1 else 0
    out = []
    for row in rec:
        r = _lib.ChestResult.from_buffer_copy(row.tobytes())
        m = _lib.ChestMetrics()
        rc = _lib.load().ldpc_hip_dmrs_pusch_finalize(ctypes.byref(r), ctypes.c_float(float(scaling)), int(sym.size), l0,
                                                      l1, int(numerology), ctypes.byref(m))
        if rc != _lib.OK:
            raise ValueError("ldpc_hip_dmrs_pusch_finalize: an argument outside its range")
        out.append(dict(epre=m.epre, rsrp=m.rsrp, noise_var=m.noise_var, snr=m.snr,
                        cfo_Hz=m.cfo_Hz if m.has_cfo else None))
    return out


class dmrs_pusch_estimator:
    """dmrs_pusch_estimator.h."""

    def estimate(self, estimate: device_channel_estimate, grid: device_grid, config: pusch_config_t) -> None:
        raise NotImplementedError


class dmrs_pusch_estimator_hip(dmrs_pusch_estimator):
    """Estimates one transmission's channel from a device grid: one launch, asynchronous on `stream` (default: torch's
    current stream when torch has the GPU open, else the context's)."""

    def __init__(self, fd_smoothing_strategy="filter", compensate_cfo=False, ctx: Optional[_lib.Context] = None,
                 stream: int = 0):
        if fd_smoothing_strategy not in STRATEGIES:
            raise NotImplementedError(f"fd_smoothing_strategy {fd_smoothing_strategy!r}: only 'none' and 'filter'")
        if compensate_cfo:
            raise NotImplementedError("CFO compensation is not supported; the CFO is estimated and reported.")
        self.strategy = fd_smoothing_strategy
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self.stream = stream

    def estimate(self, estimate: device_channel_estimate, grid: device_grid, config: pusch_config_t) -> None:
        if grid.cf32:
            raise ValueError("The received grid is cbf16.")
        rows = chest_rows()
        rows.add(grid.shape, estimate.shape, config, self.strategy, grid_offset=grid.offset,
                 grid_symbol_stride=grid.symbol_stride, grid_port_stride=grid.port_stride, est_offset=estimate.offset,
                 symbol_stride=estimate.symbol_stride, plane_stride=estimate.plane_stride,
                 pilots_offset=estimate.pilots_offset, result_offset=estimate.result_offset)
        dmrs_pusch_estimate_launch(self.ctx, rows, grid.ptr, estimate.ptr, estimate.results_ptr, self.stream,
                                   estimate.cf32, estimate.filtered_ptr)


class dmrs_pusch_estimator_factory:
    """signal_processor_factories.h."""

    def __init__(self, fd_smoothing_strategy="filter", compensate_cfo=False, ctx: Optional[_lib.Context] = None,
                 stream: int = 0):
        if fd_smoothing_strategy not in STRATEGIES:
            raise NotImplementedError(f"fd_smoothing_strategy {fd_smoothing_strategy!r}: only 'none' and 'filter'")
        if compensate_cfo:
            raise NotImplementedError("CFO compensation is not supported; the CFO is estimated and reported.")
        self.args = (fd_smoothing_strategy, compensate_cfo, ctx, stream)

    def create(self) -> dmrs_pusch_estimator:
        return dmrs_pusch_estimator_hip(*self.args)


def create_dmrs_pusch_estimator_hip_factory(fd_smoothing_strategy="filter", compensate_cfo=False,
                                            ctx: Optional[_lib.Context] = None,
                                            stream: int = 0) -> dmrs_pusch_estimator_factory:
    """Stands for create_dmrs_pusch_estimator_factory_sw(prg_factory, ch_estimator_factory, strategy, compensate_cfo)."""
    return dmrs_pusch_estimator_factory(fd_smoothing_strategy, compensate_cfo, ctx, stream)
