"""Pseudo-random sequence generator on the MI355X: the Python mirror of srsRAN's `pseudo_random_generator`
(include/srsran/phy/upper/sequence_generators/pseudo_random_generator.h:38-130) on top of the C ABI
(`ldpc_hip_prs_init`, `ldpc_hip_descramble_launch` / `_sync`, `ldpc_hip_scramble_bits_launch`,
include/srsran_ldpc_hip.h).

The sequence is the length-31 Gold sequence of TS 38.211 5.2.1. PUSCH uses it to scramble the codeword bits with
c_init = rnti * 2^15 + n_id; the receiver reverts it on the LLRs after soft demodulation
(pusch_demodulator_impl.cpp:139-140, 289-293). The device generates the sequence; the host only computes start states,
in O(log offset). There is no CPU fallback: without the HIP library the calls raise, and everything but
`init` / `advance` / `get_state` needs a GPU."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib


def pusch_c_init(rnti: int, n_id: int) -> int:
    """pusch_demodulator_impl.cpp:139: c_init = rnti * 2^15 + n_id."""
    return ((int(rnti) << 15) + int(n_id)) & 0x7FFFFFFF


def prs_state(c_init: int, offset: int = 0) -> "state_s":
    """ldpc_hip_prs_init: the generator state `offset` bits into the sequence of c_init (host only, no GPU)."""
    st = _lib.PrsState()
    rc = _lib.load().ldpc_hip_prs_init(c_init, offset, ctypes.byref(st))
    if rc != _lib.OK:
        raise _lib.LdpcHipError(f"ldpc_hip_prs_init(c_init={c_init:#x}, offset={offset}) failed ({rc})")
    return state_s(int(st.x1), int(st.x2), int(c_init), int(offset))


@dataclass(frozen=True)
class state_s:
    """pseudo_random_generator::state_s: bit i of x1 / x2 is x1 / x2 (1600 + offset + i). The C ABI addresses a
    sequence by (c_init, offset), so a state also remembers where it was taken."""
    x1: int
    x2: int
    c_init: int = -1
    offset: int = 0


class pseudo_random_generator:
    """pseudo_random_generator.h:38-130 (the packed-bit and LLR forms)."""

    def init(self, c_init_or_state) -> None:
        raise NotImplementedError

    def advance(self, count: int) -> None:
        raise NotImplementedError

    def get_state(self) -> state_s:
        raise NotImplementedError


class pseudo_random_generator_hip(pseudo_random_generator):
    """The generator on the GPU: host arrays in and out, one HIP round trip per call. Every call consumes the sequence
    bits it uses, as the reference's does."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self._ctx = ctx
        self.c_init, self.offset = 0, 0

    @property
    def ctx(self) -> _lib.Context:
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def init(self, c_init_or_state) -> None:
        """init(c_init) or init(state) (a state from get_state() / prs_state())."""
        if isinstance(c_init_or_state, state_s):
            st = c_init_or_state
            if st.c_init < 0:
                raise ValueError("init(state): the state does not say which sequence (c_init, offset) it belongs to")
            self.c_init, self.offset = st.c_init, st.offset
        else:
            c_init = int(c_init_or_state)
            if not 0 <= c_init <= 0x7FFFFFFF:
                raise ValueError("c_init must fit 31 bits")
            self.c_init, self.offset = c_init, 0

    def advance(self, count: int) -> None:
        self.offset += int(count)

    def get_state(self) -> state_s:
        return prs_state(self.c_init, self.offset)

    def generate(self, nof_bits: int) -> np.ndarray:
        """generate(bit_buffer): the next nof_bits sequence bits packed MSB first (trailing bits of the last byte 0)."""
        return self._bits(None, nof_bits)

    def apply_xor(self, data: np.ndarray, nof_bits: int = -1) -> np.ndarray:
        """apply_xor: int8 data are LLRs (sign flipped where the sequence bit is 1); uint8 data are bits packed MSB
        first, nof_bits of them (default: all), the last byte's bits beyond nof_bits unchanged. Returns a new array."""
        data = np.ascontiguousarray(data)
        if data.dtype == np.int8:
            out = np.empty_like(data)
            _lib.check(self.ctx.handle,
                       self.ctx.lib.ldpc_hip_descramble_sync(self.ctx.handle, self.c_init, self.offset, data.size,
                                                             data.ctypes.data, out.ctypes.data),
                       "ldpc_hip_descramble_sync")
            self.offset += data.size
            return out
        if data.dtype != np.uint8:
            raise ValueError("apply_xor takes int8 LLRs or uint8 packed bits")
        nof_bits = data.size * 8 if nof_bits < 0 else nof_bits
        if (nof_bits + 7) // 8 != data.size:
            raise ValueError("nof_bits does not match the packed buffer")
        return self._bits(data, nof_bits)

    def _bits(self, data, nof_bits: int) -> np.ndarray:
        import torch
        nbytes = (nof_bits + 7) // 8
        if nbytes == 0:
            return np.zeros(0, np.uint8)
        dev = torch.device("cuda", self.ctx.device)
        d_in = torch.from_numpy(data).to(dev) if data is not None else None
        d_out = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        scramble_bits_launch(self.ctx, [prs_segment(nof_bits, self.c_init, self.offset)],
                             d_in.data_ptr() if d_in is not None else 0, d_out.data_ptr())
        self.offset += nof_bits
        return d_out.cpu().numpy()


class pseudo_random_generator_factory:
    """sequence_generator_factories.h create_pseudo_random_generator_sw_factory's counterpart."""

    def __init__(self, ctx: Optional[_lib.Context] = None):
        self.ctx = ctx

    def create(self) -> pseudo_random_generator:
        return pseudo_random_generator_hip(self.ctx)


def create_pseudo_random_generator_hip_factory(ctx: Optional[_lib.Context] = None) -> pseudo_random_generator_factory:
    return pseudo_random_generator_factory(ctx)


@dataclass
class prs_segment:
    """One ldpc_hip_prs_seg: `length` LLRs (or bits) against c(seq_offset ..) of c_init; offsets in bytes from the
    launch's base pointers."""
    length: int
    c_init: int
    seq_offset: int = 0
    in_offset: int = 0
    out_offset: int = 0


def prs_descriptors(segments: Sequence[prs_segment]):
    """The ldpc_hip_prs_seg array of `segments` (build once, launch many times)."""
    arr = (_lib.PrsSeg * max(len(segments), 1))()
    for i, s in enumerate(segments):
        arr[i].in_offset, arr[i].out_offset, arr[i].seq_offset = s.in_offset, s.out_offset, s.seq_offset
        arr[i].length, arr[i].c_init = s.length, s.c_init
    return arr


def scramble_descriptors(entries):
    """The ldpc_hip_scramble_desc array of `entries`: per codeblock None (not scrambled) or (c_init, seq_offset)."""
    arr = (_lib.ScrambleDesc * max(len(entries), 1))()
    for i, e in enumerate(entries):
        if e is not None:
            arr[i].c_init, arr[i].seq_offset, arr[i].enable = e[0], e[1], 1
    return arr


def _launch(name: str, ctx: _lib.Context, segments, d_in: int, d_out: int, stream: int, n: int) -> None:
    if n < 0:
        n = len(segments)
        arr = prs_descriptors(segments)
    else:
        arr = segments
    fn = getattr(_lib.load(), name)
    _lib.check(ctx.handle,
               fn(ctx.handle, n, arr, ctypes.c_void_p(d_in or None), ctypes.c_void_p(d_out),
                  ctypes.c_void_p(_lib.stream_arg(stream))), name)


def descramble_launch(ctx: _lib.Context, segments, d_in: int, d_out: int, stream: int = 0, n: int = -1) -> None:
    """ldpc_hip_descramble_launch on device pointers (asynchronous on `stream`). `segments`: a sequence of
    prs_segment, or a prebuilt prs_descriptors() array with its length n."""
    _launch("ldpc_hip_descramble_launch", ctx, segments, d_in, d_out, stream, n)


def scramble_bits_launch(ctx: _lib.Context, segments, d_in: int, d_out: int, stream: int = 0, n: int = -1) -> None:
    """ldpc_hip_scramble_bits_launch on device pointers; d_in = 0 generates the sequence."""
    _launch("ldpc_hip_scramble_bits_launch", ctx, segments, d_in, d_out, stream, n)
