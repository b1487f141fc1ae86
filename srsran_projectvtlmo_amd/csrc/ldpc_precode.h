/*
 * The precoder's work item and host launcher (downlink, behind the modulation mapper), shared by its kernel unit
 * (ldpc_precode_kernels.hip), its translation (ldpc_hip_descs.cpp) and its host unit (ldpc_hip_precode.cpp). Nothing
 * of the decoder, the uplink family, the mapper or the equalizer is declared here.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_hip {

/* A thread owns PC_RES consecutive subcarriers of its row (all ports of them): one nibble of the row's mask, which a
 * 64-bit mask word never splits, and one PRG, since a PRG is a multiple of 12 subcarriers. Blocks [block0, block0 +
 * ceil((k_end - k_begin) / (PC_BLOCK * PC_RES))) of the launch work on the row's subcarriers [k_begin, k_end): the
 * mask words that have a bit set, so a one-PRB row high in a wide grid is one block. One wave per block, as the
 * equalizer: a 3276-subcarrier row is 13 blocks. */
constexpr int      PC_BLOCK      = 64;
constexpr int      PC_RES        = 4;
constexpr uint32_t PC_MAX_PORTS  = 4;
constexpr uint32_t PC_MAX_LAYERS = 4;

/* one 64-bit word of a row's mask (bit k % 64 of word k / 64) with the set bits of the row's earlier words */
struct precode_word {
  uint64_t bits;
  uint32_t prefix;
  uint32_t pad;
};
static_assert(sizeof(precode_word) == 16, "one 16-byte load");

/* One row: one transmission on one OFDM symbol (or, compact, one PRG of a channel_precoder call). The r-th masked
 * subcarrier reads layer i at
 *   ci8 in:   in + 2 (in_offset + L r + i) bytes                (int8 re, im)
 *   cf32 in:  in + 8 (in_offset + i in_stride + r) bytes         (float re, im; layer planes)
 * and port p of it goes to
 *   grid out:    out + 4 (out_offset + p out_stride + k) bytes  (cbf16; k the subcarrier)
 *   compact out: out + 8 (out_offset + p out_stride + r) bytes  (float re, im; port planes). */
struct precode_row {
  uint64_t in_offset, in_stride;
  uint64_t out_offset, out_stride;
  uint32_t word0;    /* the row's first precode_word in the launch's table                         */
  uint32_t weight0;  /* the row's weights [prg][port][layer], in cf32 elements of the launch's table */
  uint32_t k_begin, k_end;
  uint32_t prg_subc; /* subcarriers per PRG, counted from subcarrier 0                              */
  uint32_t block0;
  uint8_t  nof_layers, nof_ports, pad[6];
};
static_assert(sizeof(precode_row) == 64, "precoder work item layout");

/* every 1 <= layers <= ports <= 4 (precoding_constants::MAX_NOF_LAYERS / MAX_NOF_PORTS) */
constexpr bool precode_supported(uint32_t layers, uint32_t ports)
{
  return layers >= 1 && layers <= ports && ports <= PC_MAX_PORTS;
}

/* ldpc_precode_kernels.hip; nblocks as the rows' block0 count them. in_cf32: the input's form; compact: the output's.
 * (cf32 in, grid out) has no entry point and no instance. */
hipError_t launch_precode(const precode_row* d_rows, uint32_t nrows, uint32_t nblocks, const precode_word* d_words,
                          const float* d_weights, const void* d_in, void* d_out, bool in_cf32, bool compact,
                          hipStream_t stream);

} // namespace ldpc_hip
