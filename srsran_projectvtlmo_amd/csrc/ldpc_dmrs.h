/*
 * The PDSCH DM-RS generator's work item and host launcher (downlink, beside the precoder in the resource grid), shared
 * by its kernel unit (ldpc_dmrs_kernels.hip), its translation (ldpc_hip_descs.cpp) and its host unit
 * (ldpc_hip_dmrs.cpp). Nothing of the decoder, the uplink family, the mapper, the equalizer or the precoder is declared
 * here.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_hip {

/* A thread owns DMRS_RBS consecutive resource blocks of its row, for every CDM group and port: 2 DMRS_RBS dpr
 * consecutive sequence bits (12 for type 1, 8 for type 2), which with their offset inside a 32-bit sequence word
 * (at most 31) lie in two consecutive words (DMRS_RBS <= 2 keeps that so). Blocks [block0, block0 + ceil((rb_end -
 * rb_begin) / (DMRS_BLOCK DMRS_RBS))) of the launch work on the row's resource blocks [rb_begin, rb_end), its lowest to
 * its highest set one. One wave per block, as the precoder: a 273-RB row is 5 blocks. One RB per thread, not two: a
 * thread's time is its RBs' 12 REs each on up to four ports, 48 precoded stores per RB, and two RBs per thread were
 * measured slower. */
constexpr int      DMRS_BLOCK      = 64;
constexpr int      DMRS_RBS        = 1;
static_assert(DMRS_RBS * 12 + 31 <= 64, "a thread's sequence bits lie in two words");
constexpr uint32_t DMRS_MAX_PORTS  = 4;
constexpr uint32_t DMRS_MAX_LAYERS = 4;
constexpr uint32_t DMRS_NSYMB      = 14; /* OFDM symbols of a slot (normal cyclic prefix) */

/* One row: one transmission on one DM-RS symbol. Resource block n of the row (its bit n % 64 of mask word word0 +
 * n / 64 set) takes the sequence bits 2 dpr (n - ref_rb) .. + 2 dpr - 1 from the state (x1, x2), dpr = 6 (type 1) or 4
 * (type 2) pilots per RB and CDM group; pilot j of CDM group g lies on subcarrier k = 12 n + (type 1: 2 j + g; type 2:
 * 2 g + j for j < 2, 4 + 2 g + j else), and port p of it goes to element out_offset + p out_stride + k of the output
 * (cbf16, 4 bytes, or cf32, 8 bytes). */
struct dmrs_row {
  uint64_t out_offset, out_stride;
  uint32_t x1, x2;   /* the generator's state at sequence bit 0 of the symbol (prs_state_at(c_init, 0))   */
  float    a;        /* (float)(M_SQRT1_2 * (double)amplitude)                                            */
  uint32_t word0;    /* the row's first RB-mask word (64 bits) in the launch's table                      */
  uint32_t weight0;  /* the transmission's weights [port][layer], in cf32 elements of the launch's table  */
  uint32_t rb_begin, rb_end;
  uint32_t ref_rb;   /* reference_point_k_rb, at most rb_begin                                            */
  uint32_t block0;
  uint8_t  type, nof_layers, nof_ports;
  uint8_t  bypass;   /* one layer on one port with the weight 1 + 0j: the pilots are stored unmultiplied   */
  uint32_t pad;
};
static_assert(sizeof(dmrs_row) == 64, "DM-RS work item layout");

/* DM-RS types 1 and 2 at every 1 <= layers <= ports <= 4: DM-RS ports 0 to 3, two CDM groups, w_t = +1 */
constexpr bool dmrs_supported(uint32_t type, uint32_t layers, uint32_t ports)
{
  return (type == 1 || type == 2) && layers >= 1 && layers <= ports && ports <= DMRS_MAX_PORTS;
}

/* ldpc_dmrs_kernels.hip; nblocks as the rows' block0 count them. cf32: the output's elements are (float re, float im),
 * the values before the bf16 rounding, at the same element offsets and strides. */
hipError_t launch_dmrs(const dmrs_row* d_rows, uint32_t nrows, uint32_t nblocks, const uint64_t* d_words,
                       const float* d_weights, void* d_out, bool cf32, hipStream_t stream);

} // namespace ldpc_hip
