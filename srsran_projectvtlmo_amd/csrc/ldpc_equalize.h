/*
 * The channel equalizer's work item and host launcher, shared by its kernel unit (ldpc_equalize_kernels.hip) and its
 * host unit (ldpc_hip_equalize.cpp). Nothing of the decoder, the uplink family or the mapper is declared here.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_hip {

/* A thread owns EQ_RES consecutive REs of its segment (whole REs: every port and layer of them), so a plane's four
 * cbf16 elements are one 16-byte load; blocks [block0, block0 + ceil(nof_re / (EQ_BLOCK * EQ_RES))) of the launch work
 * on the segment. One wave per block: C4's 42,588 REs are 167 blocks, one per CU and more, where 256 threads would
 * leave 42 blocks on 256 CUs. */
constexpr int      EQ_BLOCK     = 64;
constexpr int      EQ_RES       = 4;
constexpr uint32_t EQ_MAX_PORTS = 4;

/* offsets and strides in cbf16 elements (4 bytes) as ldpc_hip_eq_desc gives them; out_offset in symbols / floats */
struct eq_seg {
  uint64_t sym_offset, sym_stride;
  uint64_t est_offset, est_stride;
  uint64_t out_offset;
  uint32_t nof_re;
  uint32_t block0;
  float    tx_scaling;
  float    noise_var[EQ_MAX_PORTS];
  uint8_t  algorithm, nof_rx_ports, nof_tx_layers, pad;
};
static_assert(sizeof(eq_seg) == 72, "equalizer work item layout");

/* channel_equalizer_generic_impl.cpp:184-214 within the PUSCH processor's four ports: ZF and MMSE with one layer on one
 * to four ports, ZF with two layers on two or four ports */
constexpr bool eq_supported(int algorithm, uint32_t ports, uint32_t layers)
{
  return (algorithm == 0 || algorithm == 1) &&
         ((layers == 1 && ports >= 1 && ports <= EQ_MAX_PORTS) ||
          (algorithm == 0 && layers == 2 && (ports == 2 || ports == 4)));
}

/* ldpc_equalize_kernels.hip; nblocks as the segments' block0 count them */
hipError_t launch_equalize(const eq_seg* d_segs, uint32_t nseg, uint32_t nblocks, const uint16_t* d_ch_symbols,
                           const uint16_t* d_ch_estimates, float* d_eq_symbols, float* d_eq_noise_vars,
                           hipStream_t stream);

} // namespace ldpc_hip
