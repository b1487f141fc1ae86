/*
 * The PUSCH DM-RS channel estimator's work item and host launcher (uplink, ahead of the equalizer), shared by its
 * kernel unit (ldpc_chest_kernels.hip), its translation (ldpc_hip_descs.cpp) and its host unit (ldpc_hip_chest.cpp).
 * Nothing of the decoder, the uplink family, the mapper, the equalizer, the precoder or the PDSCH DM-RS generator is
 * declared here.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_hip {

/* One workgroup per (transmission, rx port, layer) plane; its pilot vectors stay in LDS (ldpc_chest_kernels.hip). */
constexpr int      CHEST_BLOCK       = 256;
constexpr uint32_t CHEST_MAX_RB      = 275; /* MAX_RB: the widest RB mask; every RB of it may be allocated        */
constexpr uint32_t CHEST_MAX_PORTS   = 4;
constexpr uint32_t CHEST_MAX_LAYERS  = 4;
constexpr uint32_t CHEST_MAX_DMRS    = 4;   /* DM-RS symbols of a transmission                                    */
constexpr uint32_t CHEST_NSYMB       = 14;  /* OFDM symbols of a slot (normal cyclic prefix)                      */
constexpr uint32_t CHEST_DPR         = 6;   /* type 1: pilots per RB and layer                                    */
constexpr uint32_t CHEST_MAX_VPILOTS = 12;  /* port_channel_estimator_average_impl::MAX_V_PILOTS                  */
constexpr uint32_t CHEST_MAX_TAPS    = 15;  /* the filter of 3 or more RBs at stride 2                            */
constexpr uint32_t CHEST_TAP_STRIDE  = 16;  /* floats per filter in the launch's table                            */
constexpr uint32_t CHEST_NOF_FILTERS = 3;   /* 1 RB (5 taps), 2 RBs (11), 3 or more (15)                          */
constexpr uint8_t  CHEST_NO_FILTER   = 0xff;

/* One plane. Allocated RB n (bit n % 64 of mask word word0 + n / 64 set; rb_begin the lowest, rb_end one past the
 * highest, n_rb of them) has pilot j of layer `layer` on subcarrier k = 12 n + 2 j + layer / 2; DM-RS symbol s
 * (0 <= s < nsym) is OFDM symbol dmrs_sym[s] and reads the received element grid_base + dmrs_sym[s] grid_sym_stride +
 * k; its sequence bits 12 (n - rb_begin) .. + 11 come from the state (x1[s], x2[s]). The estimates go to elements
 * est_base + l est_sym_stride + 12 n + (0 .. 11) for first_symbol <= l < first_symbol + nof_symbols, the filtered
 * pilots to cf32 elements pil_base + (0 .. 6 n_rb - 1), the sums to record res_index. */
struct chest_plane {
  uint64_t grid_base, grid_sym_stride;
  uint64_t est_base, est_sym_stride;
  uint64_t pil_base;
  uint32_t res_index;
  uint32_t word0;
  uint32_t rb_begin, rb_end, n_rb;
  uint32_t x1[CHEST_MAX_DMRS], x2[CHEST_MAX_DMRS]; /* the generator's state at sequence bit 12 rb_begin of symbol s */
  float    total_scaling;  /* 1.0F / ((float)nsym * scaling)                                                      */
  float    beta;           /* scaling                                                                             */
  uint8_t  dmrs_sym[CHEST_MAX_DMRS];
  uint8_t  nsym, layer, first_symbol, nof_symbols;
  uint8_t  filter;         /* row of the launch's filter table, or CHEST_NO_FILTER: smoothing `none`              */
  uint8_t  ntaps, nvp;     /* the filter's taps and the virtual pilots per side                                   */
  uint8_t  wide;           /* est_base and est_sym_stride are multiples of 4 elements: 16-byte stores             */
  uint32_t block0;
  uint32_t pad;
};
static_assert(sizeof(chest_plane) == 120, "channel estimator work item layout");

/* ldpc_hip_chest_result (include/srsran_ldpc_hip.h) as the kernel writes it */
struct chest_record {
  float    epre_sum, filt_power, noise_sum, dot_re, dot_im;
  uint32_t nof_pilots;
  uint32_t pad[2];
};
static_assert(sizeof(chest_record) == 32, "channel estimator result record layout");

/* DM-RS type 1, DM-RS ports 0 to 3 (w_t = +1) on 1 to 4 receive ports; smoothing none (0) or filter (1), no CFO
 * compensation */
constexpr bool chest_supported(uint32_t type, uint32_t layers, uint32_t ports, uint32_t strategy, uint32_t comp_cfo)
{
  return type == 1 && layers >= 1 && layers <= CHEST_MAX_LAYERS && ports >= 1 && ports <= CHEST_MAX_PORTS &&
         strategy <= 1 && comp_cfo == 0;
}

/* ldpc_chest_kernels.hip; one block per plane. cf32: the estimates' elements are (float re, float im), the values
 * before the bf16 rounding, at the same element offsets and strides. d_pilots may be null. */
hipError_t launch_chest(const chest_plane* d_planes, uint32_t nplanes, const uint64_t* d_words, const float* d_filters,
                        const void* d_grid, void* d_est, bool cf32, void* d_pilots, void* d_results,
                        hipStream_t stream);

} // namespace ldpc_hip
