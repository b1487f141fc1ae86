/*
 * The PUSCH DM-RS channel estimator's entry points of the C ABI (include/srsran_ldpc_hip.h):
 * ldpc_hip_dmrs_pusch_supported, ldpc_hip_dmrs_pusch_estimate_launch and ldpc_hip_dmrs_pusch_finalize. The
 * transmissions and their RB masks become the one table the kernel reads in ldpc_hip_descs.cpp (make_chest_table),
 * where the finals of the raw sums are computed too (chest_finalize); the kernel is ldpc_chest_kernels.hip's.
 */
#include "ldpc_hip_ctx.h"

using namespace ldpc_hip;

extern "C" {

int ldpc_hip_dmrs_pusch_supported(uint32_t type, uint32_t nof_layers, uint32_t nof_rx_ports, uint32_t strategy,
                                  uint32_t compensate_cfo)
{
  return chest_supported(type, nof_layers, nof_rx_ports, strategy, compensate_cfo) ? 1 : 0;
}

int ldpc_hip_dmrs_pusch_estimate_launch(ldpc_hip_ctx* ctx, uint32_t nof_descs, const ldpc_hip_dmrs_pusch_desc* descs,
                                        const uint64_t* rb_masks, uint32_t nof_mask_words, const void* d_grid,
                                        void* d_estimates, int output_format, void* d_filtered_pilots,
                                        void* d_results, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (output_format != LDPC_HIP_SYM_CBF16 && output_format != LDPC_HIP_SYM_CF32) {
    return ctx->fail(LDPC_HIP_EINVAL,
                     "dmrs_pusch_estimate_launch: output_format is LDPC_HIP_SYM_CBF16 or LDPC_HIP_SYM_CF32");
  }
  if (nof_descs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || rb_masks == nullptr || d_grid == nullptr || d_estimates == nullptr || d_results == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "dmrs_pusch_estimate_launch: null argument");
  }
  chest_table t;
  if (const char* why = make_chest_table(nof_descs, descs, rb_masks, nof_mask_words, t)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  (void)hipSetDevice(ctx->device);
  const hipStream_t s = abi_stream(ctx->stream, stream);
  /* the table's blob into d_chest, then the launch on its planes, words and filters there */
  return ctx->launch_items(ctx->d_chest, t.blob, s, "ldpc_chest_kernel launch", [&](const uint8_t* base) {
    return launch_chest(reinterpret_cast<const chest_plane*>(base), static_cast<uint32_t>(t.planes.size()),
                        reinterpret_cast<const uint64_t*>(base + t.words_at),
                        reinterpret_cast<const float*>(base + t.filters_at), d_grid, d_estimates,
                        output_format == LDPC_HIP_SYM_CF32, d_filtered_pilots, d_results, s);
  });
}

int ldpc_hip_dmrs_pusch_finalize(const ldpc_hip_chest_result* sums, float scaling, uint32_t nof_dmrs_symbols,
                                 uint32_t l0, uint32_t l1, uint32_t scs, ldpc_hip_chest_metrics* out)
{
  if (sums == nullptr || out == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  return chest_finalize(*sums, scaling, nof_dmrs_symbols, l0, l1, scs, *out) == nullptr ? LDPC_HIP_OK
                                                                                         : LDPC_HIP_EINVAL;
}

} /* extern "C" */
