/*
 * The PDSCH DM-RS generator's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_dmrs_pdsch_supported,
 * ldpc_hip_dmrs_pdsch_c_init and ldpc_hip_dmrs_pdsch_map_launch. The transmissions, their RB masks and their weights
 * become the one table the kernel reads in ldpc_hip_descs.cpp (make_dmrs_table); the kernel is
 * ldpc_dmrs_kernels.hip's.
 */
#include "ldpc_hip_ctx.h"

using namespace ldpc_hip;

extern "C" {

int ldpc_hip_dmrs_pdsch_supported(uint32_t type, uint32_t nof_layers, uint32_t nof_ports)
{
  return dmrs_supported(type, nof_layers, nof_ports) ? 1 : 0;
}

uint32_t ldpc_hip_dmrs_pdsch_c_init(uint32_t slot_index, uint32_t symbol, uint32_t scrambling_id, uint32_t n_scid)
{
  return dmrs_c_init(slot_index, symbol, scrambling_id, n_scid);
}

int ldpc_hip_dmrs_pdsch_map_launch(ldpc_hip_ctx* ctx, uint32_t nof_descs, const ldpc_hip_dmrs_pdsch_desc* descs,
                                   const float* weights, uint32_t nof_weights, const uint64_t* rb_masks,
                                   uint32_t nof_mask_words, void* d_grid, int output_format, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (output_format != LDPC_HIP_SYM_CBF16 && output_format != LDPC_HIP_SYM_CF32) {
    return ctx->fail(LDPC_HIP_EINVAL,
                     "dmrs_pdsch_map_launch: output_format is LDPC_HIP_SYM_CBF16 or LDPC_HIP_SYM_CF32");
  }
  if (nof_descs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || weights == nullptr || rb_masks == nullptr || d_grid == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "dmrs_pdsch_map_launch: null argument");
  }
  dmrs_table t;
  if (const char* why = make_dmrs_table(nof_descs, descs, weights, nof_weights, rb_masks, nof_mask_words, t)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  (void)hipSetDevice(ctx->device);
  const hipStream_t s = abi_stream(ctx->stream, stream);
  /* the table's blob into d_dmrs, then the launch on its rows, words and weights there */
  return ctx->launch_items(ctx->d_dmrs, t.blob, s, "ldpc_dmrs_kernel launch", [&](const uint8_t* base) {
    return launch_dmrs(reinterpret_cast<const dmrs_row*>(base), static_cast<uint32_t>(t.rows.size()), t.nblocks,
                       reinterpret_cast<const uint64_t*>(base + t.words_at),
                       reinterpret_cast<const float*>(base + t.weights_at), d_grid,
                       output_format == LDPC_HIP_SYM_CF32, s);
  });
}

} /* extern "C" */
