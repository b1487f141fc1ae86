/*
 * The precoder's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_precode_supported,
 * ldpc_hip_precode_map_launch and ldpc_hip_precode_sync. The rows, their masks and their weights become the one table
 * the kernel reads in ldpc_hip_descs.cpp (make_precode_table); the kernel is ldpc_precode_kernels.hip's.
 */
#include <vector>

#include "ldpc_hip_ctx.h"

using namespace ldpc_hip;

namespace {

/* the table's blob into d_precode, then the launch on its rows, words and weights there */
int precode_rows(ldpc_hip_ctx* ctx, const precode_table& t, const void* d_in, void* d_out, bool in_cf32, bool compact,
                 hipStream_t s)
{
  return ctx->launch_items(ctx->d_precode, t.blob, s, "ldpc_precode_kernel launch", [&](const uint8_t* base) {
    return launch_precode(reinterpret_cast<const precode_row*>(base), static_cast<uint32_t>(t.rows.size()), t.nblocks,
                          reinterpret_cast<const precode_word*>(base + t.words_at),
                          reinterpret_cast<const float*>(base + t.weights_at), d_in, d_out, in_cf32, compact, s);
  });
}

} // namespace

extern "C" {

int ldpc_hip_precode_supported(uint32_t nof_layers, uint32_t nof_ports)
{
  return precode_supported(nof_layers, nof_ports) ? 1 : 0;
}

int ldpc_hip_precode_map_launch(ldpc_hip_ctx* ctx, uint32_t nof_rows, const ldpc_hip_precode_desc* descs,
                                const float* weights, uint32_t nof_weights, const uint64_t* masks,
                                uint32_t nof_mask_words, const void* d_symbols, void* d_grid, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_rows == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || weights == nullptr || masks == nullptr || d_symbols == nullptr || d_grid == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode_map_launch: null argument");
  }
  precode_table t;
  if (const char* why =
          make_precode_table(nof_rows, descs, weights, nof_weights, masks, nof_mask_words, false, 0, t)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  (void)hipSetDevice(ctx->device);
  return precode_rows(ctx, t, d_symbols, d_grid, false, false, abi_stream(ctx->stream, stream));
}

int ldpc_hip_precode_sync(ldpc_hip_ctx* ctx, uint32_t nof_re, uint32_t nof_layers, uint32_t nof_ports,
                          const void* input, int input_format, const float* weights, float* output)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (!precode_supported(nof_layers, nof_ports)) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode: unsupported topology (1 <= layers <= ports <= 4)");
  }
  if (input_format != LDPC_HIP_SYM_CF32 && input_format != LDPC_HIP_SYM_CI8) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode_sync: input_format is LDPC_HIP_SYM_CF32 or LDPC_HIP_SYM_CI8");
  }
  if (static_cast<uint64_t>(nof_re) * nof_layers >= (1ULL << 31)) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode_sync: nof_re * nof_layers must be below 2^31");
  }
  if (weights == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode_sync: null argument");
  }
  /* one PRG, every RE masked */
  std::vector<uint64_t> mask((nof_re + 63U) / 64U, ~0ULL);
  if (nof_re % 64U != 0) {
    mask.back() = (1ULL << (nof_re % 64U)) - 1ULL;
  }
  const bool            cf32 = input_format == LDPC_HIP_SYM_CF32;
  ldpc_hip_precode_desc d{};
  d.port_stride = nof_re;
  d.nof_prg     = 1;
  d.width       = nof_re;
  d.prg_size    = 1; /* unused: a compact row is one PRG */
  d.nof_layers  = static_cast<uint8_t>(nof_layers);
  d.nof_ports   = static_cast<uint8_t>(nof_ports);
  precode_table t;
  if (const char* why = make_precode_table(1, &d, weights, nof_layers * nof_ports, mask.data(),
                                           static_cast<uint32_t>(mask.size()), true, nof_re, t)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  if (nof_re == 0) {
    return LDPC_HIP_OK;
  }
  if (input == nullptr || output == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "precode_sync: null argument");
  }
  (void)hipSetDevice(ctx->device);
  const size_t nin  = static_cast<size_t>(nof_re) * nof_layers * (cf32 ? 8U : 2U);
  const size_t nout = static_cast<size_t>(nof_re) * nof_ports * 8U;
  return ctx->sync_round_trip("precode", {to_device(ctx->d_llr, 0, input, nin), to_host(ctx->d_sym, 0, output, nout)},
                              [&] {
                                return precode_rows(ctx, t, ctx->d_llr.ptr, ctx->d_sym.ptr, cf32, true, ctx->stream);
                              });
}

} /* extern "C" */
