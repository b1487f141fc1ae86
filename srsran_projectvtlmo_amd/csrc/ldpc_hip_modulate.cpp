/*
 * The modulation mapper's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_modulation_scaling,
 * ldpc_hip_modulate_launch / _sync and ldpc_hip_rate_match_modulate_launch. The descriptors become work items in
 * ldpc_hip_descs.cpp (validation, one generator start state per scrambled segment, the block count); the kernels are
 * ldpc_modulation_kernels.hip's.
 */
#include <cstring>
#include <vector>

#include "ldpc_hip_ctx.h"
#include "ldpc_hip_launch.h"

using namespace ldpc_hip;

namespace {

bool valid_format(int format) { return format == LDPC_HIP_SYM_CF32 || format == LDPC_HIP_SYM_CI8; }

int modulate_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_mod_desc* descs, const uint8_t* d_bits,
                      void* d_symbols, int format, hipStream_t s)
{
  std::vector<mod_seg> sg;
  uint32_t             blocks = 0;
  if (const char* why = make_segs(nof_segs, descs, sg, blocks, make_mod_seg)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  return ctx->launch_items(ctx->d_modsegs, sg, s, "ldpc_modulate_kernel launch", [&](const mod_seg* d_segs) {
    return launch_modulate(d_segs, static_cast<uint32_t>(sg.size()), blocks, format == LDPC_HIP_SYM_CI8, d_bits,
                           d_symbols, s);
  });
}

} // namespace

extern "C" {

float ldpc_hip_modulation_scaling(int modulation)
{
  const uint32_t bits = mod_scaling_bits(modulation);
  float          f;
  std::memcpy(&f, &bits, sizeof(f));
  return f;
}

int ldpc_hip_modulate_launch(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_mod_desc* descs,
                             const uint8_t* d_bits, void* d_symbols, int format, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (!valid_format(format)) {
    return ctx->fail(LDPC_HIP_EINVAL, "modulate_launch: invalid symbol format");
  }
  if (nof_segs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_bits == nullptr || d_symbols == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "modulate_launch: null argument");
  }
  (void)hipSetDevice(ctx->device);
  return modulate_segments(ctx, nof_segs, descs, d_bits, d_symbols, format, abi_stream(ctx->stream, stream));
}

int ldpc_hip_modulate_sync(ldpc_hip_ctx* ctx, uint32_t nof_symbols, int modulation, const uint8_t* bits, void* symbols,
                           int format)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (!valid_modulation(modulation)) {
    return ctx->fail(LDPC_HIP_EINVAL, "modulate: invalid modulation scheme");
  }
  if (!valid_format(format)) {
    return ctx->fail(LDPC_HIP_EINVAL, "modulate_sync: invalid symbol format");
  }
  if (nof_symbols == 0) {
    return LDPC_HIP_OK;
  }
  if (bits == nullptr || symbols == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "modulate_sync: null argument");
  }
  (void)hipSetDevice(ctx->device);
  const size_t nin  = (static_cast<size_t>(nof_symbols) * bits_per_symbol(modulation) + 7U) / 8U;
  const size_t nout = static_cast<size_t>(nof_symbols) * (format == LDPC_HIP_SYM_CI8 ? 2U : 8U);
  ldpc_hip_mod_desc d{};
  d.nof_symbols = nof_symbols;
  d.modulation  = static_cast<uint8_t>(modulation);
  return ctx->sync_round_trip("modulate", {to_device(ctx->d_llr, 0, bits, nin), to_host(ctx->d_sym, 0, symbols, nout)},
                              [&] {
                                return modulate_segments(ctx, 1, &d, ctx->d_llr.as<uint8_t>(), ctx->d_sym.ptr, format,
                                                         ctx->stream);
                              });
}

int ldpc_hip_rate_match_modulate_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_rm_desc* descs,
                                        const ldpc_hip_mod_desc* mod, const uint8_t* d_cws, void* d_symbols,
                                        int format, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (!valid_format(format)) {
    return ctx->fail(LDPC_HIP_EINVAL, "rate_match_modulate_launch: invalid symbol format");
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || mod == nullptr || d_cws == nullptr || d_symbols == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "rate_match_modulate_launch: null argument");
  }
  std::vector<rm_mod_cb> cbs(nof_cbs);
  uint64_t               blocks = 0;
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    if (const char* why = make_rm_mod_cb(descs[i], mod[i], blocks, cbs[i])) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  return ctx->launch_items(ctx->d_rmmod, cbs, s, "ldpc_rate_match_modulate_kernel launch",
                           [&](const rm_mod_cb* d_cbs) {
                             return launch_rate_match_modulate(d_cbs, nof_cbs, static_cast<uint32_t>(blocks),
                                                               format == LDPC_HIP_SYM_CI8, d_cws, d_symbols, s);
                           });
}

} /* extern "C" */
