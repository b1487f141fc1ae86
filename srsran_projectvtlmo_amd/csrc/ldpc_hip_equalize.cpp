/*
 * The channel equalizer's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_equalize_supported,
 * ldpc_hip_equalize_launch and ldpc_hip_equalize_sync. The descriptors become work items in ldpc_hip_descs.cpp
 * (validation and the block count); the kernel is ldpc_equalize_kernels.hip's.
 */
#include <vector>

#include "ldpc_hip_ctx.h"

using namespace ldpc_hip;

namespace {

int equalize_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_eq_desc* descs, const uint16_t* d_sym,
                      const uint16_t* d_est, float* d_eq, float* d_nv, hipStream_t s)
{
  std::vector<eq_seg> sg;
  uint32_t            blocks = 0;
  if (const char* why = make_segs(nof_segs, descs, sg, blocks, make_eq_seg)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  return ctx->launch_items(ctx->d_eqsegs, sg, s, "ldpc_equalize_kernel launch", [&](const eq_seg* d_segs) {
    return launch_equalize(d_segs, static_cast<uint32_t>(sg.size()), blocks, d_sym, d_est, d_eq, d_nv, s);
  });
}

} // namespace

extern "C" {

int ldpc_hip_equalize_supported(int algorithm, uint32_t nof_rx_ports, uint32_t nof_tx_layers)
{
  return eq_supported(algorithm, nof_rx_ports, nof_tx_layers) ? 1 : 0;
}

int ldpc_hip_equalize_launch(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_eq_desc* descs,
                             const uint16_t* d_ch_symbols, const uint16_t* d_ch_estimates, float* d_eq_symbols,
                             float* d_eq_noise_vars, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_segs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_ch_symbols == nullptr || d_ch_estimates == nullptr || d_eq_symbols == nullptr ||
      d_eq_noise_vars == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "equalize_launch: null argument");
  }
  (void)hipSetDevice(ctx->device);
  return equalize_segments(ctx, nof_segs, descs, d_ch_symbols, d_ch_estimates, d_eq_symbols, d_eq_noise_vars,
                           abi_stream(ctx->stream, stream));
}

int ldpc_hip_equalize_sync(ldpc_hip_ctx* ctx, int algorithm, uint32_t nof_re, uint32_t nof_rx_ports,
                           uint32_t nof_tx_layers, const uint16_t* ch_symbols, const uint16_t* ch_estimates,
                           const float* noise_vars, float tx_scaling, float* eq_symbols, float* eq_noise_vars)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  ldpc_hip_eq_desc d{};
  d.sym_stride = d.est_stride = d.nof_re = nof_re;
  d.tx_scaling                           = tx_scaling;
  uint64_t blocks = 0;
  eq_seg   g;
  if (eq_supported(algorithm, nof_rx_ports, nof_tx_layers)) {
    d.algorithm     = static_cast<uint8_t>(algorithm);
    d.nof_rx_ports  = static_cast<uint8_t>(nof_rx_ports);
    d.nof_tx_layers = static_cast<uint8_t>(nof_tx_layers);
  } else {
    d.algorithm = 0xffU; /* refused below with the launch's message */
  }
  if (const char* why = make_eq_seg(d, blocks, g)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  if (nof_re == 0) {
    return LDPC_HIP_OK;
  }
  if (ch_symbols == nullptr || ch_estimates == nullptr || noise_vars == nullptr || eq_symbols == nullptr ||
      eq_noise_vars == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "equalize_sync: null argument");
  }
  for (uint32_t p = 0; p != nof_rx_ports; ++p) {
    d.noise_var[p] = noise_vars[p];
  }
  (void)hipSetDevice(ctx->device);
  const size_t nsym = static_cast<size_t>(nof_re) * nof_rx_ports * 4U;
  const size_t nest = nsym * nof_tx_layers;
  const size_t nout = static_cast<size_t>(nof_re) * nof_tx_layers;
  /* d_llr: received REs then estimates (nsym is a multiple of 4 bytes, so the estimates stay element-aligned) */
  return ctx->sync_round_trip(
      "equalize",
      {to_device(ctx->d_llr, 0, ch_symbols, nsym), to_device(ctx->d_llr, nsym, ch_estimates, nest),
       to_host(ctx->d_sym, 0, eq_symbols, nout * 8U), to_host(ctx->d_nv, 0, eq_noise_vars, nout * 4U)},
      [&] {
        const uint8_t* in = ctx->d_llr.as<uint8_t>();
        return equalize_segments(ctx, 1, &d, reinterpret_cast<const uint16_t*>(in),
                                 reinterpret_cast<const uint16_t*>(in + nsym), ctx->d_sym.as<float>(),
                                 ctx->d_nv.as<float>(), ctx->stream);
      });
}

} /* extern "C" */
