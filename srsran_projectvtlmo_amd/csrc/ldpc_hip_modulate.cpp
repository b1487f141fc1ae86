/*
 * The modulation mapper's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_modulation_scaling,
 * ldpc_hip_modulate_launch / _sync and ldpc_hip_rate_match_modulate_launch. The host validates the descriptors,
 * computes one generator start state per scrambled segment (prs_state_at) and counts the blocks; the kernels are
 * ldpc_modulation_kernels.hip's.
 */
#include <cstring>
#include <vector>

#include "ldpc_hip_ctx.h"
#include "ldpc_hip_descs.h"
#include "ldpc_hip_launch.h"

using namespace ldpc_hip;

namespace {

constexpr uint64_t MAX_BLOCKS = 0x7fffffffULL;

/* the mapper's part of a work item; why != nullptr: refused */
const char* make_mod_seg(const ldpc_hip_mod_desc& d, uint64_t& blocks, mod_seg& g)
{
  if (!valid_modulation(d.modulation)) {
    return "modulate: invalid modulation scheme";
  }
  if (d.scramble != 0 && (d.c_init & ~PRS_MASK) != 0U) {
    return "modulate: c_init above 31 bits";
  }
  if (d.nof_symbols >= 0x80000000U) {
    /* a thread's first symbol (chunk x symbols per chunk) is 32-bit in the kernels, the last block's surplus threads
     * included */
    return "modulate: a segment holds fewer than 2^31 symbols";
  }
  const uint32_t qm = bits_per_symbol(d.modulation);
  g                 = mod_seg{};
  g.bit_offset      = d.bit_offset;
  g.sym_offset      = d.symbol_offset;
  g.nof_symbols     = d.nof_symbols;
  g.block0          = static_cast<uint32_t>(blocks);
  g.modulation      = d.modulation;
  if (d.scramble != 0) {
    const ldpc_hip_prs_state st = prs_state_at(d.c_init, d.seq_offset);
    g.x1                        = st.x1;
    g.x2                        = st.x2;
  }
  const uint64_t per_chunk = mod_chunk_bits(qm) / qm;
  const uint64_t chunks    = (d.nof_symbols + per_chunk - 1U) / per_chunk;
  blocks += (chunks + MOD_BLOCK - 1U) / MOD_BLOCK;
  return blocks > MAX_BLOCKS ? "modulate: too many symbols for one launch" : nullptr;
}

bool valid_format(int format) { return format == LDPC_HIP_SYM_CF32 || format == LDPC_HIP_SYM_CI8; }

int modulate_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_mod_desc* descs, const uint8_t* d_bits,
                      void* d_symbols, int format, hipStream_t s)
{
  std::vector<mod_seg> sg;
  sg.reserve(nof_segs);
  uint64_t blocks = 0;
  for (uint32_t i = 0; i != nof_segs; ++i) {
    mod_seg        g;
    const uint64_t before = blocks;
    if (const char* why = make_mod_seg(descs[i], blocks, g)) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
    if (blocks != before) {
      sg.push_back(g);
    }
  }
  if (sg.empty()) {
    return LDPC_HIP_OK;
  }
  hipError_t e = upload_descs(ctx->d_modsegs, ctx->c_modsegs, sg.data(), sg.size() * sizeof(mod_seg), s);
  if (e == hipSuccess) {
    e = launch_modulate(ctx->d_modsegs.as<mod_seg>(), static_cast<uint32_t>(sg.size()), static_cast<uint32_t>(blocks),
                        format == LDPC_HIP_SYM_CI8, d_bits, d_symbols, s);
  }
  return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "ldpc_modulate_kernel launch");
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
  hipError_t   e;
  if ((e = ctx->d_llr.reserve(nin)) != hipSuccess || (e = ctx->d_sym.reserve(nout)) != hipSuccess) {
    return ctx->hip_fail(e, "hipMalloc(modulate)");
  }
  if ((e = hipMemcpyAsync(ctx->d_llr.ptr, bits, nin, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "hipMemcpyAsync(modulate in)");
  }
  ldpc_hip_mod_desc d{};
  d.nof_symbols = nof_symbols;
  d.modulation  = static_cast<uint8_t>(modulation);
  const int r   = modulate_segments(ctx, 1, &d, ctx->d_llr.as<uint8_t>(), ctx->d_sym.ptr, format, ctx->stream);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  if ((e = hipMemcpyAsync(symbols, ctx->d_sym.ptr, nout, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "modulate_sync");
  }
  return LDPC_HIP_OK;
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
    const char* why = make_rm_cb(descs[i], cbs[i].rm);
    if (why == nullptr) {
      why = make_mod_seg(mod[i], blocks, cbs[i].mod);
    }
    if (why == nullptr && mod[i].modulation == LDPC_HIP_MOD_PI_2_BPSK) {
      why = "rate_match_modulate_launch: pi/2-BPSK is not a PDSCH scheme (a span per codeblock would restart the "
            "symbol parity): rate-match, then ldpc_hip_modulate_launch over the codeword";
    }
    if (why == nullptr && (bits_per_symbol(mod[i].modulation) != descs[i].modulation_order ||
                           static_cast<uint64_t>(mod[i].nof_symbols) * descs[i].modulation_order != descs[i].rm_length ||
                           descs[i].rm_length >= 0x80000000U)) {
      why = "rate_match_modulate_launch: symbols x bits per symbol must equal rm_length, the scheme's bits per symbol "
            "modulation_order";
    }
    if (why != nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  hipError_t  e = upload_descs(ctx->d_rmmod, ctx->c_rmmod, cbs.data(), cbs.size() * sizeof(rm_mod_cb), s);
  if (e == hipSuccess) {
    e = launch_rate_match_modulate(ctx->d_rmmod.as<rm_mod_cb>(), nof_cbs, static_cast<uint32_t>(blocks),
                                   format == LDPC_HIP_SYM_CI8, d_cws, d_symbols, s);
  }
  return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "ldpc_rate_match_modulate_kernel launch");
}

} /* extern "C" */
