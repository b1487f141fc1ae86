/*
 * The precoder's entry points of the C ABI (include/srsran_ldpc_hip.h): ldpc_hip_precode_supported,
 * ldpc_hip_precode_map_launch and ldpc_hip_precode_sync, with the translation of the rows, their masks (the per-word
 * prefix counts are computed here) and their weights into the one table the kernel of ldpc_precode_kernels.hip reads.
 */
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "ldpc_hip_ctx.h"
#include "ldpc_precode.h"

using namespace ldpc_hip;

namespace {

/* A weight component the reference's complex multiply handles without its NaN fall-back (__mulsc3, taken only when
 * both result components are NaN): finite and below 2^64, so that no intermediate overflows (127 2^64 2 4 < FLT_MAX). */
bool weight_ok(float v) { return std::isfinite(v) && std::fabs(v) < 18446744073709551616.0F; }

/* the launch's table: rows, then mask words, then weights (16-byte aligned each) */
struct precode_table {
  std::vector<precode_row>  rows;
  std::vector<precode_word> words;
  uint32_t                  nblocks = 0;
  std::vector<uint8_t>      blob;
  size_t                    words_at = 0, weights_at = 0;
};

/* compact: the row is a channel_precoder call's, one PRG whatever its length */
const char* make_precode_table(uint32_t n, const ldpc_hip_precode_desc* descs, const float* weights,
                               uint32_t nof_weights, const uint64_t* masks, uint32_t nof_mask_words, bool compact,
                               precode_table& t)
{
  for (uint64_t i = 0; i != 2ULL * nof_weights; ++i) {
    if (!weight_ok(weights[i])) {
      return "precode: a weight component is not finite or is 2^64 or more in magnitude";
    }
  }
  /* a mask's words with their prefix counts, once per (first word, words) */
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
  uint64_t                                          blocks = 0;
  for (uint32_t i = 0; i != n; ++i) {
    const ldpc_hip_precode_desc& d = descs[i];
    if (!precode_supported(d.nof_layers, d.nof_ports)) {
      return "precode: unsupported topology (1 <= layers <= ports <= 4)";
    }
    if (d.prg_size == 0) {
      return "precode: prg_size must be at least 1";
    }
    if (!compact && d.width > d.port_stride) {
      return "precode: a row is wider than its port stride";
    }
    const uint32_t nw = (d.width + 63U) / 64U;
    if (d.mask_offset > nof_mask_words || nw > nof_mask_words - d.mask_offset) {
      return "precode: a row's mask lies outside the masks";
    }
    const uint64_t* m = masks + d.mask_offset;
    if (d.width % 64U != 0 && (m[nw - 1] >> (d.width % 64U)) != 0) {
      return "precode: a mask bit beyond the row's width";
    }
    uint32_t lo = nw, hi = 0;
    for (uint32_t w = 0; w != nw; ++w) {
      if (m[w] != 0) {
        lo = lo == nw ? w : lo;
        hi = w;
      }
    }
    if (lo == nw) {
      continue; /* no masked RE */
    }
    const uint32_t prg_subc = compact ? 0xffffffffU : 12U * d.prg_size;
    const uint32_t k_last   = hi * 64U + 63U - static_cast<uint32_t>(__builtin_clzll(m[hi]));
    const uint64_t wl       = static_cast<uint64_t>(d.nof_layers) * d.nof_ports;
    if (k_last / prg_subc >= d.nof_prg || d.weight_offset > nof_weights ||
        d.nof_prg * wl > nof_weights - d.weight_offset) {
      return "precode: a masked subcarrier's PRG lies outside the weight block";
    }
    auto it = seen.find({d.mask_offset, nw});
    if (it == seen.end()) {
      it = seen.emplace(std::make_pair(d.mask_offset, nw), static_cast<uint32_t>(t.words.size())).first;
      uint64_t prefix = 0;
      for (uint32_t w = 0; w != nw; ++w) {
        t.words.push_back(precode_word{m[w], static_cast<uint32_t>(prefix), 0});
        prefix += static_cast<uint64_t>(__builtin_popcountll(m[w]));
      }
    }
    precode_row r{};
    r.in_offset  = d.sym_offset;
    r.out_offset = d.grid_offset;
    r.out_stride = d.port_stride;
    r.word0      = it->second;
    r.weight0    = d.weight_offset;
    r.k_begin    = lo * 64U;
    r.k_end      = std::min(d.width, (hi + 1U) * 64U);
    r.prg_subc   = prg_subc;
    r.block0     = static_cast<uint32_t>(blocks);
    r.nof_layers = d.nof_layers;
    r.nof_ports  = d.nof_ports;
    blocks += (r.k_end - r.k_begin + PC_BLOCK * PC_RES - 1U) / (PC_BLOCK * PC_RES);
    if (blocks > MAX_LAUNCH_BLOCKS) {
      return "precode: too many blocks in one launch";
    }
    t.rows.push_back(r);
  }
  t.nblocks    = static_cast<uint32_t>(blocks);
  t.words_at   = t.rows.size() * sizeof(precode_row);
  t.weights_at = t.words_at + t.words.size() * sizeof(precode_word);
  t.blob.resize(t.weights_at + 8U * static_cast<size_t>(nof_weights));
  if (!t.rows.empty()) {
    std::memcpy(t.blob.data(), t.rows.data(), t.words_at);
    std::memcpy(t.blob.data() + t.words_at, t.words.data(), t.weights_at - t.words_at);
    std::memcpy(t.blob.data() + t.weights_at, weights, 8U * static_cast<size_t>(nof_weights));
  }
  return nullptr;
}

int precode_rows(ldpc_hip_ctx* ctx, precode_table& t, const void* d_in, void* d_out, bool in_cf32, bool compact,
                 hipStream_t s)
{
  if (t.rows.empty()) {
    return LDPC_HIP_OK;
  }
  hipError_t e = ctx->d_precode.upload(t.blob.data(), t.blob.size(), s);
  if (e == hipSuccess) {
    const uint8_t* base = ctx->d_precode.as<uint8_t>();
    e = launch_precode(reinterpret_cast<const precode_row*>(base), static_cast<uint32_t>(t.rows.size()), t.nblocks,
                       reinterpret_cast<const precode_word*>(base + t.words_at),
                       reinterpret_cast<const float*>(base + t.weights_at), d_in, d_out, in_cf32, compact, s);
  }
  return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "ldpc_precode_kernel launch");
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
  if (const char* why = make_precode_table(nof_rows, descs, weights, nof_weights, masks, nof_mask_words, false, t)) {
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
                                           static_cast<uint32_t>(mask.size()), true, t)) {
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
  hipError_t   e;
  if ((e = ctx->d_llr.reserve(nin)) != hipSuccess || (e = ctx->d_sym.reserve(nout)) != hipSuccess) {
    return ctx->hip_fail(e, "hipMalloc(precode)");
  }
  if ((e = hipMemcpyAsync(ctx->d_llr.ptr, input, nin, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "hipMemcpyAsync(precode in)");
  }
  t.rows[0].in_stride = nof_re;
  std::memcpy(t.blob.data(), t.rows.data(), sizeof(precode_row));
  const int r = precode_rows(ctx, t, ctx->d_llr.ptr, ctx->d_sym.ptr, cf32, true, ctx->stream);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  if ((e = hipMemcpyAsync(output, ctx->d_sym.ptr, nout, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "precode_sync");
  }
  return LDPC_HIP_OK;
}

} /* extern "C" */
