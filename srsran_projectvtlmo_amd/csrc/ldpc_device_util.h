/*
 * Device helpers shared by every kernel: the LLR constants, the wave reductions, the CRC arithmetic, the absolute LDS
 * pointers and the clamps. Nothing of the decoder: the downlink code object (ldpc_downlink_kernels.hip) and the uplink
 * family (ldpc_uplink_kernels.h) include only this header, ldpc_dwq_loop.h and ldpc_dematch_body.h.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ldpc_hip_device.h"

namespace ldpc_hip {
namespace {

constexpr int LLR_MAX = 120;
constexpr int LLR_INF = 127;
constexpr int LLR_INTERNAL_INF = LLR_MAX + 1; /* decoder-internal infinity, see "Check-to-variable storage" */

__device__ __forceinline__ bool llr_isinf(int v) { return v > LLR_MAX || v < -LLR_MAX; }

/* Wave-wide XOR reduction (wave64): DPP within each 16-lane row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
 * row_mirror), then the four rows' lanes 0, 16, 32, 48 read out as scalars: no LDS round trips (a ds_bpermute
 * butterfly costs six). Every lane gets the total. */
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
  v ^= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xb1, 0xf, 0xf, false));
  v ^= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x4e, 0xf, 0xf, false));
  v ^= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x141, 0xf, 0xf, false));
  v ^= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x140, 0xf, 0xf, false));
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 0) ^
                               __builtin_amdgcn_readlane(static_cast<int>(v), 16) ^
                               __builtin_amdgcn_readlane(static_cast<int>(v), 32) ^
                               __builtin_amdgcn_readlane(static_cast<int>(v), 48));
}

/* Wave-wide maximum of non-negative ints, the same DPP pattern as wave_xor; every lane gets the result. */
__device__ __forceinline__ int wave_max(int v)
{
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false));
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

/* (a(x) * b(x)) mod G(x) over GF(2); a, b of degree < order; poly includes the x^order term. */
__device__ __forceinline__ uint32_t gf2_mulmod(uint32_t a, uint32_t b, int order, uint32_t poly)
{
  /* a * b mod poly over GF(2) for a, b < x^order (order <= 24; poly includes its x^order term), Horner over the bits
   * of b from the top: 32-bit operations only, the remainder reduced at every step */
  const uint32_t top = 1U << order;
  uint32_t       r   = 0;
  for (int i = order - 1; i >= 0; --i) {
    r <<= 1;
    r ^= (r & top) ? poly : 0U;
    r ^= ((b >> i) & 1U) ? a : 0U;
  }
  return r;
}

__device__ __forceinline__ void crc_params(int poly_id, int& order, uint32_t& poly)
{
  /* hw_dec_cb_crc_type numbering; polynomials of crc_calculator_generic_impl.cpp:28-56 */
  if (poly_id == LDPC_HIP_CRC16) {
    order = 16;
    poly  = 0x11021U;
  } else if (poly_id == LDPC_HIP_CRC24B) {
    order = 24;
    poly  = 0x1800063U;
  } else {
    order = 24;
    poly  = 0x1864cfbU;
  }
}

/* CRC remainder of the first L bits of the packed (MSB-first) message in LDS. Linear decomposition:
 * front-pad to nw 32-bit words (leading zeros do not change a zero-init CRC), remainder =
 * XOR_w [(W_w * x^r mod G) * (x^(32 (nw-1-w)) mod G) mod G]. Block-uniform result. s_table: the poly's LDS copy
 * (CRC_LDS_WORDS: slicing-by-4 tables T_0..T_3, then the powers), so a word's CRC is four independent LDS lookups
 * and its power one more, with no global load on the early-stop path. */
[[maybe_unused]] __device__ uint32_t block_crc(const uint8_t* hb, int L, int poly_id, const uint32_t* s_table,
                                               uint32_t* s_red, const uint32_t* __restrict__ g_mcol)
{
  const uint32_t* g_pow = s_table + 4 * 256;
  int      order;
  uint32_t poly;
  crc_params(poly_id, order, poly);
  const uint32_t mask = (order == 32) ? 0xffffffffU : ((1U << order) - 1U);
  const int      nw   = (L + 31) / 32;
  const int      p    = nw * 32 - L;
  uint32_t       acc  = 0;
  for (int w = threadIdx.x; w < nw; w += blockDim.x) {
    /* the multiplier's columns first (global, L2-resident; independent of the message, so their latency overlaps the
     * LDS reads below) */
    const uint4* mc = reinterpret_cast<const uint4*>(g_mcol + (nw - 1 - w) * 24);
    uint4        col[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      col[q] = mc[q];
    }
    /* hb is 4-byte aligned (lay.hard): one LDS dword per word, byte-swapped to MSB-first */
    auto be = [&](int i) -> uint32_t {
      if (i < 0) {
        return 0U;
      }
      return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(hb + 4 * i));
    };
    const uint32_t W   = (p == 0) ? be(w) : ((be(w - 1) << (32 - p)) | (be(w) >> p));
    const uint32_t crc = (s_table[3 * 256 + (W >> 24)] ^ s_table[2 * 256 + ((W >> 16) & 0xffU)] ^
                          s_table[256 + ((W >> 8) & 0xffU)] ^ s_table[W & 0xffU]) & mask;
    /* crc * x^(32 (nw - 1 - w)) mod G: the XOR of the columns of crc's set bits (bits >= order are zero) */
    const uint32_t cw[24] = {col[0].x, col[0].y, col[0].z, col[0].w, col[1].x, col[1].y, col[1].z, col[1].w,
                             col[2].x, col[2].y, col[2].z, col[2].w, col[3].x, col[3].y, col[3].z, col[3].w,
                             col[4].x, col[4].y, col[4].z, col[4].w, col[5].x, col[5].y, col[5].z, col[5].w};
    uint32_t       prod[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      prod[i & 3] ^= cw[i] & (0U - ((crc >> i) & 1U));
    }
    acc ^= (prod[0] ^ prod[1]) ^ (prod[2] ^ prod[3]);
    (void)g_pow;
  }
  acc              = wave_xor(acc);
  const int wave   = threadIdx.x >> 6;
  const int nwaves = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_red[wave] = acc;
  }
  __syncthreads();
  /* lane i reads wave i's word (one LDS read, not a chain of nwaves dependent ones), then a wave XOR */
  const int lane = threadIdx.x & 63;
  return wave_xor(lane < nwaves ? s_red[lane] : 0U);
}

__device__ __forceinline__ int med3i(int x, int lo, int hi) { return min(max(x, lo), hi); } /* v_med3_i32 */

/* Four int8 LLRs with +-127 (infinity) mapped to the decoder-internal +-121. */
__device__ __forceinline__ uint32_t clamp_inf4(uint32_t w)
{
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int v = med3i(__builtin_amdgcn_sbfe(static_cast<int>(w), 8 * b, 8), -LLR_INTERNAL_INF, LLR_INTERNAL_INF);
    r |= (static_cast<uint32_t>(v) & 0xffU) << (8 * b);
  }
  return r;
}

/* LDS byte at an absolute LDS address. The decode kernel has no static LDS, so its dynamic LDS (smem) starts at LDS
 * address 0 and the soft bits (lay.soft == 0) are addressed by column offset alone -- checked once per launch. */
typedef __attribute__((address_space(3))) int8_t lds_i8;
__device__ __forceinline__ lds_i8* lds_byte(uint32_t addr) { return (lds_i8*)(uintptr_t)addr; }
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ lds_u32* lds_word(uint32_t addr) { return (lds_u32*)(uintptr_t)addr; }

} // namespace
} // namespace ldpc_hip
