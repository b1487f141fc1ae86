/*
 * The precoder's code object (downlink, behind the modulation mapper; nothing of the decoder, the uplink family, the
 * mapper or the equalizer is compiled here): ldpc_precode_kernel and its host launcher (ldpc_precode.h).
 *
 * resource_grid_mapper_impl.cpp:293-436 takes the masked REs of a transmission in ascending (symbol, subcarrier)
 * order, hands each PRG's share to channel_precoder_generic.cpp:50-70 and puts the result into the grid as cbf16
 * (resource_grid_writer_impl.cpp:44-81), and so does the kernel, operand by operand in float32:
 *   the r-th masked RE reads layer i at input[L r + i] (layer mapping by de-interleaving); its PRG is k / (12
 *   prg_size) from grid subcarrier 0; per port sum = to_cf(x_0) w_0 (assigned, so a zero keeps the product's sign), then
 *   sum += to_cf(x_i) w_i for i = 1 .. L - 1 in ascending order; a complex product is (ac - bd, ad + bc) in separate
 *   multiplies and adds (no contraction in this file); cf32 to cbf16 is u += 0x7fff + ((u >> 16) & 1), u >>= 16 on
 *   each component's bits (bf16.h:38-55), Re in the low half of the element.
 * channel_precoder_impl.cpp:27-70 with channel_precoder_generic.cpp:27-48 (cf32 layer planes in, cf32 port planes out)
 * is the same arithmetic; the three instances of the one body are (ci8, grid), (ci8, compact) and (cf32, compact).
 *
 * A thread owns PC_RES = 4 consecutive subcarriers of its row, one nibble of the mask, for every port. The rank of its
 * first masked subcarrier is the word's prefix plus the population count of the word's bits below the nibble. Its
 * L popcount(nibble) input symbols are consecutive: 8- or 16-byte loads for a full nibble where the address allows,
 * else 4-byte loads from the first 4-byte boundary with 2-byte loads at either end. A full nibble on a 16-byte-aligned
 * grid address leaves as one 16-byte store per port, anything else as 4-byte stores of the set bits only. Nothing
 * outside a row's L count symbols is read and nothing outside its masked REs written. No LDS, no scratch: every
 * register array is indexed by unrolled constants, and a partial nibble picks its results through selects.
 *
 * The ten (L, P) bodies sit behind one block-uniform switch (a row is block-uniform), as the equalizer's.
 */
#include "ldpc_block_item.h"
#include "ldpc_precode.h"

#pragma clang fp contract(off)

namespace ldpc_hip {
namespace {

struct pc_cf {
  float re, im;
};

__device__ __forceinline__ pc_cf pc_mul(pc_cf a, pc_cf b)
{
  return pc_cf{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
/* to_cf(ci8_t): int8 re in the low byte, int8 im in the high byte of a 16-bit element */
__device__ __forceinline__ pc_cf pc_from_ci8(uint32_t e)
{
  return pc_cf{static_cast<float>(static_cast<int8_t>(e & 0xffU)), static_cast<float>(static_cast<int8_t>(e >> 8))};
}
__device__ __forceinline__ uint32_t pc_bf16(float x)
{
  uint32_t u = __float_as_uint(x);
  u += 0x7fffU + ((u >> 16) & 1U);
  return u >> 16;
}
__device__ __forceinline__ uint32_t pc_cbf16(pc_cf v) { return pc_bf16(v.re) | (pc_bf16(v.im) << 16); }

/* the n <= 4 L consecutive ci8 elements at p (n >= 1), the rest zero */
template <int L>
__device__ __forceinline__ void pc_load_ci8(const uint16_t* __restrict__ p, uint32_t n, uint32_t (&e)[4 * L])
{
  constexpr int   N = 4 * L;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (n == static_cast<uint32_t>(N) && (a & 7U) == 0) { /* 8 L bytes */
    uint32_t w[N / 2];
    if (L % 2 == 0 && (a & 15U) == 0) {
#pragma unroll
      for (int g = 0; g < N / 8; ++g) {
        const uint4 v = reinterpret_cast<const uint4*>(p)[g];
        w[4 * g] = v.x, w[4 * g + 1] = v.y, w[4 * g + 2] = v.z, w[4 * g + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int g = 0; g < N / 4; ++g) {
        const uint2 v = reinterpret_cast<const uint2*>(p)[g];
        w[2 * g] = v.x, w[2 * g + 1] = v.y;
      }
    }
#pragma unroll
    for (int d = 0; d < N / 2; ++d) {
      e[2 * d] = w[d] & 0xffffU, e[2 * d + 1] = w[d] >> 16;
    }
  } else if ((a & 2U) == 0) { /* 4-byte aligned: pairs from the first element */
#pragma unroll
    for (int d = 0; d < N / 2; ++d) {
      uint32_t w = 0;
      if (static_cast<uint32_t>(2 * d + 1) < n) {
        w = *reinterpret_cast<const uint32_t*>(p + 2 * d);
      } else if (static_cast<uint32_t>(2 * d) < n) {
        w = p[2 * d];
      }
      e[2 * d] = w & 0xffffU, e[2 * d + 1] = w >> 16;
    }
  } else { /* one element, then pairs */
    e[0] = p[0];
#pragma unroll
    for (int d = 0; d < N / 2 - 1; ++d) {
      uint32_t w = 0;
      if (static_cast<uint32_t>(2 * d + 2) < n) {
        w = *reinterpret_cast<const uint32_t*>(p + 2 * d + 1);
      } else if (static_cast<uint32_t>(2 * d + 1) < n) {
        w = p[2 * d + 1];
      }
      e[2 * d + 1] = w & 0xffffU, e[2 * d + 2] = w >> 16;
    }
    e[N - 1] = static_cast<uint32_t>(N - 1) < n ? p[N - 1] : 0U;
  }
}

/* the thread's nibble: the row's subcarriers k0 .. k0 + 3 */
template <bool IN_CF32, bool COMPACT, int L, int P>
__device__ __forceinline__ void pc_nibble(const precode_row& rw, uint32_t k0, const precode_word* __restrict__ words,
                                          const float* __restrict__ weights, const void* __restrict__ in,
                                          void* __restrict__ out)
{
  if (k0 >= rw.k_end) {
    return;
  }
  const precode_word mw  = words[rw.word0 + k0 / 64U];
  const uint32_t     sh  = k0 & 63U;
  const uint32_t     nib = static_cast<uint32_t>(mw.bits >> sh) & 0xfU;
  if (nib == 0U) {
    return;
  }
  const uint32_t cnt = __popc(nib);
  const uint64_t r0  = mw.prefix + static_cast<uint32_t>(__popcll(mw.bits & ((1ULL << sh) - 1ULL)));

  /* the PRG's weights [port][layer]; the nibble lies in one PRG (12 prg_size is a multiple of 4) */
  const float2* wp = reinterpret_cast<const float2*>(weights) + rw.weight0 +
                     static_cast<uint64_t>(k0 / rw.prg_subc) * static_cast<uint32_t>(P * L);
  pc_cf w[P][L];
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const float2 v = wp[p * L + i];
      w[p][i]        = pc_cf{v.x, v.y};
    }
  }

  /* x[q][i]: layer i of the nibble's q-th masked subcarrier; zero for q >= cnt */
  pc_cf x[PC_RES][L];
  if constexpr (IN_CF32) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const float2* pl = static_cast<const float2*>(in) + rw.in_offset + static_cast<uint64_t>(i) * rw.in_stride + r0;
      if (cnt == PC_RES && (reinterpret_cast<uintptr_t>(pl) & 15U) == 0) {
        const float4 lo = reinterpret_cast<const float4*>(pl)[0], hi = reinterpret_cast<const float4*>(pl)[1];
        x[0][i] = pc_cf{lo.x, lo.y}, x[1][i] = pc_cf{lo.z, lo.w};
        x[2][i] = pc_cf{hi.x, hi.y}, x[3][i] = pc_cf{hi.z, hi.w};
      } else {
#pragma unroll
        for (int q = 0; q < PC_RES; ++q) {
          x[q][i] = pc_cf{0.0F, 0.0F};
          if (static_cast<uint32_t>(q) < cnt) {
            const float2 v = pl[q];
            x[q][i]        = pc_cf{v.x, v.y};
          }
        }
      }
    }
  } else {
    uint32_t e[PC_RES * L];
    pc_load_ci8<L>(static_cast<const uint16_t*>(in) + rw.in_offset + static_cast<uint64_t>(L) * r0,
                   static_cast<uint32_t>(L) * cnt, e);
#pragma unroll
    for (int q = 0; q < PC_RES; ++q) {
#pragma unroll
      for (int i = 0; i < L; ++i) {
        x[q][i] = pc_from_ci8(e[L * q + i]);
      }
    }
  }

  /* channel_precoder_generic.cpp:58-68 */
  pc_cf o[PC_RES][P];
#pragma unroll
  for (int q = 0; q < PC_RES; ++q) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      pc_cf sum = pc_mul(x[q][0], w[p][0]);
#pragma unroll
      for (int i = 1; i < L; ++i) {
        const pc_cf m = pc_mul(x[q][i], w[p][i]);
        sum.re += m.re;
        sum.im += m.im;
      }
      o[q][p] = sum;
    }
  }

#pragma unroll
  for (int p = 0; p < P; ++p) {
    if constexpr (COMPACT) {
      float2* c = static_cast<float2*>(out) + rw.out_offset + static_cast<uint64_t>(p) * rw.out_stride + r0;
      if (cnt == PC_RES && (reinterpret_cast<uintptr_t>(c) & 15U) == 0) {
        reinterpret_cast<float4*>(c)[0] = make_float4(o[0][p].re, o[0][p].im, o[1][p].re, o[1][p].im);
        reinterpret_cast<float4*>(c)[1] = make_float4(o[2][p].re, o[2][p].im, o[3][p].re, o[3][p].im);
      } else {
#pragma unroll
        for (int q = 0; q < PC_RES; ++q) {
          if (static_cast<uint32_t>(q) < cnt) {
            c[q] = make_float2(o[q][p].re, o[q][p].im);
          }
        }
      }
    } else {
      uint32_t* g = static_cast<uint32_t*>(out) + rw.out_offset + static_cast<uint64_t>(p) * rw.out_stride + k0;
      if (nib == 0xfU && (reinterpret_cast<uintptr_t>(g) & 15U) == 0) {
        *reinterpret_cast<uint4*>(g) =
            make_uint4(pc_cbf16(o[0][p]), pc_cbf16(o[1][p]), pc_cbf16(o[2][p]), pc_cbf16(o[3][p]));
      } else {
#pragma unroll
        for (int b = 0; b < PC_RES; ++b) {
          if (((nib >> b) & 1U) != 0U) {
            /* the bit's rank in the nibble, at most b */
            const uint32_t q = __popc(nib & ((1U << b) - 1U));
            pc_cf          v = o[0][p];
#pragma unroll
            for (int s = 1; s <= b; ++s) {
              v = q == static_cast<uint32_t>(s) ? o[s][p] : v;
            }
            g[b] = pc_cbf16(v);
          }
        }
      }
    }
  }
}

} // namespace

template <bool IN_CF32, bool COMPACT>
__global__ void __launch_bounds__(PC_BLOCK)
    ldpc_precode_kernel(const precode_row* __restrict__ rows, uint32_t nrows, const precode_word* __restrict__ words,
                        const float* __restrict__ weights, const void* __restrict__ in, void* __restrict__ out)
{
  const precode_row rw = rows[block_item(rows, nrows)];
  const uint32_t    k0 = rw.k_begin + ((blockIdx.x - rw.block0) * PC_BLOCK + threadIdx.x) * PC_RES;
  /* block-uniform; the host admits these ten only */
#define PC_CASE(L, P)                                                          \
  case (L - 1) * 4 + (P - 1):                                                  \
    pc_nibble<IN_CF32, COMPACT, L, P>(rw, k0, words, weights, in, out);        \
    break;
  switch ((rw.nof_layers - 1U) * 4U + (rw.nof_ports - 1U)) {
    PC_CASE(1, 1)
    PC_CASE(1, 2)
    PC_CASE(1, 3)
    PC_CASE(1, 4)
    PC_CASE(2, 2)
    PC_CASE(2, 3)
    PC_CASE(2, 4)
    PC_CASE(3, 3)
    PC_CASE(3, 4)
    PC_CASE(4, 4)
    default: break;
  }
#undef PC_CASE
}

hipError_t launch_precode(const precode_row* d_rows, uint32_t nrows, uint32_t nblocks, const precode_word* d_words,
                          const float* d_weights, const void* d_in, void* d_out, bool in_cf32, bool compact,
                          hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  if (in_cf32 && !compact) {
    return hipErrorInvalidValue;
  }
  if (in_cf32) {
    hipLaunchKernelGGL((ldpc_precode_kernel<true, true>), dim3(nblocks), dim3(PC_BLOCK), 0, stream, d_rows, nrows,
                       d_words, d_weights, d_in, d_out);
  } else if (compact) {
    hipLaunchKernelGGL((ldpc_precode_kernel<false, true>), dim3(nblocks), dim3(PC_BLOCK), 0, stream, d_rows, nrows,
                       d_words, d_weights, d_in, d_out);
  } else {
    hipLaunchKernelGGL((ldpc_precode_kernel<false, false>), dim3(nblocks), dim3(PC_BLOCK), 0, stream, d_rows, nrows,
                       d_words, d_weights, d_in, d_out);
  }
  return hipGetLastError();
}

} // namespace ldpc_hip
