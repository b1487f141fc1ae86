/*
 * The PDSCH DM-RS generator's code object (downlink, beside the precoder in the resource grid; nothing of the decoder,
 * the uplink family, the mapper, the equalizer or the precoder is compiled here): ldpc_dmrs_kernel and its host
 * launcher (ldpc_dmrs.h).
 *
 * dmrs_pdsch_processor_impl.cpp:84-262 generates, per DM-RS symbol, the pilots of the allocated resource blocks from
 * the sequence of the symbol's c_init (dmrs_helper.h:44-109 over pseudo_random_generator_impl.cpp:154-246), applies
 * each DM-RS port's CDM code and hands each CDM group's one or two layers to resource_grid_mapper_impl.cpp:47-147,
 * 165-291, which precodes them on one PRG (channel_precoder_generic.cpp:27-48) and puts the result into the grid as
 * cbf16 (resource_grid_writer_impl.cpp). So does the kernel, operand by operand:
 *   pilot j (0 <= j < dpr; dpr = 6 for type 1, 4 for type 2) of resource block n uses the sequence bits
 *   b = 2 (dpr (n - reference_point_k_rb) + j) and b + 1, wherever the allocation's other resource blocks are; its
 *   value is (a ^ c(b) << 31, a ^ c(b + 1) << 31) on the bits of a = (float)(M_SQRT1_2 * (double)amplitude);
 *   DM-RS port i is layer i in CDM group i / 2, on subcarriers 2 j + g (type 1) or {2 g, 2 g + 1, 6 + 2 g, 7 + 2 g}
 *   (type 2) of the resource block; the group's second port (odd i) has its odd-j pilots negated, both components'
 *   sign bits flipped; with ports 0 to 3 only, w_t is +1 whether DM-RS symbols are adjacent or not;
 *   per CDM group and antenna port sum = x_0 w_0 (assigned), then sum += x_1 w_1; a complex product is (ac - bd,
 *   ad + bc) in separate multiplies and adds (no contraction in this file); cf32 to cbf16 is u += 0x7fff +
 *   ((u >> 16) & 1), u >>= 16 on each component's bits, Re in the low half of the element;
 *   one layer on one port with the weight 1 + 0j is stored unmultiplied (the mapper's bypass), which shows at a = +-0.
 *
 * A thread owns DMRS_RBS = 1 resource block of its row, for every CDM group and port: one prs_jump_words from the
 * symbol's start state to the 32-bit sequence word of its first bit, two prs_next_word steps, and its 2 dpr bits,
 * which may straddle a word, are in a 64-bit window. No input buffer, no LDS, no scratch: every register array is
 * indexed by unrolled constants. The two output forms of the one body are cbf16 grid elements and, at the same element
 * offsets and strides, the cf32 values before the rounding.
 *
 * The ten (L, P) bodies sit behind one block-uniform switch (a row is block-uniform), as the precoder's; the type and
 * the bypass are block-uniform branches inside a body.
 */
#include "ldpc_block_item.h"
#include "ldpc_dmrs.h"
#include "ldpc_prs_device.h"

#pragma clang fp contract(off)

namespace ldpc_hip {
namespace {

struct dm_cf {
  float re, im;
};

__device__ __forceinline__ dm_cf dm_mul(dm_cf a, dm_cf b)
{
  return dm_cf{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ uint32_t dm_bf16(float x)
{
  uint32_t u = __float_as_uint(x);
  u += 0x7fffU + ((u >> 16) & 1U);
  return u >> 16;
}
__device__ __forceinline__ uint32_t dm_cbf16(dm_cf v) { return dm_bf16(v.re) | (dm_bf16(v.im) << 16); }

/* one resource block: `bits` holds its 2 dpr sequence bits from bit 0, rb its first subcarrier's elements of port 0 */
template <bool CF32, int L, int P>
__device__ __forceinline__ void dm_rb(const dmrs_row& rw, uint32_t bits, const dm_cf (&w)[P][L], uint64_t rb,
                                      void* __restrict__ out)
{
  const uint32_t a    = __float_as_uint(rw.a);
  const bool     t1   = rw.type == 1;
  const uint32_t dpr  = t1 ? 6U : 4U;
  constexpr int  NCDM = (L + 1) / 2;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    if (static_cast<uint32_t>(j) < dpr) {
      const uint32_t re = a ^ (((bits >> (2 * j)) & 1U) << 31), im = a ^ (((bits >> (2 * j + 1)) & 1U) << 31);
      const dm_cf    x0{__uint_as_float(re), __uint_as_float(im)};
      /* the CDM group's second port: w_f = {+1, -1} */
      const uint32_t flip = (j & 1) != 0 ? 0x80000000U : 0U;
      const dm_cf    x1{__uint_as_float(re ^ flip), __uint_as_float(im ^ flip)};
#pragma unroll
      for (int g = 0; g < NCDM; ++g) {
        const uint32_t subc = t1 ? 2 * j + g : (j < 2 ? 2 * g + j : 4 + 2 * g + j);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          dm_cf v = x0;
          if (!(L == 1 && P == 1 && rw.bypass != 0)) {
            v = dm_mul(x0, w[p][2 * g]);
            if (2 * g + 1 < L) { /* folded once g is unrolled */
              const dm_cf m = dm_mul(x1, w[p][2 * g + 1 < L ? 2 * g + 1 : 0]);
              v.re += m.re;
              v.im += m.im;
            }
          }
          const uint64_t e = rb + static_cast<uint64_t>(p) * rw.out_stride + subc;
          if constexpr (CF32) {
            static_cast<float2*>(out)[e] = make_float2(v.re, v.im);
          } else {
            static_cast<uint32_t*>(out)[e] = dm_cbf16(v);
          }
        }
      }
    }
  }
}

/* the thread's resource blocks: n0 .. n0 + DMRS_RBS - 1 of the row */
template <bool CF32, int L, int P>
__device__ __forceinline__ void dm_rbs(const dmrs_row& rw, uint32_t n0, const uint64_t* __restrict__ words,
                                       const float* __restrict__ weights, void* __restrict__ out)
{
  bool set[DMRS_RBS];
  bool any = false;
#pragma unroll
  for (int r = 0; r < DMRS_RBS; ++r) {
    const uint32_t n = n0 + r;
    set[r]           = n < rw.rb_end && ((words[rw.word0 + n / 64U] >> (n & 63U)) & 1ULL) != 0ULL;
    any              = any || set[r];
  }
  if (!any) {
    return;
  }
  const float2* wp = reinterpret_cast<const float2*>(weights) + rw.weight0;
  dm_cf         w[P][L];
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const float2 v = wp[p * L + i];
      w[p][i]        = dm_cf{v.x, v.y};
    }
  }
  /* the thread's first sequence bit; its 2 DMRS_RBS dpr bits end before bit 64 of the word it lies in (ldpc_dmrs.h) */
  const uint32_t per_rb = rw.type == 1 ? 12U : 8U;
  const uint32_t b0     = per_rb * (n0 - rw.ref_rb);
  uint32_t       x1 = rw.x1, x2 = rw.x2;
  prs_jump_words(x1, x2, b0 >> 5);
  const uint64_t lo  = prs_next_word(x1, x2);
  const uint64_t hi  = prs_next_word(x1, x2);
  const uint64_t win = (lo | (hi << 32)) >> (b0 & 31U);
#pragma unroll
  for (int r = 0; r < DMRS_RBS; ++r) {
    if (set[r]) {
      dm_rb<CF32, L, P>(rw, static_cast<uint32_t>(win >> (per_rb * r)), w,
                        rw.out_offset + 12ULL * (n0 + static_cast<uint32_t>(r)), out);
    }
  }
}

} // namespace

template <bool CF32>
__global__ void __launch_bounds__(DMRS_BLOCK)
    ldpc_dmrs_kernel(const dmrs_row* __restrict__ rows, uint32_t nrows, const uint64_t* __restrict__ words,
                     const float* __restrict__ weights, void* __restrict__ out)
{
  const dmrs_row rw = rows[block_item(rows, nrows)];
  const uint32_t n0 = rw.rb_begin + ((blockIdx.x - rw.block0) * DMRS_BLOCK + threadIdx.x) * DMRS_RBS;
  if (n0 >= rw.rb_end) {
    return;
  }
  /* block-uniform; the host admits these ten only */
#define DM_CASE(L, P)                                         \
  case (L - 1) * 4 + (P - 1):                                 \
    dm_rbs<CF32, L, P>(rw, n0, words, weights, out);          \
    break;
  switch ((rw.nof_layers - 1U) * 4U + (rw.nof_ports - 1U)) {
    DM_CASE(1, 1)
    DM_CASE(1, 2)
    DM_CASE(1, 3)
    DM_CASE(1, 4)
    DM_CASE(2, 2)
    DM_CASE(2, 3)
    DM_CASE(2, 4)
    DM_CASE(3, 3)
    DM_CASE(3, 4)
    DM_CASE(4, 4)
    default: break;
  }
#undef DM_CASE
}

hipError_t launch_dmrs(const dmrs_row* d_rows, uint32_t nrows, uint32_t nblocks, const uint64_t* d_words,
                       const float* d_weights, void* d_out, bool cf32, hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  if (cf32) {
    hipLaunchKernelGGL((ldpc_dmrs_kernel<true>), dim3(nblocks), dim3(DMRS_BLOCK), 0, stream, d_rows, nrows, d_words,
                       d_weights, d_out);
  } else {
    hipLaunchKernelGGL((ldpc_dmrs_kernel<false>), dim3(nblocks), dim3(DMRS_BLOCK), 0, stream, d_rows, nrows, d_words,
                       d_weights, d_out);
  }
  return hipGetLastError();
}

} // namespace ldpc_hip
