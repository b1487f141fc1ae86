/*
 * The pseudo-random sequence on the device (TS 38.211 5.2.1; ldpc_hip_device.h "pseudo-random sequence generator"),
 * shared by the uplink (descrambler, packed-bit scrambler, the dematcher's fused descrambler: ldpc_dematch_body.h,
 * ldpc_uplink_kernels.h) and the downlink (the modulation mapper's scrambler: ldpc_modulation_kernels.hip; the PDSCH
 * DM-RS generator: ldpc_dmrs_kernels.hip).
 * A thread owns a run of consecutive 32-bit sequence words of its segment: it jumps from the segment's start state to
 * its first word (prs_jump_words: one polynomial jump per non-zero radix-32 digit of the word index, the polynomials
 * from g_prs_jump, 1.5 KiB of constant data built at compile time from the recurrences) and then steps word by word
 * (prs_next_word: the 64-bit extension of both states gives the 32 sequence bits and the states 32 bits on).
 * One g_prs_jump per translation unit that includes this header.
 */
#pragma once

#include "ldpc_device_util.h"

namespace ldpc_hip {
namespace {

__device__ const prs_jump_table g_prs_jump = prs_make_jump_table();

template <bool X2>
__device__ __forceinline__ uint32_t prs_jump_dev(uint32_t s, uint32_t p)
{
  const uint64_t v = prs_extend<X2>(s);
  uint32_t       r = 0;
#pragma unroll
  for (int k = 0; k != 31; ++k) {
    r ^= static_cast<uint32_t>(v >> k) & (0U - ((p >> k) & 1U));
  }
  return r & PRS_MASK;
}

/* (x1, x2) advanced by j sequence words */
__device__ __forceinline__ void prs_jump_words(uint32_t& x1, uint32_t& x2, uint32_t j)
{
  for (int m = 0; m != PRS_JUMP_DIGITS && (j >> (5 * m)) != 0U; ++m) {
    const uint32_t d = (j >> (5 * m)) & 31U;
    if (d != 0U) {
      x1 = prs_jump_dev<false>(x1, g_prs_jump.p[0][m][d]);
      x2 = prs_jump_dev<true>(x2, g_prs_jump.p[1][m][d]);
    }
  }
}

/* the 32 sequence bits at the states (bit i = c(n0 + i)); the states move 32 bits on */
__device__ __forceinline__ uint32_t prs_next_word(uint32_t& x1, uint32_t& x2)
{
  const uint64_t v1 = prs_extend<false>(x1), v2 = prs_extend<true>(x2);
  x1                = static_cast<uint32_t>(v1 >> 32) & PRS_MASK;
  x2                = static_cast<uint32_t>(v2 >> 32) & PRS_MASK;
  return static_cast<uint32_t>(v1) ^ static_cast<uint32_t>(v2);
}

} // namespace
} // namespace ldpc_hip
