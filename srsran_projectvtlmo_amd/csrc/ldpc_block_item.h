/*
 * The segment launches' block lookup on the device: a launch's work items lie in block order, each with the launch's
 * block count before it (block0, ldpc_hip_descs.h), and a workgroup finds its own by blockIdx.x. Shared by the kernels
 * of the demodulator, the sequence generator, the modulation mapper, the equalizer, the precoder and the DM-RS
 * generator; nothing of the decoder or of any of these stages is declared here.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_hip {

/* this block's item: the last one with block0(item) <= blockIdx.x (n >= 1 items in block order, the first at 0) */
template <typename T, typename F>
__device__ __forceinline__ uint32_t block_item(const T* __restrict__ items, uint32_t n, F block0)
{
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (block0(items[mid]) <= blockIdx.x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

/* the same for items with a block0 member */
template <typename T>
__device__ __forceinline__ uint32_t block_item(const T* __restrict__ items, uint32_t n)
{
  return block_item(items, n, [](const T& s) { return s.block0; });
}

} // namespace ldpc_hip
