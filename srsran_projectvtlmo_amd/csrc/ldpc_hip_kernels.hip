/*
 * The decode code object: the generic and mixed decode kernels, the core specialised kernels (the mixed kernel's
 * bodies; ldpc_spec_unit.hip instantiates the rest) and their work-queue kernels, this object's graph table and the
 * host launchers of every decode kernel, and, included at the end, the uplink kernel family (ldpc_uplink_kernels.h:
 * rate dematcher, TB join, demodulator, descrambler), which needs nothing of the decoder. The uplink family shares
 * this code object on purpose: a slot's kernels are launched back to back (decode, then TB join), and launched from
 * two code objects they took 0.8 us per C4 slot longer than from one (profiles/r09/ab_kernel_units.txt). The downlink
 * family, which no decode launch follows, is a code object of its own (ldpc_downlink_kernels.hip).
 */
#include <algorithm>
#include <vector>

#define LDPC_SPEC_TU_GRAPHS LDPC_SPEC_GRAPHS_CORE
#include "ldpc_decode_cb.h"
#include "ldpc_hip_launch.h"

namespace ldpc_hip {

/* Several (BG, Z) groups of one plan in ONE launch of 768-thread workgroups (a mixed slot: the large TB's BG1 Z=384
 * CBs on the specialised body beside the small TBs' BG2 CBs on the generic one). Workgroup b decodes CB b of the
 * plan's group-sorted order; its group is the last one with first_block <= b. Used when the whole plan fits the
 * device at once, so one launch replaces a fork/join of per-group launches and their event waits. */
template <bool SF08>
__global__ void __launch_bounds__(768)
    ldpc_decode_mixed_kernel(const dec_cb* __restrict__ cbs, const mixed_group* __restrict__ groups, uint32_t ngroups,
                             const step_task* __restrict__ tasks, const int8_t* llr_base, /* see ldpc_decode_kernel */
                             uint8_t* __restrict__ out_base, ldpc_hip_cb_result* __restrict__ res_base,
                             const uint32_t* __restrict__ crc_tables, const dematch_cb* __restrict__ dm_cbs)
{
  const dematch_cb dm_none{}; /* fused dematcher: dm_cbs[block], or none */
  uint32_t lo = 0, hi = ngroups;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (groups[mid].first_block <= blockIdx.x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const mixed_group g = groups[lo];
  if constexpr (SF08) {
    bool done = false; /* g.spec: specialised kernel id + 1 (a workgroup-uniform branch) */
    sp::static_for<spec::NOF_CORE_SPECS>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      if (g.spec == static_cast<uint32_t>(i + 1)) {
        decode_cb<true, i>(cbs[blockIdx.x], g.graph_slot, tasks + g.task_offset, g.lay, llr_base, out_base, res_base,
                           crc_tables, dm_cbs, dm_none);
        done = true;
      }
    });
    if (done) {
      return;
    }
  }
  decode_cb<SF08, -1>(cbs[blockIdx.x], g.graph_slot, tasks + g.task_offset, g.lay, llr_base, out_base, res_base,
                      crc_tables, dm_cbs, dm_none);
}

/* the persistent work-queue kernels (ldpc_hip_dwq.cpp) of the core graphs */
LDPC_DWQ_KERNELS(dwq_kernel_core, LDPC_SPEC_GRAPHS_CORE)

/* ---- host-side launch helpers (ldpc_hip_launch.h) ---- */

/* host launch stub of specialised kernel `id` (core: this unit; the others: ldpc_spec_unit.hip) */
const void* spec_kernel_ptr(int id)
{
#define LDPC_SPEC_KERNEL(id, bg, z, ils) reinterpret_cast<const void*>(&ldpc_decode_kernel<true, id>),
#define LDPC_SPEC_KERNEL_EXT(id, bg, z, ils) spec_kernel_##id(),
  static const void* const spec_kernels[] = {
      LDPC_SPEC_GRAPHS_CORE(LDPC_SPEC_KERNEL) LDPC_SPEC_GRAPHS_UNITS(LDPC_SPEC_KERNEL_EXT)};
#undef LDPC_SPEC_KERNEL
#undef LDPC_SPEC_KERNEL_EXT
  static_assert(sizeof(spec_kernels) / sizeof(spec_kernels[0]) == spec::NOF_SPECS, "specialised kernel table");
  return (id >= 0 && id < spec::NOF_SPECS) ? spec_kernels[id] : nullptr;
}

/* host launch stub of the split-row address table writer of specialised graph `id` */
const void* spec_split_kernel_ptr(int id)
{
#define LDPC_SPEC_KERNEL(id, bg, z, ils) reinterpret_cast<const void*>(&ldpc_split_table_kernel<id>),
#define LDPC_SPEC_KERNEL_EXT(id, bg, z, ils) spec_split_kernel_##id(),
  static const void* const split_kernels[] = {
      LDPC_SPEC_GRAPHS_CORE(LDPC_SPEC_KERNEL) LDPC_SPEC_GRAPHS_UNITS(LDPC_SPEC_KERNEL_EXT)};
#undef LDPC_SPEC_KERNEL
#undef LDPC_SPEC_KERNEL_EXT
  static_assert(sizeof(split_kernels) / sizeof(split_kernels[0]) == spec::NOF_SPECS, "split table writer table");
  return (id >= 0 && id < spec::NOF_SPECS) ? split_kernels[id] : nullptr;
}

/* The split-row address tables of every specialised BG1 graph into the context's table buffer (d_tables), one
 * workgroup per graph; spec_ids[p] = the specialised id of BG1 lifting size p, or -1. Synchronous (context open). */
hipError_t write_split_tables(uint32_t* d_tables, const int* spec_ids, hipStream_t stream)
{
  /* the one-wave graphs' lane-split address tables (their graphs have no split-row table) */
  for (int id = 0; id != spec::NOF_SPECS; ++id) {
    const long off = quad_table_offset(id);
    if (off < 0) {
      continue;
    }
    auto* k = reinterpret_cast<void (*)(uint32_t*)>(const_cast<void*>(spec_split_kernel_ptr(id)));
    hipLaunchKernelGGL(k, dim3(1), dim3(64 * spec_waves(id)), 0, stream, d_tables + off);
    if (hipGetLastError() != hipSuccess) {
      return hipErrorLaunchFailure;
    }
  }
  for (int p = 0; p != 51; ++p) {
    if (spec_ids[p] < 0 || quad_table_offset(spec_ids[p]) >= 0) {
      continue;
    }
    auto* k = reinterpret_cast<void (*)(uint32_t*)>(const_cast<void*>(spec_split_kernel_ptr(spec_ids[p])));
    hipLaunchKernelGGL(k, dim3(1), dim3(64 * spec_waves(spec_ids[p])), 0, stream,
                       d_tables + SPLIT_TAB_OFFSET + p * SPLIT_TAB_STRIDE);
    if (hipGetLastError() != hipSuccess) {
      return hipErrorLaunchFailure;
    }
  }
  return hipStreamSynchronize(stream);
}

hipError_t launch_decode(bool sf08, int spec, const dec_cb* d_cbs, uint32_t n, int graph_slot,
                         const step_task* tasks, const lds_layout& lay, int block, const int8_t* llr, uint8_t* out,
                         ldpc_hip_cb_result* res, const uint32_t* d_crc, hipStream_t stream, const dec_cb* host_one,
                         const dematch_cb* d_dm, const dematch_cb* host_dm_one, uint32_t dm_lds)
{
  if (n == 0) {
    return hipSuccess;
  }
  /* one CB with its descriptor on the host: passed by value, the kernel reads no descriptor table */
  const bool   inl = host_one != nullptr && n == 1;
  const dec_cb one = inl ? *host_one : dec_cb{};
  /* fused dematcher (d_dm or, one CB, its descriptor by value): its staging (and tables) need dm_lds
   * (dm_fused_budget; 0: DM_FUSED_LDS) */
  const bool       dm_inl = host_dm_one != nullptr && n == 1;
  const bool       fused  = d_dm != nullptr || dm_inl;
  const dematch_cb dm_one = dm_inl ? *host_dm_one : dematch_cb{};
  const uint32_t   lds    = fused ? std::max(lay.total, dm_lds != 0 ? dm_lds : DM_FUSED_LDS) : lay.total;
  using kernel_fn = void (*)(const dec_cb*, dec_cb, int, const step_task*, lds_layout, const int8_t*, uint8_t*,
                             ldpc_hip_cb_result*, const uint32_t*, const dematch_cb*, dematch_cb);
  if (spec >= spec::NOF_SPECS || (spec >= 0 && (block != 64 * spec_waves(spec) || !sf08))) {
    return hipErrorInvalidValue; /* a specialised kernel: its own wave count, scaling factor 0.8 */
  }
  kernel_fn k = spec >= 0 ? reinterpret_cast<kernel_fn>(const_cast<void*>(spec_kernel_ptr(spec)))
                          : (sf08 ? &ldpc_decode_kernel<true, -1> : &ldpc_decode_kernel<false, -1>);
  hipLaunchKernelGGL(k, dim3(n), dim3(block), lds, stream, inl ? nullptr : d_cbs, one, graph_slot, tasks, lay, llr,
                     out, res, d_crc, dm_inl ? nullptr : d_dm, dm_one);
  return hipGetLastError();
}

hipError_t launch_decode_mixed(bool sf08, const dec_cb* d_cbs, uint32_t n, const mixed_group* d_groups,
                               uint32_t ngroups, uint32_t lds_bytes, const step_task* tasks, const int8_t* llr,
                               uint8_t* out, ldpc_hip_cb_result* res, const uint32_t* d_crc, hipStream_t stream,
                               const dematch_cb* d_dm, uint32_t dm_lds)
{
  if (n == 0) {
    return hipSuccess;
  }
  auto* k = sf08 ? &ldpc_decode_mixed_kernel<true> : &ldpc_decode_mixed_kernel<false>;
  hipLaunchKernelGGL(k, dim3(n), dim3(MIXED_BLOCK),
                     d_dm != nullptr ? std::max(lds_bytes, dm_lds != 0 ? dm_lds : DM_FUSED_LDS) : lds_bytes,
                     stream, d_cbs, d_groups, ngroups, tasks, llr, out, res, d_crc, d_dm);
  return hipGetLastError();
}

hipError_t upload_graphs(const graph_desc* graphs, int n)
{
  /* c_graphs is a static __constant__ per code object: this one's copy, then the downlink unit's (the encoder's) */
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_graphs), graphs, sizeof(graph_desc) * static_cast<size_t>(n));
  return e != hipSuccess ? e : upload_encoder_graphs(graphs, n);
}

LDPC_DIAG_READERS /* diagnostic builds: ldpc_hip_diag_read, ldpc_hip_diag2_read (ldpc_diag.h) */

hipError_t configure_kernels(uint32_t max_lds)
{
  std::vector<const void*> ks = {reinterpret_cast<const void*>(&ldpc_decode_kernel<true, -1>),
                                 reinterpret_cast<const void*>(&ldpc_decode_kernel<false, -1>),
                                 reinterpret_cast<const void*>(&ldpc_decode_mixed_kernel<true>),
                                 reinterpret_cast<const void*>(&ldpc_decode_mixed_kernel<false>)};
  for (int id = 0; id != spec::NOF_SPECS; ++id) {
    ks.push_back(spec_kernel_ptr(id));
  }
  for (const void* k : ks) {
    const hipError_t e =
        hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(max_lds));
    if (e != hipSuccess) {
      return e;
    }
  }
  return hipSuccess;
}

} // namespace ldpc_hip

#include "ldpc_uplink_kernels.h"
