/*
 * The host launchers of the kernel units, declared once: ldpc_hip_kernels.hip (with ldpc_uplink_kernels.h),
 * ldpc_downlink_kernels.hip and ldpc_spec_unit.hip define them
 * and the host runtime calls them, all through this header, so a signature or default argument cannot drift.
 * (spec_waves, quad_table_offset and the other schedule queries of ldpc_graph.cpp are in ldpc_graph.h.)
 */
#pragma once

#include <hip/hip_runtime.h>

#include "ldpc_graph.h"
#include "ldpc_spec.h"

namespace ldpc_hip {

/* ---- ldpc_hip_kernels.hip and the uplink family it includes; ldpc_downlink_kernels.hip: upload_encoder_graphs (called
 * by upload_graphs), launch_encode, launch_rate_match, launch_pdsch_encode, dwq_kernel_encode, dwq_kernel_copy ---- */
hipError_t upload_graphs(const graph_desc* graphs, int n);
hipError_t upload_encoder_graphs(const graph_desc* graphs, int n);
hipError_t configure_kernels(uint32_t max_lds);
hipError_t write_split_tables(uint32_t* d_tables, const int* spec_ids, hipStream_t stream);
/* host_one / host_dm_one: a one-CB launch's descriptors by value; d_dm: the fused dematcher's, dm_lds its LDS budget */
hipError_t launch_decode(bool sf08, int spec, const dec_cb* d_cbs, uint32_t n, int graph_slot,
                         const step_task* tasks, const lds_layout& lay, int block, const int8_t* llr, uint8_t* out,
                         ldpc_hip_cb_result* res, const uint32_t* d_crc, hipStream_t stream,
                         const dec_cb* host_one = nullptr, const dematch_cb* d_dm = nullptr,
                         const dematch_cb* host_dm_one = nullptr, uint32_t dm_lds = 0);
hipError_t launch_decode_mixed(bool sf08, const dec_cb* d_cbs, uint32_t n, const mixed_group* d_groups,
                               uint32_t ngroups, uint32_t lds_bytes, const step_task* tasks, const int8_t* llr,
                               uint8_t* out, ldpc_hip_cb_result* res, const uint32_t* d_crc, hipStream_t stream,
                               const dematch_cb* d_dm = nullptr, uint32_t dm_lds = 0);
hipError_t launch_encode(const enc_cb* d_cbs, uint32_t n, const uint8_t* msg, uint8_t* cw, const uint32_t* d_crc,
                         hipStream_t stream);
hipError_t launch_rate_match(const ratematch_cb* d_cbs, uint32_t n, const uint8_t* cw, uint8_t* out,
                             hipStream_t stream);
hipError_t launch_pdsch_encode(const pdsch_enc_cb* d_cbs, const pdsch_enc_cb* host_one, uint32_t n,
                               const uint8_t* msg, uint8_t* out, const uint32_t* d_crc, hipStream_t stream);
hipError_t launch_tb_join(const tbj_block* d_blocks, uint32_t nblocks, const uint8_t* msgs, ldpc_hip_cb_result* cb,
                          uint8_t* tb, ldpc_hip_tb_result* res, const uint32_t* d_crc, uint32_t* d_work,
                          hipStream_t stream);
hipError_t launch_dematch(const dematch_cb* d_cbs, uint32_t n, const demod_tables& tab, hipStream_t stream,
                          const dematch_cb* host_one = nullptr);
hipError_t launch_demodulate(const demod_seg* d_segs, uint32_t nseg, uint32_t nblocks, const demod_tables& tab,
                             const float* d_sym, const float* d_nv, int8_t* d_llr, hipStream_t stream);
hipError_t launch_prs(const prs_seg* d_segs, uint32_t nseg, uint32_t nblocks, bool bits, const uint8_t* d_in,
                      uint8_t* d_out, hipStream_t stream);
/* ---- ldpc_modulation_kernels.hip: the modulation mapper, stand-alone and behind the rate matcher; ci8: int8 (re, im)
 * pairs, else float pairs; nblocks as the items' block0 count them ---- */
hipError_t launch_modulate(const mod_seg* d_segs, uint32_t nseg, uint32_t nblocks, bool ci8, const uint8_t* d_bits,
                           void* d_sym, hipStream_t stream);
hipError_t launch_rate_match_modulate(const rm_mod_cb* d_cbs, uint32_t ncb, uint32_t nblocks, bool ci8,
                                      const uint8_t* d_cws, void* d_sym, hipStream_t stream);
/* the persistent work-queue kernels that are not per graph (ldpc_hip_dwq.cpp) */
const void* dwq_kernel_dematch();
const void* dwq_kernel_encode();
const void* dwq_kernel_copy();

/* ---- every kernel unit (ldpc_spec.h LDPC_KERNEL_UNITS: core is ldpc_hip_kernels.hip, a..p are ldpc_spec_unit.hip
 * compiled per letter, spec_unit() 1..16): the host launch stubs of its specialised kernels and split-row table
 * writers, and the work-queue kernel of specialised graph id (nullptr when the unit does not hold it) ---- */
#define LDPC_SPEC_KERNEL_DECL(id, bg, z, ils) const void* spec_kernel_##id(); const void* spec_split_kernel_##id();
LDPC_SPEC_GRAPHS_UNITS(LDPC_SPEC_KERNEL_DECL)
#undef LDPC_SPEC_KERNEL_DECL
#define LDPC_DWQ_UNIT_DECL(u, x) const void* dwq_kernel_##u(int id);
LDPC_KERNEL_UNITS(LDPC_DWQ_UNIT_DECL)
#undef LDPC_DWQ_UNIT_DECL

} // namespace ldpc_hip
