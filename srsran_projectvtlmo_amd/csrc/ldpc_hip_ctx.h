/*
 * The host runtime's shared state behind the C ABI of include/srsran_ldpc_hip.h: the context, decode plans, the HAL
 * queue's operations and the external HARQ repository, with the functions its units call across each other:
 * ldpc_hip_api.cpp (context, plans, *_launch entry points), ldpc_hip_sync.cpp (synchronous entry points),
 * ldpc_hip_modulate.cpp (modulation mapper), ldpc_hip_equalize.cpp (channel equalizer), ldpc_hip_precode.cpp
 * (precoder), ldpc_hip_dmrs.cpp (PDSCH DM-RS), ldpc_hip_chest.cpp (PUSCH DM-RS channel estimator), ldpc_hip_hal.cpp
 * (HAL decoder queue), ldpc_hip_enc_queue.cpp (PDSCH encoder queue) and ldpc_hip_descs.cpp (descriptor translations,
 * the precoder's, the DM-RS generator's and the channel estimator's tables among them, host only). The segment stages
 * share the two tails here: launch_items (work items up, one launch) and sync_round_trip (a *_sync call's host buffers
 * through the scratch).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "ldpc_hip_buffers.h"
#include "ldpc_hip_descs.h"
#include "ldpc_hip_dwq.h"

/* One operation of the HAL batch (hw_accelerator_pusch_dec configure + enqueue). */
struct hal_op {
  uint32_t              cb_index = 0;
  ldpc_hip_hw_config    cfg{};
  ldpc_hip_dematch_desc dm{};          /* the operation's rate dematching (cb_length = 66Z / 50Z), validated at enqueue */
  uint32_t              msg_bytes = 0;
  uint64_t              llr_off   = 0; /* in the LLR staging arena (h_llr / q_llr)                    */
  uint64_t              soft_off  = 0; /* external HARQ: in the arena; otherwise in h_soft / q_soft    */
  uint64_t              out_off   = 0; /* in the message arena (h_out / q_out)                         */
  uint32_t              pos       = 0; /* decode position in the launched batch (result index)          */
  ldpc_hip::dwq*        q         = nullptr; /* the work queue running this op (a work-queue batch), else null */
  uint32_t              ticket    = 0;
  bool                  dropped   = false;
  bool                  dequeued  = false;
  ldpc_hip_cb_result    res{};
};

/* failed: a launch failed after work was queued; the batch cannot be relaunched (its dematch may already have combined
 * into the HARQ soft buffers) and reads as an error until the queue is reserved or freed again. */
enum class hal_state { idle, staging, launched, failed };

/* The external HARQ buffer repository (ext_harq_buffer_context_repository.h:44-96) and the HBM it describes. One
 * atomic word per entry: bit 31 = entry in use (not empty), bits 0-30 = soft-data length.
 * caller_state (ldpc_hip_harq_device_memory): the device's HARQ memory only -- the caller keeps the entry state in its
 * own ext_harq_buffer_context_repository and decides drops (acc100's split: the repository holds the metadata, the
 * accelerator's HARQ memory the soft bits, bbdev_ldpc_decoder.cpp:146); then there is no state array and the arena
 * grows on demand (grow), under arena_mu: launches read the arena pointer under a shared lock, a growth takes it
 * exclusively and waits for the device before it moves the soft bits. */
struct ldpc_hip_harq_repo {
  static constexpr uint32_t IN_USE = 0x80000000U;
  static constexpr uint32_t MAX_CODEBLOCKS = 1U << 20;
  int                                      device         = 0;
  uint32_t                                 nof_codeblocks = 0;
  bool                                     debug_mode     = false;
  bool                                     caller_state   = false;
  ldpc_hip::dev_buffer                     arena; /* nof_codeblocks x LDPC_HIP_HARQ_STRIDE int8 */
  std::unique_ptr<std::atomic<uint32_t>[]> state;
  std::atomic<int>                         refs{1};
  std::shared_mutex                        arena_mu;
  /* What may still use the arena's address after a batch has been issued: the work-queue items of HAL batches (a grid
   * may claim one after its batch's arena lock is gone), and the launch-path batches of every context attached to the
   * arena (each records its done event after its batch). grow() waits for exactly these, not for the whole device (a
   * hipDeviceSynchronize also waited for the persistent work-queue grids, up to their 50 ms lifetime). */
  std::mutex                                       inflight_mu;
  std::vector<std::pair<ldpc_hip::dwq*, uint32_t>> inflight;
  std::vector<hipEvent_t>                          user_events;

  void track_item(ldpc_hip::dwq* q, uint32_t ticket)
  {
    std::lock_guard<std::mutex> lock(inflight_mu);
    inflight.erase(std::remove_if(inflight.begin(), inflight.end(),
                                  [](const std::pair<ldpc_hip::dwq*, uint32_t>& it) {
                                    return ldpc_hip::dwq_done(it.first, it.second);
                                  }),
                   inflight.end());
    inflight.emplace_back(q, ticket);
  }
  void add_user(hipEvent_t ev)
  {
    std::lock_guard<std::mutex> lock(inflight_mu);
    user_events.push_back(ev);
  }
  void remove_user(hipEvent_t ev)
  {
    std::lock_guard<std::mutex> lock(inflight_mu);
    user_events.erase(std::remove(user_events.begin(), user_events.end(), ev), user_events.end());
  }
  /* with arena_mu held exclusively (no batch can be issued): every issued user of the arena has finished */
  hipError_t wait_users();

  int8_t* entry(uint32_t id) const { return arena.as<int8_t>() + static_cast<size_t>(id) * LDPC_HIP_HARQ_STRIDE; }
  /* caller_state memory: makes absolute_cb_id addressable (doubling, at least to the next multiple of 1024 entries).
   * Waits for every issued user of the arena first (wait_users): a batch already issued holds the old address. */
  hipError_t grow(uint32_t id);
  /* get(absolute_codeblock_id, new_data), :69-83: a fresh entry (soft-data length 0) on new data or when empty;
   * returns the entry's soft-data length. */
  uint32_t get(uint32_t id, bool new_data)
  {
    uint32_t s = state[id].load(std::memory_order_acquire);
    if ((s & IN_USE) == 0 || new_data) {
      s = IN_USE;
      state[id].store(s, std::memory_order_release);
    }
    return s & ~IN_USE;
  }
  /* the soft-data length a completed decode leaves (acc100 reads it back at dequeue, acc100_impl.cpp:206-207) */
  void set_len(uint32_t id, uint32_t len) { state[id].store(IN_USE | len, std::memory_order_release); }
  /* free(absolute_codeblock_id), :86-96: kept in debug mode */
  void free(uint32_t id)
  {
    if (!debug_mode) {
      state[id].store(0U, std::memory_order_release);
    }
  }
  void release();
};

namespace ldpc_hip {

/* The device copy of a *_launch entry point's work items, with what was last uploaded into it. A slot pipeline
 * relaunches the same descriptors slot after slot, and a host-to-device copy from pageable memory is performed
 * synchronously by HIP (the host waits for the stream), so an upload equal to the previous one into the same
 * allocation, on the same stream, is skipped; any other is refused while the stream is capturing. */
struct desc_table {
  hipError_t upload(const void* src, size_t n, hipStream_t s);
  template <typename T>
  const T* as() const { return buf.as<const T>(); }
private:
  dev_buffer           buf;
  std::vector<uint8_t> last; /* the bytes in buf[0, last.size()), copied there on last_stream at address last_ptr */
  void*                last_ptr    = nullptr;
  hipStream_t          last_stream = nullptr;
};

/* The HIP stream an entry point's `stream` argument names: NULL the context's own stream; hipStreamLegacy
 * ((hipStream_t)1, the legacy default stream) the null stream, which is that stream to every runtime call; any other
 * handle (a stream, or hipStreamPerThread, which the runtime resolves itself) as given. Round 4 passed hipStreamLegacy
 * through unchanged, and a multi-group plan's fork (hipEventRecord / hipStreamWaitEvent on it) crashed in the runtime
 * (tools/ubench/stream_probe.hip). */
inline hipStream_t abi_stream(hipStream_t ctx_stream, void* stream)
{
  if (stream == nullptr) {
    return ctx_stream;
  }
  if (static_cast<hipStream_t>(stream) == hipStreamLegacy) {
    return nullptr;
  }
  return static_cast<hipStream_t>(stream);
}

/* One copy of a *_sync call's round trip (sync_round_trip): `bytes` between host memory and buf + offset. */
struct sync_copy {
  dev_buffer* buf;
  size_t      offset, bytes;
  const void* from; /* host memory copied to the device before the stage runs, or null */
  void*       to;   /* host memory the device's bytes are copied to after it, or null */
};
inline sync_copy to_device(dev_buffer& buf, size_t offset, const void* host, size_t bytes)
{
  return {&buf, offset, bytes, host, nullptr};
}
inline sync_copy to_host(dev_buffer& buf, size_t offset, void* host, size_t bytes)
{
  return {&buf, offset, bytes, nullptr, host};
}

} // namespace ldpc_hip

struct ldpc_hip_plan;

struct ldpc_hip_ctx {
  int                               device = 0;
  hipStream_t                       stream = nullptr;
  hipEvent_t                        done_event = nullptr;
  std::string                       err;
  std::vector<ldpc_hip::graph_desc> graphs; /* host copy, NOF_GRAPH_SLOTS entries: wide (BG1 then BG2, by lifting
                                               position), then the narrow schedules (NARROW_SLOT_BASE + slot) */
  int                     n_cu = 256;  /* compute units of the device */
  std::vector<uint8_t>    narrow_fits2 = std::vector<uint8_t>(102, 0); /* narrow schedule runs two CBs per CU */
  std::vector<uint8_t>    graph_valid;
  std::vector<uint8_t>    graph_spec; /* id + 1 of the specialised kernel (ldpc_spec.h) for this graph, 0: none */
  ldpc_hip::dev_buffer    d_crc;
  ldpc_hip::dev_buffer    d_tasks; /* step_task records of all graphs (ldpc_graph.cpp build_tasks) */
  /* the *_launch entry points' work items on the device (launch_items) */
  ldpc_hip::desc_table    d_dmdesc;  /* ldpc_hip_rate_dematch_launch descriptors */
  ldpc_hip::desc_table    d_encdesc; /* ldpc_hip_encode_launch descriptors */
  ldpc_hip::desc_table    d_rmdesc;  /* ldpc_hip_rate_match_launch descriptors */
  ldpc_hip::desc_table    d_dmsegs;  /* ldpc_hip_demodulate_launch segments */
  ldpc_hip::desc_table    d_prssegs; /* ldpc_hip_descramble_launch / ldpc_hip_scramble_bits_launch segments */
  ldpc_hip::desc_table    d_modsegs; /* ldpc_hip_modulate_launch segments */
  ldpc_hip::desc_table    d_rmmod;   /* ldpc_hip_rate_match_modulate_launch codeblocks */
  ldpc_hip::desc_table    d_eqsegs;  /* ldpc_hip_equalize_launch segments */
  ldpc_hip::desc_table    d_precode; /* ldpc_hip_precode_map_launch / _sync: make_precode_table's blob, as bytes */
  ldpc_hip::desc_table    d_dmrs;    /* ldpc_hip_dmrs_pdsch_map_launch: make_dmrs_table's blob, as bytes */
  ldpc_hip::desc_table    d_chest;   /* ldpc_hip_dmrs_pusch_estimate_launch: make_chest_table's blob, as bytes */
  ldpc_hip::desc_table    d_tbaux;   /* ldpc_hip_tb_join_launch: its TB's descriptor, TB and chunk per workgroup */
  ldpc_hip::dev_buffer    d_tbwork;  /* ldpc_hip_tb_join_launch: per-TB chunk CRCs + arrival counter (zero at rest) */
  ldpc_hip::demod_tables  dtab{};    /* demodulator slopes / intercepts (make_demod_tables) */
  ldpc_hip_params         params{};
  /* fork/join of multi-group decode plans: groups after the first run on auxiliary streams (created on first use) */
  std::vector<hipStream_t> aux_streams;
  std::vector<hipEvent_t>  aux_events; /* [0]: fork point, [1 + i]: auxiliary stream i done */

  /* scratch for the synchronous entry points */
  ldpc_hip::dev_buffer d_llr, d_out, d_res, d_soft, d_desc, d_sym, d_nv;
  /* the one-codeblock software route (ldpc_decoder_hip::decode / ldpc_rate_dematcher_hip::rate_dematch, one call per
   * CB): pinned staging the kernel reads and writes in place (zero-copy), an event the caller spins on */
  ldpc_hip::pinned_buffer s_in, s_out;
  /* the one-CB decode's LLRs in device memory the host writes through the BAR (ldpc_hip_buffers.h bar_buffer), so the
   * kernel reads HBM; s_in serves when it cannot be had (bar_failed: not asked again) */
  ldpc_hip::bar_buffer s_bar;
  bool                 bar_failed = false;
  /* a one-CB work-queue wait timed out while the queue's grid stayed resident: it may still write s_in / s_out, so the
   * one-CB calls of this context refuse from then on (the context is to be closed) */
  bool       staging_lost = false;
  hipEvent_t sync_event   = nullptr;
  bool       sync_zc      = true; /* LDPC_HIP_SYNC_ZERO_COPY=0 (environment): the copy path, for A/B timing */
  /* the device work queues (ldpc_hip_dwq.h): workgroup size and body LDS of every queue key's persistent kernel */
  int                  key_block[ldpc_hip::DWQ_KEYS] = {};
  uint32_t             key_lds[ldpc_hip::DWQ_KEYS]   = {};
  bool                 use_dwq                       = false;
  ldpc_hip::lds_layout spec_lay[102] = {}; /* the specialised layout of each graph with a specialised body */

  /* HAL queue (ldpc_hip_enqueue / ldpc_hip_dequeue): staged operations of the current batch in pinned host memory,
   * moved with one copy per direction per batch */
  hal_state               hstate = hal_state::idle;
  std::vector<hal_op>     hops;  /* operations of the current batch, in enqueue order */
  std::vector<int32_t>    hslot; /* cb_index -> index in hops, -1 when absent          */
  uint32_t                hdequeued = 0;
  ldpc_hip::pinned_buffer h_llr, h_soft, h_out; /* h_llr: LLRs then descriptors; h_out: messages then results */
  ldpc_hip::dev_buffer    q_llr, q_soft, q_out;
  uint64_t                h_llr_used = 0, h_soft_used = 0, h_out_used = 0, h_res_off = 0;
  /* early copy (LDPC_HIP_LAUNCH_HAL_NO_EARLY_COPY off): h_llr[0, h_llr_copied) is already queued for q_llr on
   * hq_stream; hcopy: the current batch stages this way */
  uint64_t h_llr_copied = 0;
  bool     hcopy        = false;
  /* the early copy through the copy work queue (hal_copy_staged): its queue for this batch and its items' tickets */
  ldpc_hip::dwq*        hcopy_q = nullptr;
  std::vector<uint32_t> hcopy_tickets;
  ldpc_hip_plan*        hplan = nullptr; /* the batch's decode plan (descriptors in q_llr after the LLRs); owned, see close */

  /* external HARQ: the repository this context's HAL queue keeps its soft buffers in (one reference held) */
  ldpc_hip_harq_repo* repo = nullptr;
  /* the HAL queue's stream: the context stream (dedicated queue), or one of the device's shared queues between
   * ldpc_hip_queue_reserve and ldpc_hip_queue_free (LDPC_HIP_LAUNCH_SHARED_QUEUE) */
  hipStream_t hq_stream = nullptr;
  int         hq_shared = -1; /* index of the borrowed shared queue, -1: none */
  bool        hbatch_done = false; /* the launched batch's event has been seen complete (later dequeues skip the query) */

  int fail(int code, const std::string& msg)
  {
    err = msg;
    return code;
  }
  int hip_fail(hipError_t e, const std::string& where)
  {
    err = where + ": " + hipGetErrorString(e);
    return LDPC_HIP_EDEVICE;
  }
  /* The tail of a *_launch entry point: the work items into their table on stream s, then launch(the device items);
   * a HIP error of either is reported as `what`. No item (every segment empty): nothing touches the device. */
  template <typename T, typename Launch>
  int launch_items(ldpc_hip::desc_table& table, const std::vector<T>& items, hipStream_t s, const char* what,
                   Launch&& launch)
  {
    if (items.empty()) {
      return LDPC_HIP_OK;
    }
    hipError_t e = table.upload(items.data(), items.size() * sizeof(T), s);
    if (e == hipSuccess) {
      e = launch(table.as<T>());
    }
    return e == hipSuccess ? LDPC_HIP_OK : hip_fail(e, what);
  }
  /* The host round trip of a stage's *_sync entry point, on the context's stream: every copy's scratch buffer reserved
   * (one named more than once for its largest offset + bytes), the to_device copies queued, run() (the stage's segments
   * on the scratch; a code other than LDPC_HIP_OK is returned as it is), the to_host copies queued, the stream
   * synchronised. `name` is the stage's in the error of a HIP failure, which also says the step. */
  template <typename Run>
  int sync_round_trip(const char* name, std::initializer_list<ldpc_hip::sync_copy> copies, Run&& run)
  {
    hipError_t e = hipSuccess;
    for (const ldpc_hip::sync_copy& c : copies) {
      size_t need = 0;
      for (const ldpc_hip::sync_copy& o : copies) {
        need = o.buf == c.buf ? std::max(need, o.offset + o.bytes) : need;
      }
      if ((e = c.buf->reserve(need)) != hipSuccess) {
        return hip_fail(e, std::string("hipMalloc(") + name + ")");
      }
    }
    for (const ldpc_hip::sync_copy& c : copies) {
      if (c.from != nullptr && (e = hipMemcpyAsync(c.buf->as<uint8_t>() + c.offset, c.from, c.bytes,
                                                   hipMemcpyHostToDevice, stream)) != hipSuccess) {
        return hip_fail(e, std::string("hipMemcpyAsync(") + name + " in)");
      }
    }
    const int r = run();
    if (r != LDPC_HIP_OK) {
      return r;
    }
    for (const ldpc_hip::sync_copy& c : copies) {
      if (c.to != nullptr && e == hipSuccess) {
        e = hipMemcpyAsync(c.to, c.buf->as<uint8_t>() + c.offset, c.bytes, hipMemcpyDeviceToHost, stream);
      }
    }
    if (e != hipSuccess || (e = hipStreamSynchronize(stream)) != hipSuccess) {
      return hip_fail(e, std::string(name) + "_sync");
    }
    return LDPC_HIP_OK;
  }
};

struct launch_group {
  int                  slot;
  uint32_t             first;
  uint32_t             count;
  ldpc_hip::lds_layout lay;
  int                  block;
  bool                 sf08; /* scaling factor 0.8f: integer scaling path */
};

struct ldpc_hip_plan {
  ldpc_hip_ctx*             ctx = nullptr;
  uint32_t                  n   = 0;
  ldpc_hip::dev_buffer      d_cbs;
  std::vector<launch_group> groups;
  /* mixed launch (ldpc_decode_mixed_kernel): all groups in one launch when the plan fits the device at once */
  bool                 mixed     = false;
  uint32_t             mixed_lds = 0;
  ldpc_hip::dev_buffer d_groups; /* mixed_group per launch group */
  /* the device descriptors launch_plan reads: d_cbs / d_groups, or a caller's buffer (the HAL batch's q_llr) */
  const ldpc_hip::dec_cb*      cbs_dev    = nullptr;
  const ldpc_hip::mixed_group* groups_dev = nullptr;
  /* a one-CB plan built on launch (the HAL batch): the descriptor also on the host, passed by value */
  bool             has_one = false;
  ldpc_hip::dec_cb one{};
  /* the device descriptors in block order on the host (block i decodes caller descriptor h_cbs[i].result_index), and
   * the fused dematcher's descriptors in the same order (ldpc_hip_dematch_decode_launch) */
  std::vector<ldpc_hip::dec_cb> h_cbs;
  ldpc_hip::desc_table          d_dm;
};

namespace ldpc_hip {

/* ---- ldpc_hip_api.cpp ---- */
/* Host part of a decode plan: validates the descriptors, groups the CBs by (BG, Z, scaling path), picks the launch
 * form (specialised / generic, narrow schedules, one mixed launch) and fills the device descriptors `cbs` (group
 * order) and `mg` (mixed launch groups). Nothing touches the device. */
int plan_host(ldpc_hip_ctx* ctx, uint32_t n, const ldpc_hip_dec_desc* descs, ldpc_hip_plan& plan,
              std::vector<dec_cb>& cbs, std::vector<mixed_group>& mg);
/* A plan that owns its device descriptors (ldpc_hip_decode_plan_create, ldpc_hip_decode_sync). */
int build_plan(ldpc_hip_ctx* ctx, uint32_t n, const ldpc_hip_dec_desc* descs, ldpc_hip_plan& plan);
/* d_dm (block order) / dm_one (a one-CB plan's descriptor by value): the fused rate dematcher in front of each CB's
 * decode (ldpc_dematch_body.h), writing the soft buffers the decode then reads; nullptr: decode only. */
int launch_plan(ldpc_hip_plan& plan, const int8_t* d_llr, uint8_t* d_out, ldpc_hip_cb_result* d_res,
                hipStream_t stream, const dematch_cb* d_dm = nullptr, const dematch_cb* dm_one = nullptr,
                uint32_t dm_lds = 0);
/* the segments as work items and the launch, shared by the *_launch and *_sync entry points */
int demodulate_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_demod_desc* descs, const float* d_sym,
                        const float* d_nv, int8_t* d_llr, hipStream_t s);
int prs_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_prs_seg* segs, bool bits, const uint8_t* d_in,
                 uint8_t* d_out, hipStream_t s);

/* ---- ldpc_hip_hal.cpp ---- */
/* Waits for a launched batch (queue_reserve / queue_free / close while operations are in flight). */
void hal_sync(ldpc_hip_ctx* ctx);
/* the HAL queue's borrowed shared stream back to the device's pool */
void release_shared_queue(ldpc_hip_ctx* ctx);

} // namespace ldpc_hip
