/*
 * The HAL decoder queue of the C ABI (include/srsran_ldpc_hip.h): hw_accelerator_pusch_dec semantics
 * (include/srsran/hal/phy/upper/channel_processors/pusch/hw_accelerator_pusch_dec.h:83-115; caller flow
 * pusch_decoder_hw_impl.cpp:132-410) on the context's stream or one of the device's shared queues.
 */
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <thread>

#include "ldpc_hip_ctx.h"
#include "ldpc_hip_launch.h"

using namespace ldpc_hip;

namespace {

/* waits for the batch's early-copy items (they read h_llr and write q_llr); the first error */
hipError_t hal_wait_copies(ldpc_hip_ctx* ctx)
{
  hipError_t r = hipSuccess;
  for (uint32_t t : ctx->hcopy_tickets) {
    const hipError_t e = dwq_wait(ctx->hcopy_q, t);
    r                  = r == hipSuccess ? e : r;
  }
  ctx->hcopy_tickets.clear();
  return r;
}

/* Drops the batch's staged operations (the HARQ arena keeps its entries). */
void hal_reset(ldpc_hip_ctx* ctx, hal_state next)
{
  for (const hal_op& op : ctx->hops) {
    if (op.cb_index < ctx->hslot.size()) {
      ctx->hslot[op.cb_index] = -1;
    }
  }
  ctx->hops.clear();
  ctx->hdequeued    = 0;
  ctx->h_llr_copied = 0;
  ctx->hcopy        = false;
  dwq_unpin(ctx->hcopy_q); /* admitted (pinned) when the batch began */
  ctx->hcopy_q      = nullptr;
  ctx->hcopy_tickets.clear(); /* waited for by hal_sync / the launch */
  ctx->h_llr_used   = 0;
  ctx->h_soft_used = 0;
  ctx->h_out_used  = 0;
  ctx->hstate      = next;
}

/* Zero-copy batches: with the HARQ soft buffers in the HBM arena, a batch whose staged LLRs and descriptors take at
 * most hal_zero_copy_max_bytes() (LDPC_HIP_HAL_ZERO_COPY_MAX, default 4 MiB: C4's 128-CB TB, 1.25 MB of LLRs, first
 * dequeue 92-110 -> 74 us against 256 KiB, profiles/r04/route_ab.json) is read by the kernels straight from the
 * pinned staging buffer, and the decoder writes messages and results straight into the pinned readback buffer: no DMA
 * copy either way, and two fewer dependent operations in the stream (a small TB's latency). Larger batches (a large
 * TB's LLRs) go through one DMA copy each way. */
uint64_t hal_zero_copy_max_bytes()
{
  static const uint64_t v = [] {
    const char* e = std::getenv("LDPC_HIP_HAL_ZERO_COPY_MAX"); /* bytes; A/B timing of the threshold */
    return e != nullptr ? std::strtoull(e, nullptr, 10) : 4ULL * 1024ULL * 1024ULL;
  }();
  return v;
}
/* a zero-copy batch of at most this many codeblocks goes to the device work queue (one item per codeblock; the queue's
 * grid has 32 workgroups by default), a larger one is one launch with a workgroup per codeblock */
constexpr size_t HAL_DWQ_MAX_CBS = 16;

/* Early copy of a large batch's LLRs (LDPC_HIP_LAUNCH_HAL_NO_EARLY_COPY). Round 4's zero-copy launch of C4's 128-CB TB
 * read its 1.25 MB of LLRs from pinned memory over PCIe after the last enqueue (the fused kernel 57.6 us at ~30 GB/s,
 * profiles/r04/hal_kernel_trace.txt). Now each chunk of staged LLRs goes to q_llr by the copy engine while the caller
 * is still enqueueing, and at the first dequeue only the last chunk and the descriptors cross: the kernel reads HBM.
 * Not per-item work-queue traffic (measured slower in round 4, profiles/r04/route_ab_eager_v1.json). */
uint64_t hal_copy_chunk_bytes()
{
  static const uint64_t v = [] {
    const char* e = std::getenv("LDPC_HIP_HAL_COPY_CHUNK"); /* bytes; A/B timing of the chunk size */
    return e != nullptr ? std::max<uint64_t>(4096, std::strtoull(e, nullptr, 10)) : 256ULL * 1024ULL;
  }();
  return v;
}

/* Early copy on (LDPC_HIP_LAUNCH_HAL_EARLY_COPY or LDPC_HIP_HAL_EARLY_COPY=1) by hipMemcpyAsync per chunk: measured
 * slower than the zero-copy read on the GPU box (C4's 128-CB TB 100 -> 123 us, profiles/r05), so it is off by default.
 * The work-queue form (hal_dwq_copy) is the other way to copy early. */
bool hal_early_copy(const ldpc_hip_ctx* ctx)
{
  static const bool env = [] {
    const char* e = std::getenv("LDPC_HIP_HAL_EARLY_COPY");
    return e != nullptr && std::atoi(e) != 0;
  }();
  return (env || (ctx->params.launch_flags & LDPC_HIP_LAUNCH_HAL_EARLY_COPY) != 0) &&
         (ctx->params.launch_flags & LDPC_HIP_LAUNCH_HAL_COPY) == 0;
}

/* Early copy through the copy work queue (LDPC_HIP_HAL_DWQ_COPY=1; needs the work queues): a large batch's
 * staged LLRs go to HBM in 64 KiB items of a resident grid while the caller enqueues (no runtime call per piece), and
 * the batch kernel reads HBM instead of pinned memory over PCIe. */
bool hal_dwq_copy(const ldpc_hip_ctx* ctx)
{
  static const bool env = [] {
    const char* e = std::getenv("LDPC_HIP_HAL_DWQ_COPY");
    return e != nullptr && std::atoi(e) != 0;
  }();
  return env && ctx->use_dwq && (ctx->params.launch_flags & LDPC_HIP_LAUNCH_HAL_COPY) == 0;
}

constexpr uint64_t HAL_COPY_PIECE = 64U * 1024U; /* bytes per copy item */

/* Queues h_llr[h_llr_copied, upto) for q_llr once at least a chunk (force: anything) is staged: as copy items when
 * the batch has a copy queue (hcopy_q; upto a multiple of 16), else on hq_stream. */
hipError_t hal_copy_staged(ldpc_hip_ctx* ctx, bool force, uint64_t upto)
{
  const uint64_t n = upto - ctx->h_llr_copied;
  if (n == 0 || (!force && n < (ctx->hcopy_q != nullptr ? HAL_COPY_PIECE : hal_copy_chunk_bytes()))) {
    return hipSuccess;
  }
  if (upto > ctx->q_llr.size) { /* the device copy moves: what was queued is lost, copy from the start again */
    (void)hal_wait_copies(ctx);
    hipError_t e = hipStreamSynchronize(ctx->hq_stream);
    if (e == hipSuccess) {
      e = ctx->q_llr.reserve(std::max<uint64_t>(upto, 2 * ctx->q_llr.size));
    }
    if (e != hipSuccess) {
      return e;
    }
    ctx->h_llr_copied = 0;
  }
  if (ctx->hcopy_q != nullptr) {
    while (ctx->h_llr_copied < upto) {
      const uint64_t m = std::min<uint64_t>(HAL_COPY_PIECE, upto - ctx->h_llr_copied);
      if (!force && m < HAL_COPY_PIECE) {
        break;
      }
      const dwq_copy_payload pl{ctx->h_llr.dev_as<uint8_t>() + ctx->h_llr_copied,
                                ctx->q_llr.as<uint8_t>() + ctx->h_llr_copied, (m + 15U) / 16U};
      dwq_item it{};
      std::memcpy(static_cast<void*>(&it), &pl, sizeof(pl));
      it.spec           = 1;
      uint32_t   ticket = 0xffffffffU;
      hipError_t e      = dwq_submit(ctx->hcopy_q, it, ticket, false);
      if (ticket != 0xffffffffU) {
        ctx->hcopy_tickets.push_back(ticket);
      }
      if (e != hipSuccess) {
        return e;
      }
      ctx->h_llr_copied += m;
    }
    return hipSuccess;
  }
  const hipError_t e = hipMemcpyAsync(ctx->q_llr.as<uint8_t>() + ctx->h_llr_copied,
                                      ctx->h_llr.as<uint8_t>() + ctx->h_llr_copied, upto - ctx->h_llr_copied,
                                      hipMemcpyHostToDevice, ctx->hq_stream);
  if (e == hipSuccess) {
    ctx->h_llr_copied = upto;
  }
  return e;
}

/* h_llr may move in reserve(): copies still reading the old allocation finish first */
hipError_t hal_reserve_llr(ldpc_hip_ctx* ctx, uint64_t n, uint64_t keep)
{
  if (n > ctx->h_llr.size && ctx->h_llr_copied != 0) {
    (void)hal_wait_copies(ctx);
    const hipError_t e = hipStreamSynchronize(ctx->hq_stream);
    if (e != hipSuccess) {
      return e;
    }
  }
  return ctx->h_llr.reserve(n, keep);
}

/* The first dequeue of a staged batch: one H2D of the staged LLRs (and host soft buffers), one descriptor upload,
 * dematch + decode of the live operations, one D2H of messages, results (and soft buffers), then an event; or, for a
 * zero-copy batch, the two kernels on the pinned buffers alone. */
int hal_launch_issue(ldpc_hip_ctx* ctx, bool& issued)
{
  const bool ext = ctx->repo != nullptr;
  /* the HARQ memory's address stays fixed until this batch is queued (ldpc_hip_harq_repo::grow) */
  std::shared_lock<std::shared_mutex> arena_lock;
  if (ext) {
    arena_lock = std::shared_lock<std::shared_mutex>(ctx->repo->arena_mu);
  }
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i != ctx->hops.size(); ++i) {
    if (!ctx->hops[i].dropped) {
      live.push_back(i);
    }
  }
  hipError_t e = hipSuccess;
  if (!live.empty()) {
    int8_t* soft_base = nullptr;
    /* one readback: the result records follow the messages in q_out / h_out */
    ctx->h_res_off       = align16(ctx->h_out_used);
    const uint64_t rback = ctx->h_res_off + live.size() * sizeof(ldpc_hip_cb_result);
    if ((e = ctx->q_out.reserve(rback)) != hipSuccess ||
        (!ext && (e = ctx->q_soft.reserve(std::max<uint64_t>(ctx->h_soft_used, 16))) != hipSuccess) ||
        (e = ctx->h_out.reserve(rback, 0)) != hipSuccess) {
      return ctx->hip_fail(e, "HAL buffers");
    }
    soft_base = ext ? ctx->repo->arena.as<int8_t>() : ctx->q_soft.as<int8_t>();
    /* descriptors: dematch_cb[live], then the decode plan's dec_cb[live] and mixed_group[groups] */
    std::vector<ldpc_hip_dec_desc> dd(live.size());
    std::vector<dematch_cb>        dm(live.size());
    for (uint32_t k = 0; k != live.size(); ++k) {
      hal_op& op = ctx->hops[live[k]];
      op.pos     = k;
      /* llr: set once q_llr has its final size (below) */
      if (const char* why = make_dematch_cb(op.dm, nullptr, soft_base + op.soft_off, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, dm[k])) {
        return ctx->fail(LDPC_HIP_EINVAL, why);
      }
      dd[k] = make_dec_desc_from_hw(op.cfg, op.dm.cb_length, op.soft_off, op.out_off);
    }
    if (ctx->hplan == nullptr) {
      ctx->hplan = new ldpc_hip_plan();
    }
    std::vector<dec_cb>      cbs;
    std::vector<mixed_group> mg;
    int r = plan_host(ctx, static_cast<uint32_t>(dd.size()), dd.data(), *ctx->hplan, cbs, mg);
    if (r != LDPC_HIP_OK) {
      return r;
    }
    /* the dematcher runs fused into the decode kernels (one launch; LDPC_HIP_LAUNCH_SEPARATE_DEMATCH: its own kernel
     * first): its descriptors then go in the plan's block order */
    const bool fuse_dm = (ctx->params.launch_flags & LDPC_HIP_LAUNCH_SEPARATE_DEMATCH) == 0;
    if (fuse_dm) {
      std::vector<dematch_cb> dmp(dm.size());
      for (size_t i = 0; i != cbs.size(); ++i) {
        dmp[i] = dm[cbs[i].result_index];
      }
      dm.swap(dmp);
    }
    const uint32_t dm_lds  = fuse_dm ? dm_fused_budget(dm.data(), dm.size()) : 0U;
    const size_t dm_bytes  = dm.size() * sizeof(dematch_cb);
    const size_t cb_off    = align16(dm_bytes);
    const size_t cb_bytes  = cbs.size() * sizeof(dec_cb);
    const size_t mg_off    = align16(cb_off + cb_bytes);
    const size_t desc_size = mg_off + mg.size() * sizeof(mixed_group);
    /* one upload: the descriptors follow the staged LLRs in h_llr / q_llr */
    const uint64_t d0    = align16(ctx->h_llr_used);
    const uint64_t up    = align16(d0 + desc_size); /* copy items move 16-byte words */
    if ((e = hal_reserve_llr(ctx, up, ctx->h_llr_used)) != hipSuccess) {
      return ctx->hip_fail(e, "HAL descriptors");
    }
    if (up > ctx->q_llr.size) { /* q_llr moves: a copy queued early is lost (hal_copy_staged copies it again) */
      (void)hal_wait_copies(ctx);
      if ((e = hipStreamSynchronize(ctx->hq_stream)) != hipSuccess || (e = ctx->q_llr.reserve(up)) != hipSuccess) {
        return ctx->hip_fail(e, "HAL descriptors");
      }
      ctx->h_llr_copied = 0;
    }
    const bool zc = ext && up <= hal_zero_copy_max_bytes() &&
                    (ctx->params.launch_flags & LDPC_HIP_LAUNCH_HAL_COPY) == 0 && ctx->h_llr.dev != nullptr &&
                    ctx->h_out.dev != nullptr;
    /* early-copied batch: the LLRs (and descriptors) in HBM, the outputs still written straight into pinned memory */
    const bool early = zc && ctx->hcopy && live.size() > HAL_DWQ_MAX_CBS;
    if (!early) {
      (void)hal_wait_copies(ctx); /* copies of a batch that reads pinned memory after all (nothing reads q_llr) */
    }
    /* LLRs and descriptors as the kernels see them: the device copy, or (zero-copy) the pinned buffer itself */
    uint8_t* const llr_dev = (zc && !early) ? ctx->h_llr.dev_as<uint8_t>() : ctx->q_llr.as<uint8_t>();
    uint8_t* const out_dev = zc ? ctx->h_out.dev_as<uint8_t>() : ctx->q_out.as<uint8_t>();
    for (uint32_t k = 0; k != live.size(); ++k) { /* q_llr may have moved in reserve(): device pointers only now */
      const uint32_t c = fuse_dm ? cbs[k].result_index : k; /* dm[k] is live CB c's */
      dm[k].llr        = reinterpret_cast<int8_t*>(llr_dev) + ctx->hops[live[c]].llr_off;
    }
    uint8_t* hd = ctx->h_llr.as<uint8_t>() + d0;
    std::memcpy(hd, dm.data(), dm_bytes);
    std::memcpy(hd + cb_off, cbs.data(), cb_bytes);
    if (!mg.empty()) {
      std::memcpy(hd + mg_off, mg.data(), mg.size() * sizeof(mixed_group));
    }
    uint8_t* qd            = llr_dev + d0;
    ctx->hplan->cbs_dev    = reinterpret_cast<const dec_cb*>(qd + cb_off);
    ctx->hplan->groups_dev = reinterpret_cast<const mixed_group*>(qd + mg_off);
    ctx->hplan->has_one    = cbs.size() == 1; /* one-CB batch: both descriptors by value (no host-memory table read) */
    if (ctx->hplan->has_one) {
      ctx->hplan->one = cbs[0];
    }
    /* A zero-copy batch whose graphs all have specialised bodies goes to the device work queues: one item per
     * codeblock (fused dematch + decode), no launch, and each dequeue waits for its own codeblock only. */
    bool via_dwq = zc && !early && fuse_dm && ctx->use_dwq && cbs.size() <= HAL_DWQ_MAX_CBS;
    std::vector<const launch_group*> cb_grp(cbs.size(), nullptr);
    std::vector<dwq*>                cb_q(cbs.size(), nullptr);
    for (size_t i = 0; i != cbs.size() && via_dwq; ++i) {
      via_dwq = false;
      for (const launch_group& g : ctx->hplan->groups) {
        if (i >= g.first && i < g.first + g.count) {
          via_dwq   = g.sf08 && g.slot < NARROW_SLOT_BASE && ctx->graph_spec[g.slot] != 0;
          cb_grp[i] = &g;
        }
      }
      if (via_dwq) {
        const int sid = ctx->graph_spec[cb_grp[i]->slot] - 1;
        cb_q[i]       = dwq_get(ctx->device, 1 + sid, ctx->key_block[1 + sid], ctx->key_lds[1 + sid]);
        via_dwq       = cb_q[i] != nullptr;
      }
    }
    /* every queue the batch uses has a grid running (or one started now) within the residency budget; otherwise the
     * whole batch takes the launch path, so no item is ever left waiting for a stream */
    std::vector<dwq*> pinned; /* the distinct queues admitted (pinned) until the batch's items are submitted */
    for (size_t i = 0; i != cbs.size() && via_dwq; ++i) {
      if (std::find(pinned.begin(), pinned.end(), cb_q[i]) != pinned.end()) {
        continue;
      }
      via_dwq = dwq_admit(cb_q[i]);
      if (via_dwq) {
        pinned.push_back(cb_q[i]);
      }
    }
    struct unpin_all {
      std::vector<dwq*>& v;
      ~unpin_all()
      {
        for (dwq* q : v) {
          dwq_unpin(q);
        }
      }
    } unpin_guard{pinned};
    if (via_dwq) {
      issued = true;
      for (size_t i = 0; i != cbs.size(); ++i) {
        const launch_group* grp = cb_grp[i];
        const int           sid = ctx->graph_spec[grp->slot] - 1;
        dwq*                q   = cb_q[i];
        dwq_item it{};
        it.cb         = cbs[i];
        it.lay        = grp->lay;
        it.dm         = dm[i];
        it.llr_base   = soft_base;
        it.out_base   = out_dev;
        it.res_base   = reinterpret_cast<ldpc_hip_cb_result*>(out_dev + ctx->h_res_off);
        it.crc_tables = ctx->d_crc.as<uint32_t>();
        it.spec       = static_cast<uint32_t>(sid + 1);
        hal_op&  op     = ctx->hops[live[cbs[i].result_index]];
        uint32_t ticket = 0xffffffffU;
        e               = dwq_submit(q, it, ticket, false);
        if (ticket != 0xffffffffU) { /* published (also when an error follows): hal_sync waits for it */
          op.q      = q;
          op.ticket = ticket;
          if (ext) {
            ctx->repo->track_item(q, ticket); /* the arena may not move before this item is done (grow) */
          }
        }
        if (e != hipSuccess) {
          return ctx->hip_fail(e, "HAL work queue submit");
        }
      }
      ctx->hstate      = hal_state::launched;
      ctx->hbatch_done = false;
      return LDPC_HIP_OK;
    }
    hipStream_t s = ctx->hq_stream;
    issued        = true; /* from here on the stream may hold part of the batch */
    if (early && (e = hal_copy_staged(ctx, true, up)) == hipSuccess && ctx->hcopy_q != nullptr) {
      e = hal_wait_copies(ctx); /* the kernel reads q_llr: every copy item done (they run on the queue's own stream) */
    }
    if ((early && e != hipSuccess) || /* the last chunk and the descriptors */
        (!zc && (e = hipMemcpyAsync(ctx->q_llr.ptr, ctx->h_llr.ptr, up, hipMemcpyHostToDevice, s)) != hipSuccess) ||
        (!ext && (e = hipMemcpyAsync(ctx->q_soft.ptr, ctx->h_soft.ptr, ctx->h_soft_used, hipMemcpyHostToDevice, s)) !=
                     hipSuccess)) {
      return ctx->hip_fail(e, "HAL upload");
    }
    if (!fuse_dm && (e = launch_dematch(reinterpret_cast<const dematch_cb*>(qd), static_cast<uint32_t>(dm.size()),
                                        ctx->dtab, s, dm.size() == 1 ? dm.data() : nullptr)) != hipSuccess) {
      return ctx->hip_fail(e, "HAL dematch");
    }
    r = launch_plan(*ctx->hplan, soft_base, out_dev, reinterpret_cast<ldpc_hip_cb_result*>(out_dev + ctx->h_res_off),
                    s, fuse_dm ? reinterpret_cast<const dematch_cb*>(qd) : nullptr,
                    fuse_dm && dm.size() == 1 ? dm.data() : nullptr, dm_lds);
    if (r != LDPC_HIP_OK) {
      return r;
    }
    if ((!zc && (e = hipMemcpyAsync(ctx->h_out.ptr, ctx->q_out.ptr, rback, hipMemcpyDeviceToHost, s)) != hipSuccess) ||
        (!ext && (e = hipMemcpyAsync(ctx->h_soft.ptr, ctx->q_soft.ptr, ctx->h_soft_used, hipMemcpyDeviceToHost, s)) !=
                     hipSuccess)) {
      return ctx->hip_fail(e, "HAL readback");
    }
  }
  issued = true;
  if ((e = hipEventRecord(ctx->done_event, ctx->hq_stream)) != hipSuccess) {
    return ctx->hip_fail(e, "hipEventRecord");
  }
  ctx->hstate      = hal_state::launched;
  ctx->hbatch_done = false;
  return LDPC_HIP_OK;
}

/* hal_launch_issue, and on an error after any part of the batch was queued the batch is marked failed: a later dequeue
 * must not launch it again (its dematch may already have combined the LLRs into the HARQ soft buffers). */
int hal_launch(ldpc_hip_ctx* ctx)
{
  bool issued = false;
  int  r      = LDPC_HIP_ENOMEM;
  try {
    r = hal_launch_issue(ctx, issued);
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory (HAL launch)";
  }
  if (r != LDPC_HIP_OK && issued) {
    ctx->hstate = hal_state::failed;
    /* whatever part of the batch reached the stream ends before the done event (the HARQ memory's grow waits on it) */
    (void)hipEventRecord(ctx->done_event, ctx->hq_stream);
  }
  return r;
}

/* The device's shared hardware queues: HIP streams a context borrows per TB when opened with
 * LDPC_HIP_LAUNCH_SHARED_QUEUE, as acc100 without a dedicated queue reserves a bbdev queue in reserve_queue, spinning
 * until one is free, and frees it in free_queue (hw_accelerator_pusch_dec_acc100_impl.cpp:70-98). The pool holds
 * LDPC_HIP_SHARED_QUEUES streams (environment; default 4 = GPU_MAX_HW_QUEUES' default, one stream per hardware queue)
 * and lives as long as the process. */
struct shared_queue_pool {
  std::mutex               mu;
  std::vector<hipStream_t> streams;
  std::vector<uint8_t>     busy;
};

shared_queue_pool* queue_pool(int device)
{
  static std::mutex                                       mu;
  static std::map<int, std::unique_ptr<shared_queue_pool>> pools;
  std::lock_guard<std::mutex>                             lock(mu);
  std::unique_ptr<shared_queue_pool>&                     p = pools[device];
  if (!p) {
    p            = std::make_unique<shared_queue_pool>();
    const char* v = std::getenv("LDPC_HIP_SHARED_QUEUES");
    const int   n = std::max(1, std::min(64, v != nullptr ? std::atoi(v) : 4));
    (void)hipSetDevice(device);
    for (int i = 0; i != n; ++i) {
      hipStream_t st = nullptr;
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        break;
      }
      p->streams.push_back(st);
      p->busy.push_back(0);
    }
  }
  return p->streams.empty() ? nullptr : p.get();
}

/* reserve_queue without a dedicated queue: the index of a free shared queue, spinning (yielding) until one is */
int acquire_shared_queue(shared_queue_pool* p, hipStream_t& s)
{
  while (true) {
    {
      std::lock_guard<std::mutex> lock(p->mu);
      for (size_t i = 0; i != p->streams.size(); ++i) {
        if (p->busy[i] == 0) {
          p->busy[i] = 1;
          s          = p->streams[i];
          return static_cast<int>(i);
        }
      }
    }
    std::this_thread::yield();
  }
}

hal_op* hal_find(ldpc_hip_ctx* ctx, uint32_t cb_index)
{
  if (cb_index >= ctx->hslot.size() || ctx->hslot[cb_index] < 0) {
    return nullptr;
  }
  return &ctx->hops[static_cast<size_t>(ctx->hslot[cb_index])];
}

/* HAL operation indices: a TB has at most MAX_NOF_SEGMENTS = 162 codeblocks (sch_constants.h:38); larger indices are
 * contract violations, not a reason to grow the index table without bound */
constexpr uint32_t HAL_MAX_CB_INDEX = 4U * 162U;

int hal_enqueue(ldpc_hip_ctx* ctx, uint32_t cb_index, const ldpc_hip_hw_config* cfg, const int8_t* llrs,
                uint32_t nof_llrs, const int8_t* soft_in, uint32_t soft_len)
{
  if (ctx->hstate == hal_state::idle) {
    return ctx->fail(LDPC_HIP_ESTATE, "enqueue without a reserved queue");
  }
  if (ctx->hstate == hal_state::failed) {
    return ctx->fail(LDPC_HIP_ESTATE, "the batch failed to launch: free or reserve the queue again");
  }
  if (ctx->hstate == hal_state::launched) {
    if (ctx->hdequeued != ctx->hops.size()) {
      /* the batch is in flight: dequeue its operations first, then enqueue again (pusch_decoder_hw_impl.cpp:
       * 237-241 breaks out of its enqueue loop on false and dequeues) */
      return ctx->fail(LDPC_HIP_EFULL, "batch in flight");
    }
    hal_reset(ctx, hal_state::staging); /* every operation dequeued: a new batch on the same reservation */
  }
  const int      bg = cfg->base_graph;
  const unsigned Z  = cfg->lifting_size;
  const unsigned N  = (bg == 1 ? 66U : 50U) * Z;
  const ldpc_hip_dematch_desc dd{static_cast<uint8_t>(cfg->modulation_order), static_cast<uint8_t>(cfg->rv),
                                 static_cast<uint8_t>(cfg->new_data), 0, N, cfg->cw_length, cfg->Nref,
                                 cfg->nof_filler_bits};
  dematch_cb checked{};
  if (cb_index >= HAL_MAX_CB_INDEX || graph_slot(bg, Z) < 0 ||
      make_dematch_cb(dd, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, checked) != nullptr ||
      cfg->cw_length != nof_llrs || nof_llrs > ctx->params.max_cb_llrs || cfg->max_nof_ldpc_iterations == 0 ||
      cfg->max_nof_ldpc_iterations > 255 || cfg->cb_crc_type > 2) {
    return ctx->fail(LDPC_HIP_EINVAL, "invalid HAL operation configuration");
  }
  const bool ext = ctx->repo != nullptr;
  if (ext && ctx->repo->caller_state) {
    /* the device's HARQ memory holds any absolute_cb_id the caller's repository hands out: grow to it */
    const hipError_t ge = ctx->repo->grow(cfg->absolute_cb_id);
    if (ge != hipSuccess) {
      return ge == hipErrorInvalidValue ? ctx->fail(LDPC_HIP_EINVAL, "absolute CB index beyond 2^20")
                                        : ctx->hip_fail(ge, "HARQ memory growth");
    }
  } else if (ext && cfg->absolute_cb_id >= ctx->repo->nof_codeblocks) {
    /* ext_harq_buffer_context_repository::get asserts (ext_harq_buffer_context_repository.h:70-73) */
    return ctx->fail(LDPC_HIP_EINVAL, "absolute CB index out of the HARQ repository's bounds");
  }
  if (!ext && soft_in != nullptr && soft_len != 0 && soft_len != N) {
    return ctx->fail(LDPC_HIP_EINVAL, "soft buffer size differs from the codeblock length");
  }
  hal_op* existing = hal_find(ctx, cb_index);
  if (existing == nullptr && ctx->hops.size() >= ctx->params.max_queue_cbs) {
    return ctx->fail(LDPC_HIP_EFULL, "HAL batch full"); /* dequeue the batch, then enqueue again */
  }
  /* staging space (pinned; grows, keeping what is staged) */
  const uint64_t llr_off  = ctx->h_llr_used;
  const uint64_t soft_off = ctx->h_soft_used;
  const uint64_t out_off  = ctx->h_out_used;
  const unsigned mb       = msg_bytes_of(bg, Z);
  hipError_t     e;
  /* a large batch (more codeblocks than the work queue takes) with external HARQ stages its LLRs into HBM early */
  if (ctx->hops.empty()) {
    ctx->hcopy   = ext && cfg->nof_segments > HAL_DWQ_MAX_CBS && (hal_early_copy(ctx) || hal_dwq_copy(ctx));
    dwq_unpin(ctx->hcopy_q);
    ctx->hcopy_q = nullptr;
    if (ctx->hcopy && !hal_early_copy(ctx)) { /* the copy work queue, if a grid can serve it now */
      dwq* q       = dwq_get(ctx->device, DWQ_KEY_COPY, COPY_THREADS, 0);
      ctx->hcopy_q = (q != nullptr && dwq_admit(q)) ? q : nullptr;
      ctx->hcopy   = ctx->hcopy_q != nullptr;
    }
    if (ctx->hcopy) { /* room for the whole batch up front, so the staging buffers do not move under queued copies */
      const uint64_t want = static_cast<uint64_t>(cfg->nof_segments) * (align16(nof_llrs) + 256U) + 65536U;
      if ((e = hal_reserve_llr(ctx, want, 0)) != hipSuccess || (e = ctx->q_llr.reserve(want)) != hipSuccess) {
        return ctx->hip_fail(e, "HAL staging");
      }
    }
  }
  if ((e = hal_reserve_llr(ctx, llr_off + align16(nof_llrs), llr_off)) != hipSuccess ||
      (e = ctx->h_out.reserve(out_off + align16(mb), 0)) != hipSuccess ||
      (!ext && (e = ctx->h_soft.reserve(soft_off + align16(N), soft_off)) != hipSuccess)) {
    return ctx->hip_fail(e, "hipHostMalloc(HAL staging)");
  }
  hal_op op{};
  op.cb_index  = cb_index;
  op.cfg       = *cfg;
  op.dm        = dd;
  op.msg_bytes = mb;
  op.llr_off   = llr_off;
  op.out_off   = out_off;
  if (ext) {
    /* hw_config + hw_enqueue of hw_accelerator_pusch_dec_acc100_impl.cpp:113, 123-125, 182-185: the entry is
     * (re)initialised on new data; a retransmission whose entry holds no soft data is dropped */
    /* (with the caller keeping the entry state, the caller has decided already: nothing is dropped here) */
    const uint32_t soft_len_now = ctx->repo->caller_state ? 1U : ctx->repo->get(cfg->absolute_cb_id, cfg->new_data != 0);
    op.dropped                  = cfg->new_data == 0 && soft_len_now == 0;
    op.soft_off                 = static_cast<uint64_t>(cfg->absolute_cb_id) * LDPC_HIP_HARQ_STRIDE;
  } else {
    op.soft_off = soft_off;
    int8_t* dst = ctx->h_soft.as<int8_t>() + soft_off;
    if (soft_in != nullptr && soft_len != 0) {
      std::memcpy(dst, soft_in, N);
    } else {
      std::memset(dst, 0, N); /* a clean buffer (rx_buffer, pusch_decoder_impl.cpp:327) */
    }
    ctx->h_soft_used = soft_off + align16(N);
  }
  if (nof_llrs != 0) {
    std::memcpy(ctx->h_llr.as<int8_t>() + llr_off, llrs, nof_llrs);
  }
  ctx->h_llr_used = llr_off + align16(nof_llrs);
  ctx->h_out_used = out_off + align16(mb);
  if (ctx->hcopy && existing == nullptr && (e = hal_copy_staged(ctx, false, ctx->h_llr_used)) != hipSuccess) {
    return ctx->hip_fail(e, "HAL early copy");
  }
  if (existing != nullptr) {
    *existing = op; /* the same codeblock enqueued again before the launch: the later configuration wins */
  } else {
    if (cb_index >= ctx->hslot.size()) {
      ctx->hslot.resize(static_cast<size_t>(cb_index) + 1, -1);
    }
    ctx->hslot[cb_index] = static_cast<int32_t>(ctx->hops.size());
    ctx->hops.push_back(op);
  }
  return op.dropped ? LDPC_HIP_DROPPED : LDPC_HIP_OK;
}

} // namespace

namespace ldpc_hip {

void hal_sync(ldpc_hip_ctx* ctx)
{
  (void)hal_wait_copies(ctx);
  if (ctx->hstate == hal_state::launched || ctx->hstate == hal_state::failed) {
    /* every work-queue item submitted (a failed batch may have submitted some before its error) */
    for (const hal_op& op : ctx->hops) {
      if (op.q != nullptr) {
        (void)dwq_wait(op.q, op.ticket);
      }
    }
  }
  if (ctx->hstate == hal_state::launched) {
    (void)hipEventSynchronize(ctx->done_event);
  } else if (ctx->hstate == hal_state::failed) {
    (void)hipStreamSynchronize(ctx->hq_stream); /* whatever part of the failed launch was queued */
  } else if (ctx->hstate == hal_state::staging && ctx->h_llr_copied != 0) {
    (void)hipStreamSynchronize(ctx->hq_stream); /* early copies of a batch never launched still read h_llr */
  }
}

void release_shared_queue(ldpc_hip_ctx* ctx)
{
  if (ctx->hq_shared >= 0) {
    shared_queue_pool*          p = queue_pool(ctx->device);
    std::lock_guard<std::mutex> lock(p->mu);
    p->busy[static_cast<size_t>(ctx->hq_shared)] = 0;
    ctx->hq_shared                                = -1;
    ctx->hq_stream                                = ctx->stream;
  }
}

} // namespace ldpc_hip

extern "C" {

int ldpc_hip_external_harq_supported(const ldpc_hip_ctx* ctx)
{
  return (ctx != nullptr && ctx->repo != nullptr) ? 1 : 0;
}

int ldpc_hip_queue_reserve(ldpc_hip_ctx* ctx)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  hal_sync(ctx);
  hal_reset(ctx, hal_state::staging);
  if ((ctx->params.launch_flags & LDPC_HIP_LAUNCH_SHARED_QUEUE) != 0 && ctx->hq_shared < 0) {
    shared_queue_pool* p = queue_pool(ctx->device);
    if (p == nullptr) {
      return ctx->fail(LDPC_HIP_EDEVICE, "no shared hardware queue could be created");
    }
    ctx->hq_shared = acquire_shared_queue(p, ctx->hq_stream);
  }
  return LDPC_HIP_OK;
}

int ldpc_hip_queue_free(ldpc_hip_ctx* ctx)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  hal_sync(ctx);
  hal_reset(ctx, hal_state::idle);
  release_shared_queue(ctx);
  return LDPC_HIP_OK;
}

int ldpc_hip_enqueue(ldpc_hip_ctx* ctx, uint32_t cb_index, const ldpc_hip_hw_config* cfg, const int8_t* llrs,
                     uint32_t nof_llrs, const int8_t* soft_in, uint32_t soft_len)
{
  if (ctx == nullptr || cfg == nullptr || (nof_llrs != 0 && llrs == nullptr)) {
    return LDPC_HIP_EINVAL;
  }
  try {
    return hal_enqueue(ctx, cb_index, cfg, llrs, nof_llrs, soft_in, soft_len);
  } catch (const std::bad_alloc&) {
    return ctx->fail(LDPC_HIP_ENOMEM, "out of host memory (enqueue)");
  }
}

int ldpc_hip_dequeue(ldpc_hip_ctx* ctx, uint32_t cb_index, uint8_t* packed_msg, uint32_t msg_bytes, int8_t* soft_out,
                     uint32_t soft_len)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  hal_op* op = hal_find(ctx, cb_index);
  if (op == nullptr) {
    return ctx->fail(LDPC_HIP_ESTATE, "dequeue of an operation that was not enqueued");
  }
  if (ctx->hstate == hal_state::failed) {
    return ctx->fail(LDPC_HIP_EDEVICE, "the batch failed to launch: " + ctx->err);
  }
  if (ctx->hstate == hal_state::staging) {
    int r = hal_launch(ctx);
    if (r != LDPC_HIP_OK) {
      return r;
    }
    op = hal_find(ctx, cb_index);
  }
  if (op->q != nullptr) {
    if (!dwq_done(op->q, op->ticket)) {
      return LDPC_HIP_NOT_READY; /* this codeblock's work item (a work-queue batch completes CB by CB) */
    }
  } else if (!ctx->hbatch_done) {
    hipError_t q = hipEventQuery(ctx->done_event);
    if (q == hipErrorNotReady) {
      return LDPC_HIP_NOT_READY;
    }
    if (q != hipSuccess) {
      return ctx->hip_fail(q, "hipEventQuery");
    }
    ctx->hbatch_done = true;
  }
  const uint32_t N = op->dm.cb_length;
  if (op->dropped) {
    op->res.crc_pass       = 0;
    op->res.nof_iterations = static_cast<uint8_t>(op->cfg.max_nof_ldpc_iterations);
    op->res.status         = LDPC_HIP_STATUS_DROPPED;
  } else {
    op->res = reinterpret_cast<const ldpc_hip_cb_result*>(ctx->h_out.as<uint8_t>() + ctx->h_res_off)[op->pos];
    if (op->res.crc_pass == 0) {
      op->res.nof_iterations = static_cast<uint8_t>(op->cfg.max_nof_ldpc_iterations); /* acc100_impl.cpp:246 */
    }
    if (packed_msg != nullptr && (op->res.status & LDPC_HIP_STATUS_OUTPUT_WRITTEN)) {
      std::memcpy(packed_msg, ctx->h_out.as<uint8_t>() + op->out_off, std::min(op->msg_bytes, msg_bytes));
    }
    if (ctx->repo == nullptr && soft_out != nullptr) {
      std::memcpy(soft_out, ctx->h_soft.as<int8_t>() + op->soft_off, std::min<uint32_t>(N, soft_len));
    }
    if (ctx->repo != nullptr && !ctx->repo->caller_state && !op->dequeued) {
      /* the entry now holds the codeblock's soft data (acc100 hw_dequeue, acc100_impl.cpp:206-207) */
      ctx->repo->set_len(op->cfg.absolute_cb_id, N);
    }
  }
  if (!op->dequeued) {
    op->dequeued = true;
    ++ctx->hdequeued;
  }
  return LDPC_HIP_OK;
}

int ldpc_hip_read_outputs(ldpc_hip_ctx* ctx, uint32_t cb_index, uint32_t absolute_cb_id, ldpc_hip_cb_result* out)
{
  (void)absolute_cb_id;
  if (ctx == nullptr || out == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  const hal_op* op = hal_find(ctx, cb_index);
  if (op == nullptr || !op->dequeued) {
    return ctx->fail(LDPC_HIP_ESTATE, "read_operation_outputs before dequeue");
  }
  *out = op->res;
  return LDPC_HIP_OK;
}

int ldpc_hip_harq_free(ldpc_hip_ctx* ctx, uint32_t absolute_cb_id)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (ctx->repo != nullptr && !ctx->repo->caller_state) { /* caller_state: the caller frees its own entry */
    if (absolute_cb_id >= ctx->repo->nof_codeblocks) {
      return ctx->fail(LDPC_HIP_EINVAL, "absolute CB index out of the HARQ repository's bounds"); /* :89-91 */
    }
    ctx->repo->free(absolute_cb_id);
  }
  return LDPC_HIP_OK;
}

} /* extern "C" */
