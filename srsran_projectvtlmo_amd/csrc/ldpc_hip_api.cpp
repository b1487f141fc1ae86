/*
 * Host runtime behind the C ABI of include/srsran_ldpc_hip.h: context (device, stream, graph schedules, CRC tables,
 * HBM HARQ arena), graph capture, batched decode plans and the *_launch entry points. The synchronous entry points
 * are in ldpc_hip_sync.cpp, the HAL operation queue in ldpc_hip_hal.cpp, the descriptor translations in
 * ldpc_hip_descs.cpp; ldpc_hip_ctx.h holds what they share.
 */
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <set>

#include "ldpc_hip_ctx.h"
#include "ldpc_hip_launch.h"

using namespace ldpc_hip;

struct ldpc_hip_graph {
  ldpc_hip_ctx*  ctx   = nullptr;
  hipGraph_t     graph = nullptr;
  hipGraphExec_t exec  = nullptr;
};

namespace {

/* "auto" decoder type: the codeblock work (layer edges x Z x expected iterations, ldpc_hip_decode_work) from which a
 * decode call is faster on the GPU than on the host CPU. Measured on the GPU box (AMD EPYC 9575F, bench.py
 * extra.sw_route, profiles/r05/bench_a_line.json): a GPU call costs 21-22 us whatever the codeblock (PCIe and work-queue
 * round trips included), the CPU decoder port 12.2 us for C4's 6-layer BG1 Z=384 codeblocks with early stop (66 k
 * work) and 87.8 us for a full 8-iteration BG1 Z=384 codeblock without it (970 k); the crossover is ~150 k. */
constexpr uint64_t LDPC_HIP_AUTO_MIN_WORK_DEFAULT = 150000ULL;
/* iterations a decode with CRC early stop is expected to run (the C4 slot's mean is 1.8, C3's 1.14) */
constexpr uint64_t LDPC_HIP_AUTO_ET_ITERATIONS = 2ULL;

constexpr size_t MAX_AUX_STREAMS = 3; /* GPU_MAX_HW_QUEUES defaults to 4: the context stream + 3 */

/* The reference's demodulator tables, computed the way it computes them (float; demodulation_mapper_qam16.cpp:39,
 * demodulation_mapper_qam64.cpp:36-67, demodulation_mapper_qam256.cpp:37-160). */
demod_tables make_demod_tables()
{
  demod_tables t{};
  const float  s10 = 1.0F / std::sqrt(10.0F), s42 = 1.0F / std::sqrt(42.0F), s170 = 1.0F / std::sqrt(170.0F);
  t.s10            = s10;
  t.w64a           = 2 * s42;
  t.w64c           = 4 * s42;
  const int   k64[3][8] = {{16, 12, 8, 4, 4, 8, 12, 16}, {8, 4, 4, 8, -8, -4, -4, -8}, {4, -4, 4, -4, 0, 0, 0, 0}};
  const float n64[3][8] = {{24, 12, 4, 0, 0, -4, -12, -24}, {20, 8, 8, 12, 12, 8, 8, 20}, {12, -4, -4, 12, 0, 0, 0, 0}};
  for (int j = 0; j != 3; ++j) {
    for (int i = 0; i != 8; ++i) {
      t.sl64[j][i] = static_cast<float>(k64[j][i]) * s42;
      t.ic64[j][i] = n64[j][i] / 21;
    }
  }
  t.w256a                = 2 * s170;
  t.w256c                = 4 * s170;
  const int   k256[4][16] = {{32, 28, 24, 20, 16, 12, 8, 4, 4, 8, 12, 16, 20, 24, 28, 32},
                             {16, 12, 8, 4, 4, 8, 12, 16, -16, -12, -8, -4, -4, -8, -12, -16},
                             {8, 4, 4, 8, -8, -4, -4, -8, 8, 4, 4, 8, -8, -4, -4, -8},
                             {4, -4, 4, -4, 4, -4, 4, -4, 0, 0, 0, 0, 0, 0, 0, 0}};
  const float n256[4][16] = {{112, 84, 60, 40, 24, 12, 4, 0, 0, -4, -12, -24, -40, -60, -84, -112},
                             {88, 60, 36, 16, 16, 28, 36, 40, 40, 36, 28, 16, 16, 36, 60, 88},
                             {52, 24, 24, 44, -20, -8, -8, -12, -12, -8, -8, -20, 44, 24, 24, 52},
                             {28, -20, 12, -4, -4, 12, -20, 28, 0, 0, 0, 0, 0, 0, 0, 0}};
  for (int j = 0; j != 4; ++j) {
    for (int i = 0; i != 16; ++i) {
      t.sl256[j][i] = static_cast<float>(k256[j][i]) * s170;
      t.ic256[j][i] = n256[j][i] / 85;
    }
  }
  return t;
}

} // namespace

/* ---- the external HARQ repository (ldpc_hip_ctx.h) ---- */
hipError_t ldpc_hip_harq_repo::wait_users()
{
  std::lock_guard<std::mutex> lock(inflight_mu);
  hipError_t                  e = hipSuccess;
  for (const auto& it : inflight) {
    /* a timed-out item is harmless only once its queue's grid has left (a stopped grid claims nothing); while the
     * grid is still resident the arena must not be freed: the error goes to the caller and the arena stays */
    if (dwq_wait(it.first, it.second) != hipSuccess && !dwq_quiesced(it.first)) {
      e = hipErrorLaunchTimeOut;
    }
  }
  if (e != hipSuccess) {
    return e;
  }
  inflight.clear();
  for (hipEvent_t ev : user_events) {
    const hipError_t r = hipEventSynchronize(ev);
    e                  = e == hipSuccess ? r : e;
  }
  return e;
}

hipError_t ldpc_hip_harq_repo::grow(uint32_t id)
{
  {
    std::shared_lock<std::shared_mutex> rd(arena_mu);
    if (id < nof_codeblocks) {
      return hipSuccess;
    }
  }
  std::unique_lock<std::shared_mutex> wr(arena_mu);
  if (id < nof_codeblocks) {
    return hipSuccess;
  }
  if (id >= MAX_CODEBLOCKS) {
    return hipErrorInvalidValue;
  }
  const uint32_t n = std::min<uint32_t>(MAX_CODEBLOCKS, std::max<uint32_t>(2U * nof_codeblocks, (id + 1024U) & ~1023U));
  hipError_t     e = hipSetDevice(device);
  void*          p = nullptr;
  const size_t   old_bytes = static_cast<size_t>(nof_codeblocks) * LDPC_HIP_HARQ_STRIDE;
  const size_t   bytes     = static_cast<size_t>(n) * LDPC_HIP_HARQ_STRIDE;
  if (e == hipSuccess) {
    e = wait_users();
  }
  if (e == hipSuccess) {
    e = hipMalloc(&p, bytes);
  }
  if (e == hipSuccess && old_bytes != 0) {
    e = hipMemcpy(p, arena.ptr, old_bytes, hipMemcpyDeviceToDevice);
  }
  if (e == hipSuccess) {
    e = hipMemset(static_cast<int8_t*>(p) + old_bytes, 0, bytes - old_bytes);
  }
  if (e != hipSuccess) {
    if (p != nullptr) {
      (void)hipFree(p);
    }
    return e;
  }
  if (arena.ptr != nullptr) {
    (void)hipFree(arena.ptr);
  }
  arena.ptr      = p;
  arena.size     = bytes;
  nof_codeblocks = n;
  return hipSuccess;
}

void ldpc_hip_harq_repo::release()
{
  if (refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {
    (void)hipSetDevice(device);
    delete this;
  }
}

namespace ldpc_hip {

hipError_t desc_table::upload(const void* src, size_t n, hipStream_t s)
{
  hipError_t e = buf.reserve(n);
  if (e != hipSuccess) {
    return e;
  }
  const auto* b = static_cast<const uint8_t*>(src);
  if (last_ptr == buf.ptr && last_stream == s && last.size() == n && std::memcmp(last.data(), b, n) == 0) {
    return hipSuccess;
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
    return hipErrorStreamCaptureUnsupported; /* new descriptors inside a graph capture: launch once before capturing */
  }
  e = hipMemcpyAsync(buf.ptr, src, n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    last.assign(b, b + n);
    last_ptr    = buf.ptr;
    last_stream = s;
  } else {
    last_ptr = nullptr; /* forgotten: no buffer's address */
  }
  return e;
}

int plan_host(ldpc_hip_ctx* ctx, uint32_t n, const ldpc_hip_dec_desc* descs, ldpc_hip_plan& plan,
              std::vector<dec_cb>& cbs, std::vector<mixed_group>& mg)
{
  const uint32_t flags = ctx->params.launch_flags;
  plan.ctx             = ctx;
  plan.n               = n;
  plan.groups.clear();
  plan.mixed     = false;
  plan.mixed_lds = 0;
  mg.clear();
  if (const char* why = make_dec_cbs(n, descs, cbs)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  /* launch groups: one kernel launch per (BG, Z, default-scaling) class, consecutive in cbs */
  for (uint32_t i = 0; i != n; ++i) {
    const ldpc_hip_dec_desc& s    = descs[cbs[i].result_index];
    const int                slot = graph_slot(s.base_graph, s.lifting_size);
    const bool               sf08 = cbs[i].scaling_factor == 0.8f;
    if (plan.groups.empty() || plan.groups.back().slot != slot || plan.groups.back().sf08 != sf08) {
      const graph_desc& g = ctx->graphs[slot];
      /* the specialised kernels implement the default scaling factor only (integer round(0.8 m)) */
      const int spec = sf08 ? static_cast<int>(ctx->graph_spec[slot]) - 1 : -1;
      plan.groups.push_back({slot, i, 0, make_lds_layout(g, spec >= 0),
                             spec >= 0 ? 64 * spec_waves(spec) : decoder_block_size(g), sf08});
    }
    plan.groups.back().count++;
  }
  /* Large groups (more CBs than CUs) of a graph with a narrow schedule take it: two workgroups per CU. */
  for (launch_group& g : plan.groups) {
    const int  ns    = NARROW_SLOT_BASE + g.slot;
    const bool avail = !(g.sf08 && ctx->graph_spec[g.slot] != 0) && ctx->graph_valid[ns] != 0 &&
                       ctx->narrow_fits2[g.slot] != 0;
    const bool want  = (flags & LDPC_HIP_LAUNCH_NARROW_ALWAYS) != 0 ||
                      ((flags & LDPC_HIP_LAUNCH_NARROW_NEVER) == 0 && g.count > static_cast<uint32_t>(ctx->n_cu));
    if (avail && want) {
      g.slot  = ns;
      g.lay   = make_lds_layout(ctx->graphs[ns]);
      g.block = decoder_block_size(ctx->graphs[ns]);
    }
  }
  /* Mixed launch: several groups, one scaling path, every CB resident at once (at most one workgroup per CU with the
   * largest group's LDS) and every group's schedule within MIXED_BLOCK threads (a wider generic schedule takes its
   * narrow form). */
  plan.mixed = plan.groups.size() > 1 && n <= static_cast<uint32_t>(ctx->n_cu) &&
               (flags & LDPC_HIP_LAUNCH_NO_MIXED) == 0;
  for (launch_group& g : plan.groups) {
    if (!plan.mixed) {
      break;
    }
    int slot = g.slot;
    /* the mixed kernel carries the core specialised bodies only; a graph whose specialised kernel is standalone-only
     * runs the generic body there, and a generic schedule wider than the mixed block takes its narrow form */
    const int  sid  = (g.sf08 && slot < NARROW_SLOT_BASE) ? static_cast<int>(ctx->graph_spec[slot]) - 1 : -1;
    const bool spec = sid >= 0 && sid < spec_core_count();
    if (!spec && slot < NARROW_SLOT_BASE && decoder_block_size(ctx->graphs[slot]) > MIXED_BLOCK &&
        ctx->graph_valid[NARROW_SLOT_BASE + slot] != 0) {
      slot = NARROW_SLOT_BASE + slot;
    }
    const lds_layout lay  = make_lds_layout(ctx->graphs[slot], spec);
    const int block = spec ? 64 * spec_waves(sid) : decoder_block_size(ctx->graphs[slot]);
    if (block > MIXED_BLOCK || g.sf08 != plan.groups[0].sf08) {
      plan.mixed = false;
      break;
    }
    mixed_group m{};
    m.first_block  = g.first;
    m.graph_slot   = slot;
    m.task_offset  = ctx->graphs[slot].task_offset;
    m.spec         = spec ? static_cast<uint32_t>(sid + 1) : 0U; /* specialised kernel id + 1 */
    m.lay          = lay;
    mg.push_back(m);
    plan.mixed_lds = std::max(plan.mixed_lds, lay.total);
  }
  if (!plan.mixed) {
    mg.clear();
  }
  return LDPC_HIP_OK;
}

int build_plan(ldpc_hip_ctx* ctx, uint32_t n, const ldpc_hip_dec_desc* descs, ldpc_hip_plan& plan)
{
  std::vector<dec_cb>      cbs;
  std::vector<mixed_group> mg;
  int                      r = plan_host(ctx, n, descs, plan, cbs, mg);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  hipError_t e = hipSuccess;
  if (!mg.empty()) {
    e = plan.d_groups.reserve(mg.size() * sizeof(mixed_group));
    if (e == hipSuccess) {
      e = hipMemcpy(plan.d_groups.ptr, mg.data(), mg.size() * sizeof(mixed_group), hipMemcpyHostToDevice);
    }
  }
  if (e == hipSuccess && n != 0) {
    e = plan.d_cbs.reserve(n * sizeof(dec_cb));
    if (e == hipSuccess) {
      e = hipMemcpy(plan.d_cbs.ptr, cbs.data(), n * sizeof(dec_cb), hipMemcpyHostToDevice);
    }
  }
  if (e != hipSuccess) {
    return ctx->hip_fail(e, "decode plan upload");
  }
  plan.cbs_dev    = plan.d_cbs.as<dec_cb>();
  plan.groups_dev = plan.d_groups.as<mixed_group>();
  plan.h_cbs      = std::move(cbs);
  return LDPC_HIP_OK;
}

int launch_plan(ldpc_hip_plan& plan, const int8_t* d_llr, uint8_t* d_out, ldpc_hip_cb_result* d_res,
                hipStream_t stream, const dematch_cb* d_dm, const dematch_cb* dm_one, uint32_t dm_lds)
{
  ldpc_hip_ctx* ctx = plan.ctx;
  if (plan.mixed) {
    const hipError_t e = launch_decode_mixed(plan.groups[0].sf08, plan.cbs_dev, plan.n, plan.groups_dev,
                                             static_cast<uint32_t>(plan.groups.size()), plan.mixed_lds,
                                             ctx->d_tasks.as<step_task>(), d_llr, d_out, d_res,
                                             ctx->d_crc.as<uint32_t>(), stream, d_dm, dm_lds);
    return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "ldpc_decode_mixed_kernel launch");
  }
  /* One launch per (BG, Z) group. Groups are independent (disjoint CBs, outputs and result slots), so with more than
   * one group (a mixed slot: the large-TB BG1 CBs beside the small-TB BG2 CBs) every group after the first runs on an
   * auxiliary stream forked from and joined back into `stream`: the groups share the GPU instead of queueing behind
   * each other. Stream order as seen by the caller is unchanged. */
  const size_t ng   = plan.groups.size();
  const size_t naux = std::min<size_t>(ng > 1 ? ng - 1 : 0, MAX_AUX_STREAMS);
  while (ctx->aux_streams.size() < naux) {
    hipStream_t s = nullptr;
    hipEvent_t  ev = nullptr;
    if (ctx->aux_events.empty()) {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        return ctx->fail(LDPC_HIP_EDEVICE, "hipEventCreate(fork)");
      }
      ctx->aux_events.push_back(ev);
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      return ctx->fail(LDPC_HIP_EDEVICE, "hipStreamCreate(aux)");
    }
    ctx->aux_streams.push_back(s);
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      return ctx->fail(LDPC_HIP_EDEVICE, "hipEventCreate(join)");
    }
    ctx->aux_events.push_back(ev);
  }
  hipError_t e = hipSuccess;
  if (naux != 0) {
    e = hipEventRecord(ctx->aux_events[0], stream);
    for (size_t i = 0; i != naux && e == hipSuccess; ++i) {
      e = hipStreamWaitEvent(ctx->aux_streams[i], ctx->aux_events[0], 0);
    }
    if (e != hipSuccess) {
      return ctx->hip_fail(e, "decode fork");
    }
  }
  for (size_t gi = 0; gi != ng; ++gi) {
    const launch_group& g  = plan.groups[gi];
    hipStream_t         gs = (gi == 0 || naux == 0) ? stream : ctx->aux_streams[(gi - 1) % naux];
    const int spec = (g.sf08 && g.slot < NARROW_SLOT_BASE) ? static_cast<int>(ctx->graph_spec[g.slot]) - 1 : -1;
    e = launch_decode(g.sf08, spec, plan.cbs_dev + g.first, g.count, g.slot,
                      ctx->d_tasks.as<step_task>() + ctx->graphs[g.slot].task_offset, g.lay, g.block, d_llr, d_out,
                      d_res, ctx->d_crc.as<uint32_t>(), gs, (plan.has_one && ng == 1) ? &plan.one : nullptr,
                      d_dm != nullptr ? d_dm + g.first : nullptr, (plan.has_one && ng == 1) ? dm_one : nullptr,
                      dm_lds);
    if (e != hipSuccess) {
      return ctx->hip_fail(e, "ldpc_decode_kernel launch");
    }
  }
  for (size_t i = 0; i != naux && e == hipSuccess; ++i) {
    e = hipEventRecord(ctx->aux_events[1 + i], ctx->aux_streams[i]);
    if (e == hipSuccess) {
      e = hipStreamWaitEvent(stream, ctx->aux_events[1 + i], 0);
    }
  }
  if (e != hipSuccess) {
    return ctx->hip_fail(e, "decode join");
  }
  return LDPC_HIP_OK;
}

/* ---- soft demodulation mapper ---- */
int demodulate_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_demod_desc* descs, const float* d_sym,
                        const float* d_nv, int8_t* d_llr, hipStream_t s)
{
  std::vector<demod_seg> sg;
  uint32_t               blocks = 0;
  if (const char* why = make_segs(nof_segs, descs, sg, blocks, make_demod_seg)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  return ctx->launch_items(ctx->d_dmsegs, sg, s, "ldpc_demodulate_kernel launch", [&](const demod_seg* d_segs) {
    return launch_demodulate(d_segs, static_cast<uint32_t>(sg.size()), blocks, ctx->dtab, d_sym, d_nv, d_llr, s);
  });
}

/* ---- pseudo-random sequences: descrambling and the packed-bit scrambler ----
 * the segments as work items with their start states, and the launch; d_in == nullptr: generate (bits only) */
int prs_segments(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_prs_seg* segs, bool bits, const uint8_t* d_in,
                 uint8_t* d_out, hipStream_t s)
{
  std::vector<prs_seg> sg;
  uint32_t             blocks = 0;
  if (const char* why = make_segs(nof_segs, segs, sg, blocks, make_prs_seg, d_in != nullptr)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  return ctx->launch_items(ctx->d_prssegs, sg, s, "ldpc_prs_kernel launch", [&](const prs_seg* d_segs) {
    return launch_prs(d_segs, static_cast<uint32_t>(sg.size()), blocks, bits, d_in, d_out, s);
  });
}

} // namespace ldpc_hip

/* =============================================================================================================== */
extern "C" {

const char* ldpc_hip_version(void) { return "srsran_ldpc_hip 0.2 gfx950"; }

int ldpc_hip_harq_repo_create(int device, uint32_t nof_codeblocks, int debug_mode, ldpc_hip_harq_repo** out)
{
  if (out == nullptr || nof_codeblocks == 0 || nof_codeblocks > (1U << 20)) {
    return LDPC_HIP_EINVAL;
  }
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) {
    return LDPC_HIP_EDEVICE;
  }
  std::unique_ptr<ldpc_hip_harq_repo> r(new (std::nothrow) ldpc_hip_harq_repo());
  if (!r) {
    return LDPC_HIP_ENOMEM;
  }
  r->device         = device;
  r->nof_codeblocks = nof_codeblocks;
  r->debug_mode     = debug_mode != 0;
  r->state.reset(new (std::nothrow) std::atomic<uint32_t>[nof_codeblocks]);
  if (!r->state) {
    return LDPC_HIP_ENOMEM;
  }
  for (uint32_t i = 0; i != nof_codeblocks; ++i) {
    r->state[i].store(0U, std::memory_order_relaxed);
  }
  const size_t bytes = static_cast<size_t>(nof_codeblocks) * LDPC_HIP_HARQ_STRIDE;
  if (r->arena.reserve(bytes) != hipSuccess || hipMemset(r->arena.ptr, 0, bytes) != hipSuccess) {
    return LDPC_HIP_ENOMEM;
  }
  *out = r.release();
  return LDPC_HIP_OK;
}

int ldpc_hip_harq_repo_release(ldpc_hip_harq_repo* repo)
{
  if (repo == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  repo->release();
  return LDPC_HIP_OK;
}

int ldpc_hip_harq_device_memory(int device, ldpc_hip_harq_repo** out)
{
  if (out == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  *out = nullptr;
  static std::mutex                        mu;
  static std::map<int, ldpc_hip_harq_repo*> mems; /* one per device, alive for the process (one reference held) */
  std::lock_guard<std::mutex>              lock(mu);
  ldpc_hip_harq_repo*&                     m = mems[device];
  if (m == nullptr) {
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || device < 0 || device >= dev_count) {
      return LDPC_HIP_EDEVICE;
    }
    std::unique_ptr<ldpc_hip_harq_repo> r(new (std::nothrow) ldpc_hip_harq_repo());
    if (!r) {
      return LDPC_HIP_ENOMEM;
    }
    r->device       = device;
    r->caller_state = true;
    const char* v   = std::getenv("LDPC_HIP_HARQ_CODEBLOCKS");
    const long  n   = v != nullptr ? std::atol(v) : 2048;
    if (n > 0 && r->grow(static_cast<uint32_t>(std::min<long>(n, ldpc_hip_harq_repo::MAX_CODEBLOCKS)) - 1U) !=
                     hipSuccess) {
      return LDPC_HIP_ENOMEM;
    }
    m = r.release();
  }
  m->refs.fetch_add(1, std::memory_order_acq_rel);
  *out = m;
  return LDPC_HIP_OK;
}

uint32_t ldpc_hip_harq_capacity(const ldpc_hip_harq_repo* repo)
{
  if (repo == nullptr) {
    return 0;
  }
  std::shared_lock<std::shared_mutex> lock(const_cast<ldpc_hip_harq_repo*>(repo)->arena_mu);
  return repo->nof_codeblocks;
}

int ldpc_hip_auto_device(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return -1;
  }
  const char* v   = std::getenv("LDPC_HIP_AUTO_DEVICE");
  const int   dev = v != nullptr ? std::atoi(v) : 0;
  if (dev < 0 || dev >= n) {
    return -1;
  }
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    (void)hipGetLastError();
    return -1; /* the kernels are built for gfx950 only */
  }
  return dev;
}

uint64_t ldpc_hip_decode_work(const ldpc_hip_dec_desc* d, const int8_t* llr)
{
  if (d == nullptr || (d->base_graph != 1 && d->base_graph != 2) || lifting_position(d->lifting_size) < 0 ||
      (d->llr_length != 0 && llr == nullptr)) {
    return 0;
  }
  const uint64_t Z = d->lifting_size;
  const uint64_t K = d->base_graph == 1 ? 22U : 10U;
  /* last non-zero LLR (ldpc_decoder_impl.cpp:97-101), scanned from the end eight bytes at a time */
  uint64_t last = d->llr_length;
  while (last >= 8) {
    uint64_t w;
    std::memcpy(&w, llr + last - 8, 8);
    if (w != 0) {
      break;
    }
    last -= 8;
  }
  while (last != 0 && llr[last - 1] == 0) {
    --last;
  }
  if (last == 0) {
    return 0;
  }
  /* codeblock length and layers (ldpc_decoder_impl.cpp:103-114) */
  uint64_t cb_len = std::max<uint64_t>(last + 2 * Z, (K + 4) * Z);
  cb_len          = (cb_len + Z - 1) / Z * Z;
  const unsigned nof_layers = static_cast<unsigned>(cb_len / Z - K);
  const uint64_t it         = (d->crc_mode & 0x0fU) == LDPC_HIP_CRC_MODE_EARLY_STOP
                                  ? std::min<uint64_t>(d->max_iterations, LDPC_HIP_AUTO_ET_ITERATIONS)
                                  : d->max_iterations;
  return static_cast<uint64_t>(layer_edges(d->base_graph, nof_layers)) * Z * it;
}

uint64_t ldpc_hip_auto_min_work(void)
{
  static const uint64_t v = [] {
    const char* e = std::getenv("LDPC_HIP_AUTO_MIN_WORK");
    return e != nullptr ? std::strtoull(e, nullptr, 10) : LDPC_HIP_AUTO_MIN_WORK_DEFAULT;
  }();
  return v;
}

int ldpc_hip_harq_repo_entry(const ldpc_hip_harq_repo* repo, uint32_t id, uint32_t* soft_data_len)
{
  if (repo == nullptr || id >= repo->nof_codeblocks) {
    return LDPC_HIP_EINVAL;
  }
  if (repo->caller_state) {
    return LDPC_HIP_ESTATE; /* the device's HARQ memory: the caller's repository holds the entry state */
  }
  const uint32_t s = repo->state[id].load(std::memory_order_acquire);
  if (soft_data_len != nullptr) {
    *soft_data_len = s & ~ldpc_hip_harq_repo::IN_USE;
  }
  return (s & ldpc_hip_harq_repo::IN_USE) != 0 ? 0 : 1;
}

int ldpc_hip_harq_repo_read(ldpc_hip_harq_repo* repo, uint32_t id, int8_t* dst, uint32_t len)
{
  if (repo == nullptr || len > LDPC_HIP_HARQ_STRIDE || (len != 0 && dst == nullptr)) {
    return LDPC_HIP_EINVAL;
  }
  std::shared_lock<std::shared_mutex> lock(repo->arena_mu);
  if (id >= repo->nof_codeblocks) {
    return LDPC_HIP_EINVAL;
  }
  (void)hipSetDevice(repo->device);
  return hipMemcpy(dst, repo->entry(id), len, hipMemcpyDeviceToHost) == hipSuccess ? LDPC_HIP_OK : LDPC_HIP_EDEVICE;
}

int ldpc_hip_open(int device, const ldpc_hip_params* params, ldpc_hip_ctx** out)
{
  return ldpc_hip_open_harq(device, params, nullptr, out);
}

int ldpc_hip_open_harq(int device, const ldpc_hip_params* params, ldpc_hip_harq_repo* repo, ldpc_hip_ctx** out)
{
  if (out == nullptr || (repo != nullptr && repo->device != device)) {
    return LDPC_HIP_EINVAL;
  }
  *out     = nullptr;
  auto ctx = std::make_unique<ldpc_hip_ctx>();
  if (params != nullptr) {
    ctx->params = *params;
  }
  if (ctx->params.max_queue_cbs == 0) {
    ctx->params.max_queue_cbs = 162; /* MAX_NOF_SEGMENTS (sch_constants.h:38) */
  }
  if (ctx->params.max_cb_llrs == 0) {
    ctx->params.max_cb_llrs = 4U * MAX_CB_LEN;
  }
  ctx->device  = device;
  ctx->dtab    = make_demod_tables();
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    return LDPC_HIP_EDEVICE;
  }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->done_event, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->sync_event, hipEventDisableTiming) != hipSuccess) {
    return LDPC_HIP_EDEVICE;
  }
  ctx->hq_stream = ctx->stream;
  {
    const char* v = std::getenv("LDPC_HIP_SYNC_ZERO_COPY");
    ctx->sync_zc  = v == nullptr || std::strcmp(v, "0") != 0;
  }
  /* the one-CB staging of the software route: a whole codeblock's LLRs plus a 32 KiB rate-matched input */
  if (ctx->s_in.reserve(MAX_CB_LEN + 32768 + 16, 0) != hipSuccess || ctx->s_out.reserve(4096, 0) != hipSuccess) {
    return LDPC_HIP_ENOMEM;
  }
  ctx->bar_failed = ctx->s_bar.reserve(MAX_CB_LEN + 16) != hipSuccess; /* optional: s_in serves without it */
  (void)hipGetLastError();
  ctx->graphs.resize(NOF_GRAPH_SLOTS);
  ctx->graph_valid.assign(NOF_GRAPH_SLOTS, 0);
  if (hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      ctx->n_cu <= 0) {
    ctx->n_cu = 256;
  }
  uint32_t max_lds = 0;
  for (int bg = 1; bg <= 2; ++bg) {
    for (int p = 0; p != 51; ++p) {
      const int slot = (bg - 1) * 51 + p;
      if (build_graph(bg, k_lifting_sizes[p], ctx->graphs[slot])) {
        ctx->graph_valid[slot] = 1;
        max_lds                = std::max({max_lds, make_lds_layout(ctx->graphs[slot]).total,
                                           make_lds_layout(ctx->graphs[slot], true).total});
      }
    }
  }
  std::vector<step_task> tasks;
  for (int slot = 0; slot != 102; ++slot) {
    if (ctx->graph_valid[slot]) {
      build_tasks(ctx->graphs[slot], tasks);
    }
  }
  /* Narrow schedules: at most NARROW_WAVES waves per workgroup, so that two workgroups share a CU (LDS and the
   * generic kernel's <= 128 VGPRs permitting). A batch of many more CBs than CUs then keeps two CBs in flight per CU,
   * each hiding the other's step latency, instead of running them one after the other. */
  for (int slot = 0; slot != 102; ++slot) {
    if (!ctx->graph_valid[slot]) {
      continue;
    }
    graph_desc& n = ctx->graphs[NARROW_SLOT_BASE + slot];
    n             = ctx->graphs[slot];
    build_tasks(n, tasks, NARROW_WAVES);
    /* valid: narrower than the wide schedule (also used to fit a mixed launch's workgroup); narrow_fits2: two
     * workgroups fit a CU's LDS (the large-batch rule) */
    ctx->graph_valid[NARROW_SLOT_BASE + slot] = (n.task_waves < ctx->graphs[slot].task_waves) ? 1 : 0;
    ctx->narrow_fits2[slot] = (2U * make_lds_layout(n).total <= 160U * 1024U) ? 1 : 0;
  }
  /* specialised kernel where its compile-time schedule equals build_graph's (LDPC_HIP_LAUNCH_NO_SPEC disables it) */
  ctx->graph_spec.assign(NOF_GRAPH_SLOTS, 0);
  for (int slot = 0; slot != 102; ++slot) {
    if (ctx->graph_valid[slot] && (ctx->params.launch_flags & LDPC_HIP_LAUNCH_NO_SPEC) == 0) {
      ctx->graph_spec[slot] = static_cast<uint8_t>(spec_index(ctx->graphs[slot], make_lds_layout(ctx->graphs[slot], true)) + 1);
    }
  }
  /* the work queues' kernels: per specialised graph, its body's width and layout (at least the fused dematcher's
   * staging); the dematch-only kernel's */
  ctx->use_dwq = dwq_enabled() && (ctx->params.launch_flags & (LDPC_HIP_LAUNCH_NO_DWQ | LDPC_HIP_LAUNCH_NO_SPEC)) == 0;
  for (int slot = 0; slot != 102; ++slot) {
    const int id = static_cast<int>(ctx->graph_spec[slot]) - 1;
    if (id < 0) {
      continue;
    }
    ctx->spec_lay[slot]    = make_lds_layout(ctx->graphs[slot], true);
    ctx->key_block[1 + id] = 64 * spec_waves(id);
    ctx->key_lds[1 + id]   = std::max(ctx->spec_lay[slot].total, DM_FUSED_LDS);
  }
  ctx->key_block[0] = DM_THREADS;
  ctx->key_lds[0]   = DM_FUSED_LDS;
  if (ctx->d_tasks.reserve(tasks.size() * sizeof(step_task)) != hipSuccess ||
      hipMemcpy(ctx->d_tasks.ptr, tasks.data(), tasks.size() * sizeof(step_task), hipMemcpyHostToDevice) !=
          hipSuccess) {
    return LDPC_HIP_EDEVICE;
  }
  {
    /* the graph table in constant memory and the kernels' LDS limit are per process and device: set once, so that a
     * context opened while another context's kernels run on the device does not rewrite them under those kernels */
    static std::mutex    once_mutex;
    static std::set<int> done;
    std::lock_guard<std::mutex> lock(once_mutex);
    if (done.count(device) == 0) {
      if (upload_graphs(ctx->graphs.data(), NOF_GRAPH_SLOTS) != hipSuccess || configure_kernels(max_lds) != hipSuccess) {
        return LDPC_HIP_EDEVICE;
      }
      done.insert(device);
    }
  }
  std::vector<uint32_t> crc = build_crc_tables();
  static_assert(sizeof(demod_tables) <= DTAB_WORDS * 4U, "DTAB_WORDS");
  std::memcpy(crc.data() + DTAB_OFFSET, &ctx->dtab, sizeof(demod_tables)); /* the fused dematcher's tables */
  if (ctx->d_crc.reserve(crc.size() * 4) != hipSuccess ||
      hipMemcpy(ctx->d_crc.ptr, crc.data(), crc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    return LDPC_HIP_EDEVICE;
  }
  {
    /* the specialised BG1 kernels' split-row address tables, after the CRC tables (SPLIT_TAB_OFFSET) */
    int spec_ids[51];
    for (int p = 0; p != 51; ++p) {
      spec_ids[p] = ctx->graph_valid[p] ? spec_index(ctx->graphs[p], make_lds_layout(ctx->graphs[p], true)) : -1;
    }
    if (write_split_tables(ctx->d_crc.as<uint32_t>(), spec_ids, ctx->stream) != hipSuccess) {
      return LDPC_HIP_EDEVICE;
    }
  }
  if (repo != nullptr) {
    repo->refs.fetch_add(1, std::memory_order_acq_rel);
    ctx->repo = repo;
  } else if (ctx->params.nof_harq_slots != 0) {
    /* a private repository (the context's own external HARQ memory) */
    const int r = ldpc_hip_harq_repo_create(device, ctx->params.nof_harq_slots, 0, &ctx->repo);
    if (r != LDPC_HIP_OK) {
      return r;
    }
  }
  if (ctx->repo != nullptr) {
    ctx->repo->add_user(ctx->done_event); /* grow() waits for this context's issued HAL batches */
  }
  *out = ctx.release();
  return LDPC_HIP_OK;
}

int ldpc_hip_close(ldpc_hip_ctx* ctx)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  (void)hipSetDevice(ctx->device);
  /* a HAL batch still in flight (work-queue items included) reads and writes this context's pinned buffers */
  hal_sync(ctx);
  if (ctx->stream != nullptr) {
    (void)hipStreamSynchronize(ctx->stream);
  }
  if (ctx->repo != nullptr) {
    ctx->repo->remove_user(ctx->done_event);
  }
  if (ctx->hq_shared >= 0) {
    (void)hipStreamSynchronize(ctx->hq_stream);
    release_shared_queue(ctx);
  }
  delete ctx->hplan;
  ctx->hplan = nullptr;
  if (ctx->done_event != nullptr) {
    (void)hipEventDestroy(ctx->done_event);
  }
  if (ctx->sync_event != nullptr) {
    (void)hipEventDestroy(ctx->sync_event);
  }
  for (hipStream_t a : ctx->aux_streams) {
    (void)hipStreamSynchronize(a);
    (void)hipStreamDestroy(a);
  }
  for (hipEvent_t ev : ctx->aux_events) {
    (void)hipEventDestroy(ev);
  }
  hipStream_t         s    = ctx->stream;
  ldpc_hip_harq_repo* repo = ctx->repo;
  delete ctx;
  if (s != nullptr) {
    (void)hipStreamDestroy(s);
  }
  if (repo != nullptr) {
    repo->release();
  }
  return LDPC_HIP_OK;
}

const char* ldpc_hip_last_error(const ldpc_hip_ctx* ctx) { return ctx == nullptr ? "null context" : ctx->err.c_str(); }

int ldpc_hip_capture_begin(ldpc_hip_ctx* ctx, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t      s = abi_stream(ctx->stream, stream);
  if (s == nullptr || s == hipStreamPerThread) {
    return ctx->fail(LDPC_HIP_EINVAL, "a default stream cannot be captured"); /* hipStreamBeginCapture refuses it */
  }
  const hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed);
  return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "hipStreamBeginCapture");
}

int ldpc_hip_capture_end(ldpc_hip_ctx* ctx, void* stream, ldpc_hip_graph** out)
{
  if (ctx == nullptr || out == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  *out          = nullptr;
  hipStream_t s = abi_stream(ctx->stream, stream);
  auto        g = std::make_unique<ldpc_hip_graph>();
  g->ctx        = ctx;
  hipError_t e  = hipStreamEndCapture(s, &g->graph);
  if (e == hipSuccess) {
    e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  }
  if (e != hipSuccess) {
    if (g->graph != nullptr) {
      (void)hipGraphDestroy(g->graph);
    }
    return ctx->hip_fail(e, "graph capture");
  }
  *out = g.release();
  return LDPC_HIP_OK;
}

int ldpc_hip_graph_launch(ldpc_hip_graph* g, void* stream)
{
  if (g == nullptr || g->exec == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  hipStream_t      s = abi_stream(g->ctx->stream, stream);
  const hipError_t e = hipGraphLaunch(g->exec, s);
  return e == hipSuccess ? LDPC_HIP_OK : g->ctx->hip_fail(e, "hipGraphLaunch");
}

int ldpc_hip_graph_destroy(ldpc_hip_graph* g)
{
  if (g == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (g->exec != nullptr) {
    (void)hipGraphExecDestroy(g->exec);
  }
  if (g->graph != nullptr) {
    (void)hipGraphDestroy(g->graph);
  }
  delete g;
  return LDPC_HIP_OK;
}

void* ldpc_hip_stream(ldpc_hip_ctx* ctx) { return ctx == nullptr ? nullptr : static_cast<void*>(ctx->stream); }

int ldpc_hip_schedule_groups(int bg, uint32_t lifting_size)
{
  graph_desc g;
  if (!build_graph(bg, lifting_size, g)) {
    return LDPC_HIP_EINVAL;
  }
  return g.n_groups;
}

int ldpc_hip_specialised(int bg, uint32_t lifting_size)
{
  graph_desc g;
  if (!build_graph(bg, lifting_size, g)) {
    return LDPC_HIP_EINVAL;
  }
  return spec_index(g, make_lds_layout(g, true)) >= 0 ? 1 : 0;
}

/* ---- plans ---- */
int ldpc_hip_decode_plan_create(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dec_desc* descs,
                                ldpc_hip_plan** plan)
{
  if (ctx == nullptr || plan == nullptr || (nof_cbs != 0 && descs == nullptr)) {
    return LDPC_HIP_EINVAL;
  }
  *plan  = nullptr;
  auto p = std::make_unique<ldpc_hip_plan>();
  (void)hipSetDevice(ctx->device);
  int r = build_plan(ctx, nof_cbs, descs, *p);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  *plan = p.release();
  return LDPC_HIP_OK;
}

int ldpc_hip_decode_plan_destroy(ldpc_hip_plan* plan)
{
  delete plan;
  return LDPC_HIP_OK;
}

int ldpc_hip_decode_launch(ldpc_hip_plan* plan, const int8_t* d_llr, uint8_t* d_out, ldpc_hip_cb_result* d_results,
                           void* stream)
{
  if (plan == nullptr || (plan->n != 0 && (d_llr == nullptr || d_out == nullptr))) {
    return LDPC_HIP_EINVAL;
  }
  hipStream_t s = abi_stream(plan->ctx->stream, stream);
  return launch_plan(*plan, d_llr, d_out, d_results, s);
}

int ldpc_hip_rate_dematch_scr_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dematch_desc* descs,
                                     const int8_t* d_llr, const uint64_t* llr_offsets,
                                     const ldpc_hip_demod_desc* demod, const float* d_symbols,
                                     const float* d_noise_vars, const ldpc_hip_scramble_desc* scr, int8_t* d_soft,
                                     const uint64_t* soft_offsets, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  if (demod == nullptr) {
    if (descs == nullptr || d_llr == nullptr || llr_offsets == nullptr || d_soft == nullptr ||
        soft_offsets == nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, "rate_dematch_launch: null argument");
    }
  } else if (descs == nullptr || d_symbols == nullptr || d_noise_vars == nullptr || d_soft == nullptr ||
             soft_offsets == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "demod_dematch_launch: null argument");
  }
  std::vector<dematch_cb> dm(nof_cbs);
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    const char* why = make_dematch_cb(descs[i], demod == nullptr ? d_llr + llr_offsets[i] : nullptr,
                                      d_soft + soft_offsets[i], demod != nullptr ? demod + i : nullptr, d_symbols,
                                      d_noise_vars, scr != nullptr ? scr + i : nullptr, nullptr, dm[i]);
    if (why != nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  return ctx->launch_items(ctx->d_dmdesc, dm, s,
                           demod != nullptr ? "ldpc_rate_dematch_kernel launch (demodulating)"
                                            : "ldpc_rate_dematch_kernel launch",
                           [&](const dematch_cb* d_cbs) { return launch_dematch(d_cbs, nof_cbs, ctx->dtab, s); });
}

int ldpc_hip_rate_dematch_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dematch_desc* descs,
                                 const int8_t* d_llr, const uint64_t* llr_offsets, int8_t* d_soft,
                                 const uint64_t* soft_offsets, void* stream)
{
  return ldpc_hip_rate_dematch_scr_launch(ctx, nof_cbs, descs, d_llr, llr_offsets, nullptr, nullptr, nullptr, nullptr,
                                          d_soft, soft_offsets, stream);
}

int ldpc_hip_demod_dematch_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dematch_desc* descs,
                                  const ldpc_hip_demod_desc* demod, const float* d_symbols,
                                  const float* d_noise_vars, int8_t* d_soft, const uint64_t* soft_offsets,
                                  void* stream)
{
  if (ctx != nullptr && nof_cbs != 0 && demod == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "demod_dematch_launch: null argument");
  }
  return ldpc_hip_rate_dematch_scr_launch(ctx, nof_cbs, descs, nullptr, nullptr, demod, d_symbols, d_noise_vars,
                                          nullptr, d_soft, soft_offsets, stream);
}

#ifdef LDPC_HIP_DIAG_CB
/* diagnostic build only: the decoder's per-workgroup phase stamps (tools/diag_cb.py) */
int ldpc_hip_diag_cb_read(ldpc_hip_ctx* ctx, uint64_t* out, uint32_t n)
{
  if (ctx == nullptr || n > DIAG_CB_WORDS / 2) {
    return LDPC_HIP_EINVAL;
  }
  (void)hipSetDevice(ctx->device);
  return hipMemcpy(out, ctx->d_crc.as<uint32_t>() + DIAG_CB_OFFSET, n * sizeof(uint64_t), hipMemcpyDeviceToHost) ==
                 hipSuccess ? LDPC_HIP_OK : LDPC_HIP_EDEVICE;
}
#endif

int ldpc_hip_dematch_decode_launch(ldpc_hip_plan* plan, const ldpc_hip_dematch_desc* descs, const int8_t* d_llr,
                                   const uint64_t* llr_offsets, const ldpc_hip_demod_desc* demod,
                                   const float* d_symbols, const float* d_noise_vars, int8_t* d_soft, uint8_t* d_out,
                                   ldpc_hip_cb_result* d_results, void* stream)
{
  return ldpc_hip_dematch_decode_scr_launch(plan, descs, d_llr, llr_offsets, demod, d_symbols, d_noise_vars, nullptr,
                                            d_soft, d_out, d_results, stream);
}

int ldpc_hip_dematch_decode_scr_launch(ldpc_hip_plan* plan, const ldpc_hip_dematch_desc* descs, const int8_t* d_llr,
                                       const uint64_t* llr_offsets, const ldpc_hip_demod_desc* demod,
                                       const float* d_symbols, const float* d_noise_vars,
                                       const ldpc_hip_scramble_desc* scr, int8_t* d_soft, uint8_t* d_out,
                                       ldpc_hip_cb_result* d_results, void* stream)
{
  if (plan == nullptr || plan->ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  ldpc_hip_ctx* ctx = plan->ctx;
  if (plan->n == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_soft == nullptr || d_out == nullptr || plan->h_cbs.size() != plan->n ||
      (demod == nullptr && (d_llr == nullptr || llr_offsets == nullptr)) ||
      (demod != nullptr && (d_symbols == nullptr || d_noise_vars == nullptr))) {
    return ctx->fail(LDPC_HIP_EINVAL, "dematch_decode_launch: null argument");
  }
  std::vector<dematch_cb> dm(plan->n); /* block order: block i dematches caller descriptor h_cbs[i].result_index */
  for (uint32_t i = 0; i != plan->n; ++i) {
    const dec_cb&  cb  = plan->h_cbs[i];
    const uint32_t k   = cb.result_index;
    const char*    why = make_dematch_cb(descs[k], demod == nullptr ? d_llr + llr_offsets[k] : nullptr,
                                         d_soft + cb.llr_offset, demod != nullptr ? demod + k : nullptr, d_symbols,
                                         d_noise_vars, scr != nullptr ? scr + k : nullptr, &cb, dm[i]);
    if (why != nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  const uint32_t   dm_lds = dm_fused_budget(dm.data(), dm.size());
  hipStream_t      hs = abi_stream(ctx->stream, stream);
  const hipError_t e  = plan->d_dm.upload(dm.data(), dm.size() * sizeof(dematch_cb), hs);
  if (e != hipSuccess) {
    return ctx->hip_fail(e, "dematch_decode_launch: descriptors");
  }
  return launch_plan(*plan, d_soft, d_out, d_results, hs, plan->d_dm.as<dematch_cb>(), nullptr, dm_lds);
}

int ldpc_hip_encode_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_enc_desc* descs, const uint8_t* d_msgs,
                           uint8_t* d_cws, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_msgs == nullptr || d_cws == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "encode_launch: null argument");
  }
  std::vector<enc_cb> e(nof_cbs);
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    const char* why = make_enc_cb(descs[i], nullptr, e[i]);
    if (why != nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  return ctx->launch_items(ctx->d_encdesc, e, s, "ldpc_encode_kernel launch", [&](const enc_cb* d_cbs) {
    return launch_encode(d_cbs, nof_cbs, d_msgs, d_cws, ctx->d_crc.as<uint32_t>(), s);
  });
}

int ldpc_hip_rate_match_launch(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_rm_desc* descs,
                               const uint8_t* d_cws, uint8_t* d_out, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_cws == nullptr || d_out == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "rate_match_launch: null argument");
  }
  std::vector<ratematch_cb> r(nof_cbs);
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    const char* why = make_rm_cb(descs[i], r[i]);
    if (why != nullptr) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  return ctx->launch_items(ctx->d_rmdesc, r, s, "ldpc_rate_match_kernel launch", [&](const ratematch_cb* d_cbs) {
    return launch_rate_match(d_cbs, nof_cbs, d_cws, d_out, s);
  });
}

int ldpc_hip_tb_join_launch(ldpc_hip_ctx* ctx, uint32_t nof_tbs, const ldpc_hip_tb_desc* descs, const uint8_t* d_msgs,
                            ldpc_hip_cb_result* d_cb_results, uint8_t* d_tb, ldpc_hip_tb_result* d_tb_results,
                            void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_tbs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_msgs == nullptr || d_cb_results == nullptr || d_tb == nullptr || d_tb_results == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "tb_join: null argument");
  }
  for (uint32_t i = 0; i != nof_tbs; ++i) {
    if (const char* why = tb_desc_reason(descs[i])) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  std::vector<tbj_block> blocks; /* per workgroup: its TB's descriptor, the TB index and the chunk */
  for (uint32_t i = 0; i != nof_tbs; ++i) {
    const uint32_t nch = (descs[i].tbs / 8U + TBJ_CHUNK - 1) / TBJ_CHUNK;
    for (uint32_t c = 0; c != nch; ++c) {
      blocks.push_back(tbj_block{descs[i], i, c});
    }
  }
  const uint32_t nblocks = static_cast<uint32_t>(blocks.size());
  hipError_t     e       = ctx->d_tbaux.upload(blocks.data(), nblocks * sizeof(tbj_block), s);
  const size_t work_bytes = static_cast<size_t>(nof_tbs) * TBJ_WORK_WORDS * 4;
  if (e == hipSuccess && ctx->d_tbwork.size < work_bytes) {
    /* arrival counters start at zero; the kernel returns each to zero after its TB */
    if ((e = hipStreamSynchronize(s)) == hipSuccess && (e = ctx->d_tbwork.reserve(work_bytes)) == hipSuccess) {
      e = hipMemsetAsync(ctx->d_tbwork.ptr, 0, ctx->d_tbwork.size, s);
    }
  }
  if (e == hipSuccess) {
    e = launch_tb_join(ctx->d_tbaux.as<tbj_block>(), nblocks, d_msgs, d_cb_results, d_tb, d_tb_results,
                       ctx->d_crc.as<uint32_t>(), ctx->d_tbwork.as<uint32_t>(), s);
  }
  return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "ldpc_tb_join_kernel launch");
}

int ldpc_hip_demodulate_launch(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_demod_desc* descs,
                               const float* d_symbols, const float* d_noise_vars, int8_t* d_llrs, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_segs == 0) {
    return LDPC_HIP_OK;
  }
  if (descs == nullptr || d_symbols == nullptr || d_noise_vars == nullptr || d_llrs == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "demodulate_launch: null argument");
  }
  (void)hipSetDevice(ctx->device);
  hipStream_t s = abi_stream(ctx->stream, stream);
  return demodulate_segments(ctx, nof_segs, descs, d_symbols, d_noise_vars, d_llrs, s);
}

int ldpc_hip_prs_init(uint32_t c_init, uint64_t offset, ldpc_hip_prs_state* state)
{
  if (state == nullptr || (c_init & ~PRS_MASK) != 0U) {
    return LDPC_HIP_EINVAL;
  }
  *state = prs_state_at(c_init, offset);
  return LDPC_HIP_OK;
}

int ldpc_hip_descramble_launch(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_prs_seg* segs, const int8_t* d_in,
                               int8_t* d_out, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_segs == 0) {
    return LDPC_HIP_OK;
  }
  if (segs == nullptr || d_in == nullptr || d_out == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "descramble_launch: null argument");
  }
  (void)hipSetDevice(ctx->device);
  return prs_segments(ctx, nof_segs, segs, false, reinterpret_cast<const uint8_t*>(d_in),
                      reinterpret_cast<uint8_t*>(d_out), abi_stream(ctx->stream, stream));
}

int ldpc_hip_scramble_bits_launch(ldpc_hip_ctx* ctx, uint32_t nof_segs, const ldpc_hip_prs_seg* segs,
                                  const uint8_t* d_in, uint8_t* d_out, void* stream)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_segs == 0) {
    return LDPC_HIP_OK;
  }
  if (segs == nullptr || d_out == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "scramble_bits_launch: null argument");
  }
  (void)hipSetDevice(ctx->device);
  return prs_segments(ctx, nof_segs, segs, true, d_in, d_out, abi_stream(ctx->stream, stream));
}

} /* extern "C" */
