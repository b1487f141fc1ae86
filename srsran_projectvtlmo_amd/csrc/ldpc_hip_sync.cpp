/*
 * The synchronous entry points of the C ABI (include/srsran_ldpc_hip.h): host buffers in, host buffers out, the call
 * returns when the result is there. One codeblock takes the software route's zero-copy path (one_cb_call); more go
 * through the context's device scratch with one copy per direction.
 */
#include <immintrin.h>

#include <cstring>

#include "ldpc_hip_ctx.h"
#include "ldpc_hip_launch.h"

using namespace ldpc_hip;

namespace {

/* Waits for the context's sync event by polling (a blocking synchronize may sleep in the driver and wake late; the
 * software route's calls take tens of microseconds). */
hipError_t spin_event(hipEvent_t ev)
{
  hipError_t q;
  while ((q = hipEventQuery(ev)) == hipErrorNotReady) {
  }
  return q;
}

/* What the two one-CB calls stage and how their errors read. */
struct one_cb_staging {
  const char*   what;      /* "sync decode" / "rate dematch": names the call in its errors                     */
  const char*   launched;  /* names the launch path's event wait                                                */
  const int8_t* llr;       /* the call's LLRs, llr_len of them: into s_bar, else s_in                           */
  size_t        llr_len;
  size_t        in_bytes;  /* s_in as the call needs it (the LLRs, and whatever it places behind them)         */
  size_t        out_bytes; /* s_out as the call needs it; 0: not used                                          */
  bool          optional;  /* without pinned staging the call has another way: returns ONE_CB_NO_STAGING       */
};
constexpr int ONE_CB_NO_STAGING = 1;

/* The software route's call for one codeblock (pusch_codeblock_decoder.cpp:42-62, one per CB and worker thread): the
 * LLRs are copied into device memory through the BAR (else into the context's pinned staging buffer), the kernel reads
 * them there and works on pinned memory in place (no DMA either way, descriptor by value), as an item of a device work
 * queue or, when no queue can take it, as a launch whose event the caller spins on.
 * item(llr_dev, it): stages the rest of the call's input, fills the work item and returns its queue (nullptr: launch).
 * launch(llr_dev): the same work as a launch on the context's stream. The outputs are in place on LDPC_HIP_OK. */
template <class Item, class Launch>
int one_cb_call(ldpc_hip_ctx* ctx, const one_cb_staging& st, Item&& item, Launch&& launch)
{
  hipError_t e;
  if (ctx->staging_lost) {
    return ctx->hip_fail(hipErrorLaunchTimeOut, std::string(st.what) + ": a stalled work-queue grid may still write "
                                                                       "this context's staging; close the context");
  }
  if ((e = ctx->s_in.reserve(st.in_bytes, 0)) != hipSuccess ||
      (st.out_bytes != 0 && (e = ctx->s_out.reserve(st.out_bytes, 0)) != hipSuccess) || ctx->s_in.dev == nullptr ||
      (st.out_bytes != 0 && ctx->s_out.dev == nullptr)) {
    if (st.optional) {
      (void)hipGetLastError();
      return ONE_CB_NO_STAGING;
    }
    return ctx->hip_fail(e != hipSuccess ? e : hipErrorInvalidValue, std::string("pinned staging (") + st.what + ")");
  }
  /* the LLRs into the BAR staging, else into s_in */
  const int8_t* llr_dev = ctx->s_in.dev_as<int8_t>();
  if (st.llr_len != 0) {
    if (!ctx->bar_failed && ctx->s_bar.reserve(st.llr_len) == hipSuccess) {
      std::memcpy(ctx->s_bar.ptr, st.llr, st.llr_len);
      llr_dev = ctx->s_bar.dev_as<int8_t>();
    } else {
      ctx->bar_failed = true;
      std::memcpy(ctx->s_in.ptr, st.llr, st.llr_len);
    }
  }
  dwq_item it{};
  dwq*     q = item(llr_dev, it);
  _mm_sfence(); /* the write-combined LLR stores before the hand-off */
  if (q != nullptr) {
    uint32_t ticket = 0;
    e               = dwq_submit(q, it, ticket, true);
    if (e != hipErrorLaunchOutOfResources) { /* refused (residency budget spent): nothing published, launch below */
      if (e != hipSuccess || (e = dwq_wait(q, ticket)) != hipSuccess) {
        ctx->staging_lost = ctx->staging_lost || !dwq_quiesced(q);
        return ctx->hip_fail(e, std::string("work queue (") + st.what + ")");
      }
      return LDPC_HIP_OK;
    }
  }
  const int r = launch(llr_dev);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  if ((e = hipEventRecord(ctx->sync_event, ctx->stream)) != hipSuccess || (e = spin_event(ctx->sync_event)) != hipSuccess) {
    return ctx->hip_fail(e, st.launched);
  }
  return LDPC_HIP_OK;
}

/* ldpc_decoder::decode of one codeblock from host memory: the message and result come back in s_out. */
int decode_one_zero_copy(ldpc_hip_ctx* ctx, const ldpc_hip_dec_desc& desc, const int8_t* llr, uint8_t* out,
                         ldpc_hip_cb_result* result)
{
  dwq_diag_entry();
  ldpc_hip_dec_desc d = desc;
  d.llr_offset        = 0;
  d.out_offset        = 0;
  dec_cb one{};
  if (const char* why = make_dec_cb(d, one)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  /* The decoder works up to the last non-zero LLR (ldpc_decoder_impl.cpp:85-112: layers and length follow it, and the
   * soft bits past it are zero), so the trailing zeros of the caller's soft buffer (a rate-dematched codeblock shorter
   * than N) need not cross PCIe: the call stages and passes the buffer up to its last non-zero 32-byte block, never
   * below the minimum length (K + 2) Z. */
  {
    const uint32_t lmin = (d.base_graph == 1 ? 24U : 12U) * d.lifting_size;
    uint32_t       n    = d.llr_length;
    while (n >= lmin + 32U) {
      uint64_t w[4];
      std::memcpy(w, llr + n - 32U, sizeof(w));
      if ((w[0] | w[1] | w[2] | w[3]) != 0) {
        break;
      }
      n -= 32U;
    }
    d.llr_length = one.llr_length = n;
  }
  const unsigned mb    = msg_bytes_of(d.base_graph, d.lifting_size);
  const size_t   res_o = align16(mb);
  const int      slot  = graph_slot(d.base_graph, d.lifting_size);
  const auto     res_dev = [&] { return reinterpret_cast<ldpc_hip_cb_result*>(ctx->s_out.dev_as<uint8_t>() + res_o); };
  const one_cb_staging st{"sync decode", "sync decode", llr, d.llr_length, d.llr_length,
                          res_o + sizeof(ldpc_hip_cb_result), false};
  const int r = one_cb_call(
      ctx, st,
      [&](const int8_t* llr_dev, dwq_item& it) -> dwq* {
        /* the device work queue of the graph's specialised body (the default scaling factor only): no plan and no
         * launch at all */
        if (!ctx->use_dwq || one.scaling_factor != 0.8f || ctx->graph_spec[slot] == 0) {
          return nullptr;
        }
        const int sid = ctx->graph_spec[slot] - 1;
        it.cb         = one;
        it.lay        = ctx->spec_lay[slot];
        it.llr_base   = llr_dev;
        it.out_base   = ctx->s_out.dev_as<uint8_t>();
        it.res_base   = res_dev();
        it.crc_tables = ctx->d_crc.as<uint32_t>();
        it.spec       = static_cast<uint32_t>(sid + 1);
        return dwq_get(ctx->device, 1 + sid, ctx->key_block[1 + sid], ctx->key_lds[1 + sid]);
      },
      [&](const int8_t* llr_dev) {
        ldpc_hip_plan            plan;
        std::vector<dec_cb>      cbs;
        std::vector<mixed_group> mg;
        const int                pr = plan_host(ctx, 1, &d, plan, cbs, mg);
        if (pr != LDPC_HIP_OK) {
          return pr;
        }
        plan.has_one = true;
        plan.one     = cbs[0];
        plan.cbs_dev = nullptr;
        return launch_plan(plan, llr_dev, ctx->s_out.dev_as<uint8_t>(), res_dev(), ctx->stream);
      });
  if (r != LDPC_HIP_OK) {
    return r;
  }
  const ldpc_hip_cb_result res = *reinterpret_cast<const ldpc_hip_cb_result*>(ctx->s_out.as<uint8_t>() + res_o);
  if (res.status & LDPC_HIP_STATUS_OUTPUT_WRITTEN) {
    std::memcpy(out, ctx->s_out.ptr, mb);
  }
  if (result != nullptr) {
    *result = res;
  }
  return LDPC_HIP_OK;
}

/* ldpc_rate_dematcher::rate_dematch of one codeblock: the old soft bits behind the LLRs in s_in, combined in place.
 * ONE_CB_NO_STAGING: nothing done, the caller takes the copy path. */
int dematch_one_zero_copy(ldpc_hip_ctx* ctx, const ldpc_hip_dematch_desc& s, int8_t* soft, const int8_t* llr)
{
  dwq_diag_entry();
  dematch_cb one{};
  if (const char* why = make_dematch_cb(s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, one)) {
    return ctx->fail(LDPC_HIP_EINVAL, why);
  }
  const size_t         soft_o = align16(s.rm_length);
  const one_cb_staging st{"rate dematch", "rate dematch (one CB)", llr, s.rm_length, soft_o + s.cb_length, 0, true};
  const int r = one_cb_call(
      ctx, st,
      [&](const int8_t* llr_dev, dwq_item& it) -> dwq* {
        /* the old soft bits also on new data: positions the dematcher does not write keep them (the limited-buffer
         * gap between the last written index and the zeroed tail, ldpc_rate_dematcher_impl.cpp:197-200); the host
         * reads them back, so they stay in pinned memory */
        std::memcpy(ctx->s_in.as<int8_t>() + soft_o, soft, s.cb_length);
        one.llr       = llr_dev;
        one.soft      = ctx->s_in.dev_as<int8_t>() + soft_o;
        it.dm         = one;
        it.crc_tables = ctx->d_crc.as<uint32_t>();
        it.spec       = 0;
        /* the dematch-only work queue */
        return ctx->use_dwq ? dwq_get(ctx->device, 0, ctx->key_block[0], ctx->key_lds[0]) : nullptr;
      },
      [&](const int8_t*) {
        const hipError_t e = launch_dematch(nullptr, 1, ctx->dtab, ctx->stream, &one);
        return e == hipSuccess ? LDPC_HIP_OK : ctx->hip_fail(e, "rate dematch (one CB)");
      });
  if (r == LDPC_HIP_OK) {
    std::memcpy(soft, ctx->s_in.as<int8_t>() + soft_o, s.cb_length);
  }
  return r;
}

} // namespace

extern "C" {

int ldpc_hip_decode_sync(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dec_desc* descs,
                         const int8_t* const* llrs, uint8_t* const* outs, ldpc_hip_cb_result* results)
{
  if (ctx == nullptr || (nof_cbs != 0 && (descs == nullptr || llrs == nullptr || outs == nullptr))) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  (void)hipSetDevice(ctx->device);
  if (nof_cbs == 1 && ctx->sync_zc && ctx->s_in.dev != nullptr) {
    return decode_one_zero_copy(ctx, descs[0], llrs[0], outs[0], results);
  }
  std::vector<ldpc_hip_dec_desc> d(descs, descs + nof_cbs);
  uint64_t                       llr_total = 0, out_total = 0;
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    d[i].llr_offset = llr_total;
    d[i].out_offset = out_total;
    llr_total += align16(d[i].llr_length);
    out_total += align16(msg_bytes_of(d[i].base_graph, d[i].lifting_size));
  }
  ldpc_hip_plan plan;
  int           r = build_plan(ctx, nof_cbs, d.data(), plan);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  hipError_t e;
  if ((e = ctx->d_llr.reserve(llr_total)) != hipSuccess || (e = ctx->d_out.reserve(out_total)) != hipSuccess ||
      (e = ctx->d_res.reserve(nof_cbs * sizeof(ldpc_hip_cb_result))) != hipSuccess) {
    return ctx->hip_fail(e, "hipMalloc(sync decode)");
  }
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    e = hipMemcpyAsync(ctx->d_llr.as<int8_t>() + d[i].llr_offset, llrs[i], d[i].llr_length, hipMemcpyHostToDevice,
                       ctx->stream);
    if (e != hipSuccess) {
      return ctx->hip_fail(e, "hipMemcpyAsync(llr)");
    }
  }
  r = launch_plan(plan, ctx->d_llr.as<int8_t>(), ctx->d_out.as<uint8_t>(), ctx->d_res.as<ldpc_hip_cb_result>(),
                  ctx->stream);
  if (r != LDPC_HIP_OK) {
    return r;
  }
  std::vector<ldpc_hip_cb_result> res(nof_cbs);
  std::vector<uint8_t>            host_out(out_total);
  if ((e = hipMemcpyAsync(res.data(), ctx->d_res.ptr, nof_cbs * sizeof(ldpc_hip_cb_result), hipMemcpyDeviceToHost,
                          ctx->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(host_out.data(), ctx->d_out.ptr, out_total, hipMemcpyDeviceToHost, ctx->stream)) !=
          hipSuccess ||
      (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "sync decode");
  }
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    if (res[i].status & LDPC_HIP_STATUS_OUTPUT_WRITTEN) {
      std::memcpy(outs[i], host_out.data() + d[i].out_offset, msg_bytes_of(d[i].base_graph, d[i].lifting_size));
    }
    if (results != nullptr) {
      results[i] = res[i];
    }
  }
  return LDPC_HIP_OK;
}

int ldpc_hip_rate_dematch_sync(ldpc_hip_ctx* ctx, uint32_t nof_cbs, const ldpc_hip_dematch_desc* descs,
                               int8_t* const* soft_bufs, const int8_t* const* llrs)
{
  if (ctx == nullptr || (nof_cbs != 0 && (descs == nullptr || soft_bufs == nullptr || llrs == nullptr))) {
    return LDPC_HIP_EINVAL;
  }
  if (nof_cbs == 0) {
    return LDPC_HIP_OK;
  }
  (void)hipSetDevice(ctx->device);
  if (nof_cbs == 1 && ctx->sync_zc) {
    const int r = dematch_one_zero_copy(ctx, descs[0], soft_bufs[0], llrs[0]);
    if (r != ONE_CB_NO_STAGING) {
      return r;
    }
  }
  uint64_t                llr_total = 0, soft_total = 0;
  std::vector<uint64_t>   lo(nof_cbs), so(nof_cbs);
  std::vector<dematch_cb> dm(nof_cbs); /* llr / soft once the scratch has its size */
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    if (const char* why = make_dematch_cb(descs[i], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          dm[i])) {
      return ctx->fail(LDPC_HIP_EINVAL, why);
    }
    lo[i] = llr_total;
    so[i] = soft_total;
    llr_total += align16(descs[i].rm_length);
    soft_total += align16(descs[i].cb_length);
  }
  hipError_t e;
  if ((e = ctx->d_llr.reserve(std::max<uint64_t>(llr_total, 16))) != hipSuccess ||
      (e = ctx->d_soft.reserve(soft_total)) != hipSuccess ||
      (e = ctx->d_desc.reserve(nof_cbs * sizeof(dematch_cb))) != hipSuccess) {
    return ctx->hip_fail(e, "hipMalloc(dematch)");
  }
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    const ldpc_hip_dematch_desc& s = descs[i];
    dm[i].llr                      = ctx->d_llr.as<int8_t>() + lo[i];
    dm[i].soft                     = ctx->d_soft.as<int8_t>() + so[i];
    if (s.rm_length != 0 &&
        (e = hipMemcpyAsync(ctx->d_llr.as<int8_t>() + lo[i], llrs[i], s.rm_length, hipMemcpyHostToDevice,
                            ctx->stream)) != hipSuccess) {
      return ctx->hip_fail(e, "hipMemcpyAsync(llr)");
    }
    if ((e = hipMemcpyAsync(ctx->d_soft.as<int8_t>() + so[i], soft_bufs[i], s.cb_length, hipMemcpyHostToDevice,
                            ctx->stream)) != hipSuccess) {
      return ctx->hip_fail(e, "hipMemcpyAsync(soft)");
    }
  }
  if ((e = hipMemcpyAsync(ctx->d_desc.ptr, dm.data(), nof_cbs * sizeof(dematch_cb), hipMemcpyHostToDevice,
                          ctx->stream)) != hipSuccess ||
      (e = launch_dematch(ctx->d_desc.as<dematch_cb>(), nof_cbs, ctx->dtab, ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "rate dematch launch");
  }
  for (uint32_t i = 0; i != nof_cbs; ++i) {
    if ((e = hipMemcpyAsync(soft_bufs[i], ctx->d_soft.as<int8_t>() + so[i], descs[i].cb_length,
                            hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) {
      return ctx->hip_fail(e, "hipMemcpyAsync(soft out)");
    }
  }
  if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
    return ctx->hip_fail(e, "rate dematch sync");
  }
  return LDPC_HIP_OK;
}

int ldpc_hip_demodulate_sync(ldpc_hip_ctx* ctx, uint32_t nof_symbols, int modulation, const float* symbols,
                             const float* noise_vars, int8_t* llrs)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (!valid_modulation(modulation)) {
    return ctx->fail(LDPC_HIP_EINVAL, "demodulate: invalid modulation scheme");
  }
  if (nof_symbols == 0) {
    return LDPC_HIP_OK;
  }
  if (symbols == nullptr || noise_vars == nullptr || llrs == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "demodulate_sync: null argument");
  }
  (void)hipSetDevice(ctx->device);
  const size_t        n = nof_symbols;
  ldpc_hip_demod_desc d{};
  d.nof_symbols = nof_symbols;
  d.modulation  = static_cast<uint8_t>(modulation);
  return ctx->sync_round_trip("demodulate",
                              {to_device(ctx->d_sym, 0, symbols, n * 8), to_device(ctx->d_nv, 0, noise_vars, n * 4),
                               to_host(ctx->d_llr, 0, llrs, n * bits_per_symbol(modulation))},
                              [&] {
                                return demodulate_segments(ctx, 1, &d, ctx->d_sym.as<float>(), ctx->d_nv.as<float>(),
                                                           ctx->d_llr.as<int8_t>(), ctx->stream);
                              });
}

int ldpc_hip_descramble_sync(ldpc_hip_ctx* ctx, uint32_t c_init, uint64_t seq_offset, uint32_t n, const int8_t* in,
                             int8_t* out)
{
  if (ctx == nullptr) {
    return LDPC_HIP_EINVAL;
  }
  if (n == 0) {
    return LDPC_HIP_OK;
  }
  if (in == nullptr || out == nullptr) {
    return ctx->fail(LDPC_HIP_EINVAL, "descramble_sync: null argument");
  }
  (void)hipSetDevice(ctx->device);
  ldpc_hip_prs_seg d{};
  d.seq_offset = seq_offset;
  d.length     = n;
  d.c_init     = c_init;
  /* in place in d_llr */
  return ctx->sync_round_trip("descramble", {to_device(ctx->d_llr, 0, in, n), to_host(ctx->d_llr, 0, out, n)}, [&] {
    return prs_segments(ctx, 1, &d, false, ctx->d_llr.as<uint8_t>(), ctx->d_llr.as<uint8_t>(), ctx->stream);
  });
}

} /* extern "C" */
