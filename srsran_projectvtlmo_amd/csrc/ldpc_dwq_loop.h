/*
 * The persistent loop of a work-queue kernel (dwq_loop): every kernel unit's work-queue kernels run their body in it.
 */
#pragma once

#include "ldpc_device_util.h"

namespace ldpc_hip {

/* ---- device work queue: the persistent loop of a unit's grid (ldpc_hip_dwq.cpp) ------------------------------------
 * Wave 0 of a workgroup polls the ring slot of the next ticket, `next` (its view of the device claim counter): one
 * round trip reads the slot's 48 words (lanes 0-47) and the host's stop word (lane 48) from pinned memory. A slot whose
 * three sequence words equal next + 1 holds a published item; lane 0 claims it with a device-scope CAS of the claim
 * counter (next -> next + 1), and the item, already in registers, goes to LDS. A failed CAS returns the counter's
 * value, which becomes `next` (another workgroup claimed it). Only published items are ever claimed, so a workgroup
 * that leaves never strands one. Idle workgroups poll in turns (workgroup b in the 0.25 us slots where
 * (t / slot) mod grid = b: one slot read per 0.25 us for the grid); a workgroup that has just finished an item polls
 * twice at once, and one that lost a claim polls again at once, so back-to-back work does not wait for a turn
 * (polling freely for 20 us after seeing work, measured in round 4, cost more PCIe and host-cache traffic than it
 * saved, profiles/r04/route_ab_eager_v1.json). The body runs (fused
 * dematch + specialised decode, or a dematch alone), every wave drains its stores, and after a barrier lane 0 makes the
 * workgroup's writes visible system-wide (release fence: the HARQ soft bits in HBM for the next transmission's
 * workgroup on any XCD, the results in pinned host memory) and stores the done flag. Every wave leaves the loop
 * together: after idle_ticks without work, after life_ticks in all, or on stop; the host relaunches a grid when it
 * finds work unclaimed and the grid gone (ldpc_hip_dwq.cpp). Every spin is bounded. */
constexpr uint32_t DWQ_NONE = 0xffffffffU;
template <class BODY>
__device__ __forceinline__ void dwq_loop(const dwq_args& a, BODY&& body)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  /* control words: [0] claimed ticket, [1] stop, [2] ticks from t0 to the claim, [3] / [4] t0; the item from [8] */
  uint32_t* s_ctl  = reinterpret_cast<uint32_t*>(smem + a.ctl_lds);
  uint32_t* s_item = s_ctl + 8;
  const int tid    = threadIdx.x;
  const int lane   = tid & 63;
  uint64_t  t0     = __builtin_amdgcn_s_memrealtime();
  uint64_t  last   = t0;
  uint32_t  next   = 0; /* wave 0: the next ticket to poll */
  uint32_t  quick  = 0; /* wave 0: polls left outside the turns (the first ones after an item) */
  if (tid == 0) {
    s_ctl[3] = static_cast<uint32_t>(t0);
    s_ctl[4] = static_cast<uint32_t>(t0 >> 32);
  }
  if (tid < 64) {
    next = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(
        __hip_atomic_load(a.dev_ctl + DWQ_D_CLAIMED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))));
  }
#ifdef LDPC_HIP_DIAG_DWQ /* diagnostic build: lane 0's 100 MHz stamps of each item, into dead words of its slot */
  uint64_t t_claim = 0;
#endif
  while (true) {
    if (tid < 64) {
      uint32_t       claim = DWQ_NONE, stop = 0;
      const uint64_t tin   = __builtin_amdgcn_s_memrealtime();
      while (claim == DWQ_NONE && stop == 0U) {
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (now - tin > 1000U) { /* 10 us: back to the idle / lifetime checks */
          break;
        }
        if (quick == 0U) {
          const uint32_t slot = static_cast<uint32_t>(now / a.slot_ticks);
          const uint32_t ahead = (blockIdx.x + gridDim.x - slot % gridDim.x) % gridDim.x; /* slots to this turn */
          if (ahead != 0U) {
            if ((a.poll_flags & DWQ_POLL_LONG_SLEEP) != 0U && ahead * a.slot_ticks > 100U) {
              __builtin_amdgcn_s_sleep(32); /* ~2,048 cycles, ~0.85 us at 2.4 GHz */
            } else {
              __builtin_amdgcn_s_sleep(2);
            }
            continue;
          }
        }
        quick = quick != 0U ? quick - 1U : 0U;
        const uint32_t* sw = a.ring + (next & a.ring_mask) * DWQ_WIRE_WORDS;
        uint32_t        w  = 0;
        if (lane < static_cast<int>(DWQ_WIRE_WORDS)) {
          w = __hip_atomic_load(sw + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else if (lane == static_cast<int>(DWQ_WIRE_WORDS)) {
          w = __hip_atomic_load(a.host_ctl + DWQ_H_STOP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        auto lane_word = [&](int l) {
          return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(w), l));
        };
        stop                = lane_word(DWQ_WIRE_WORDS);
        if (stop != 0U || (a.poll_flags & DWQ_POLL_TEST_NO_CLAIM) != 0U) {
          /* a stopped grid claims nothing more (a timed-out wait on the host stops it and then takes its exit as the
           * point after which no item of the queue can touch the caller's buffers, dwq_wait) */
          continue;
        }
        const uint32_t want = next + 1U;
        /* the checksum of payload words 0-43 (lane l carries payload word l - l / 16) against word 44 (lane 46) */
        const int      pw   = lane - (lane >> 4);
        const uint32_t mx   = (lane < static_cast<int>(DWQ_WIRE_WORDS) && (lane & 15) != 15 && pw < 44)
                                  ? dwq_mix(w, static_cast<uint32_t>(pw)) : 0U;
        const uint32_t sum  = wave_xor(mx);
        if (lane_word(15) == want && lane_word(31) == want && lane_word(47) == want && sum == lane_word(46)) {
          uint32_t exp = next;
          uint32_t ok  = 0;
          if (lane == 0) {
            /* relaxed: the item is already in registers (validated by its sequence words), the previous item's
             * writes were released with its done flag, and the acquire for the HARQ memory follows the claim; an
             * acq_rel CAS wrote back and invalidated the L2 around it on every claim */
            ok = __hip_atomic_compare_exchange_strong(a.dev_ctl + DWQ_D_CLAIMED, &exp, next + 1U, __ATOMIC_RELAXED,
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                     ? 1U
                     : 0U;
          }
          ok  = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ok)));
          exp = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(exp)));
          if (ok != 0U) {
            claim = next;
            next  = next + 1U;
            if (lane < static_cast<int>(DWQ_WIRE_WORDS) && (lane & 15) != 15) {
              s_item[lane - (lane >> 4)] = w;
            } else if (lane >= 61) {
              s_item[DWQ_WIRE_PAYLOAD + (lane - 61)] = 0; /* pad[1..3] */
            }
          } else {
            next  = exp; /* another workgroup claimed it: poll the counter's next ticket at once */
            quick = quick != 0U ? quick : 1U;
          }
          continue;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      if (claim != DWQ_NONE) {
        /* the HARQ soft bits an earlier item left in HBM, possibly from another XCD's L2, and the host's new inputs
         * in pinned staging this CU's vector cache may hold from an earlier item (a timing variant without this
         * acquire decoded stale LLRs) */
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      const uint64_t now = __builtin_amdgcn_s_memrealtime();
#ifdef LDPC_HIP_DIAG_DWQ
      t_claim = now;
#endif
      if (lane == 0) {
        s_ctl[0] = claim;
        s_ctl[1] = stop;
        s_ctl[2] = static_cast<uint32_t>(now - t0);
      }
    }
    __syncthreads();
    const uint32_t claim   = s_ctl[0];
    const uint32_t stop    = s_ctl[1];
    const uint64_t elapsed = s_ctl[2];
    if (claim == DWQ_NONE) {
      __syncthreads(); /* every wave has read the control words before wave 0 writes them again */
      if (stop != 0U || elapsed - (last - t0) > a.idle_ticks || elapsed > a.life_ticks) {
        break;
      }
      continue;
    }
    /* The item's words go to scalar registers (the launched kernel's descriptor comes from the kernel arguments into
     * SGPRs as well): a vector-register copy lived across the body and made the BG1 bodies spill. Nothing of the loop
     * lives in registers across the body: its state is rebuilt from the control words after it. */
    uint32_t words[DWQ_ITEM_WORDS];
    for (uint32_t k = 0; k != DWQ_ITEM_WORDS; ++k) {
      words[k] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_item[k])));
    }
    /* memcpy, not stores through a uint32_t* into the struct: its 64-, 16- and 8-bit fields read back after such
     * stores are not ordered after them under type-based alias analysis (a loop-carried `it` then handed the body some
     * fields of the workgroup's previous item: wrong decodes of successive calls with different lengths) */
    dwq_item it;
    __builtin_memcpy(&it, words, sizeof(it));
#ifdef LDPC_HIP_DIAG_DWQ
    const uint64_t t_item = __builtin_amdgcn_s_memrealtime();
#endif
    if (it.spec != DWQ_SPEC_NOOP) {
      body(it);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint32_t done_claim = s_ctl[0];
    t0    = (static_cast<uint64_t>(s_ctl[4]) << 32) | s_ctl[3];
    last  = t0 + s_ctl[2];
    next  = done_claim + 1U;
    quick = 2U; /* a workgroup done with an item looks at the next ticket at once (back-to-back work), twice */
    if (tid == 0) {
#ifdef LDPC_HIP_DIAG_DWQ
      uint32_t* pw = const_cast<uint32_t*>(a.ring + (claim & a.ring_mask) * DWQ_WIRE_WORDS);
      pw[44]       = static_cast<uint32_t>(t_claim);
      pw[45]       = static_cast<uint32_t>(t_item - t_claim);
      pw[46]       = static_cast<uint32_t>(__builtin_amdgcn_s_memrealtime() - t_claim);
      pw[14]       = blockIdx.x;
#endif
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(a.done + (done_claim & a.ring_mask), done_claim + 1U, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  /* the grid's last workgroup to leave tells the host (ldpc_hip_dwq.cpp ensure_running: no runtime query per submit) */
  if (tid == 0) {
    const uint32_t n = __hip_atomic_fetch_add(a.dev_ctl + DWQ_D_EXITS, 1U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n + 1U == a.exit_target) {
      __hip_atomic_store(a.host_exit, a.exit_target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

} // namespace ldpc_hip
