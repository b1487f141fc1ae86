/*
 * Diagnostic builds only (make diag / make exp FLAGS=-DLDPC_HIP_DIAG_...; tools/diag_*.py read the stamps): the stamp
 * storage and the stamp macros of every kernel, in one place. In the product build every macro here expands to
 * nothing and there is no storage.
 *
 *  LDPC_HIP_DIAG (+ _FULL)  decoder: s_memtime per step barrier (g_diag) and per (step, wave) (g_diag2, SPEC_STAMP)
 *  LDPC_HIP_DIAG_PHASE      generic row update: s_memtime at its phase boundaries (PHASE, g_diag2)
 *  LDPC_HIP_DIAG_CB (+ _DM) decode_cb (and the fused dematcher): 100 MHz stamps per workgroup in the context's table
 *                           buffer, which every unit's kernels reach (CB_STAMP, DM_STAMP; ldpc_hip_diag_cb_read)
 *  LDPC_HIP_DIAG_DM, _TBJ   rate dematcher, TB join: 100 MHz stamps per workgroup (g_diag2[block * 8 + k])
 *  LDPC_HIP_DIAG_DWQ        the work-queue loop's stamps go into the item's ring slot (ldpc_dwq_loop.h)
 *
 * g_diag and g_diag2 are static: each kernel unit that includes this header in such a build has its own copy, written
 * by its own kernels, and defines the reader of that copy: LDPC_DIAG_READERS in ldpc_hip_kernels.hip,
 * LDPC_DIAG_UNIT_READER in a specialised-kernel unit.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#if defined(LDPC_HIP_DIAG) || defined(LDPC_HIP_DIAG_PHASE) || defined(LDPC_HIP_DIAG_TBJ) || defined(LDPC_HIP_DIAG_DM)
/* s_memtime stamps of block 0 after every step barrier */
static __device__ uint64_t g_diag[4096];
/* last iteration: per step and wave, (start, end of row work) or phases; or a workgroup's eight stamps */
static __device__ uint64_t g_diag2[64 * 16 * 8];
#define LDPC_DIAG_READERS                                                                                              \
  extern "C" int ldpc_hip_diag_read(uint64_t* out, uint32_t n)                                                        \
  {                                                                                                                    \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), n * sizeof(uint64_t)) == hipSuccess ? 0 : -2;                \
  }                                                                                                                    \
  extern "C" int ldpc_hip_diag2_read(uint64_t* out, uint32_t n)                                                       \
  {                                                                                                                    \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag2), n * sizeof(uint64_t)) == hipSuccess ? 0 : -2;               \
  }
#else
#define LDPC_DIAG_READERS
#endif

/* Each specialised-kernel unit's g_diag2 (the stamps of its kernels) is read by ldpc_hip_diag2_read_<unit>
 * (tools/diag_timeline.py). */
#if defined(LDPC_HIP_DIAG)
#define LDPC_DIAG_UNIT_READER_(u)                                                                                      \
  extern "C" int ldpc_hip_diag2_read_##u(uint64_t* out, uint32_t n)                                                  \
  {                                                                                                                    \
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag2), n * sizeof(uint64_t)) == hipSuccess ? 0 : -2;               \
  }
#define LDPC_DIAG_UNIT_READER(u) LDPC_DIAG_UNIT_READER_(u)
#else
#define LDPC_DIAG_UNIT_READER(u)
#endif

#ifdef LDPC_HIP_DIAG /* specialised kernel: per (step, wave) phase stamps of block 0, overwritten every iteration */
#define SPEC_STAMP(S, k)                                                                                               \
  do {                                                                                                                 \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) {                                                                  \
      g_diag2[((S) * 16 + (threadIdx.x >> 6)) * 8 + (k)] = __builtin_amdgcn_s_memtime();                               \
    }                                                                                                                  \
  } while (0)
#else
#define SPEC_STAMP(S, k) ((void)0)
#endif
#if defined(LDPC_HIP_DIAG) && defined(LDPC_HIP_DIAG_FULL) /* phase stamps inside a step: perturb the schedule */
#define SPEC_STAMP_FULL(S, k) SPEC_STAMP(S, k)
#else
#define SPEC_STAMP_FULL(S, k) ((void)0)
#endif
#ifdef LDPC_HIP_DIAG_PHASE /* s_memtime at phase boundaries of the row update, into the caller's ph[] */
#define PHASE(i) (ph[(i)] = __builtin_amdgcn_s_memtime())
#else
#define PHASE(i) ((void)0)
#endif

/* decode_cb's stamps (its tid and crc_tables): slot k of the workgroup's eight; CB_STAMP_ENTRY is slot 6, the body's
 * entry before a fused dematcher. With LDPC_HIP_DIAG_CB_DM slots 1-3 hold the fused dematcher's stamps instead. */
#ifdef LDPC_HIP_DIAG_CB_DM
#define LDPC_DIAG_CB_DM_ON 1
#else
#define LDPC_DIAG_CB_DM_ON 0
#endif
#ifdef LDPC_HIP_DIAG_CB
#define CB_STAMP_AT(k)                                                                                                 \
  reinterpret_cast<uint64_t*>(const_cast<uint32_t*>(crc_tables) + DIAG_CB_OFFSET)[blockIdx.x * 8 + (k)] =            \
      __builtin_amdgcn_s_memrealtime()
#define CB_STAMP_ENTRY()                                                                                               \
  if (threadIdx.x == 0 && blockIdx.x < 1024) {                                                                         \
    CB_STAMP_AT(6);                                                                                                    \
  }
#define CB_STAMP(k)                                                                                                    \
  if (tid == 0 && blockIdx.x < 1024 && !(LDPC_DIAG_CB_DM_ON && (k) >= 1 && (k) <= 3)) {                              \
    CB_STAMP_AT(k);                                                                                                    \
  }
#else
#define CB_STAMP_ENTRY()
#define CB_STAMP(k)
#endif

/* dematch_body's stamps (its tab, which sits at DTAB_OFFSET of the context's table buffer) */
#if defined(LDPC_HIP_DIAG_CB_DM) /* the decoder's per-workgroup slots 1-3 */
#define DM_STAMP(k)                                                                                                    \
  if (threadIdx.x == 0 && blockIdx.x < 1024) {                                                                         \
    reinterpret_cast<uint64_t*>(const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(&tab) - DTAB_OFFSET) +       \
                                DIAG_CB_OFFSET)[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();             \
  }
#elif defined(LDPC_HIP_DIAG_DM)
#define DM_STAMP(k)                                                                                                    \
  if (threadIdx.x == 0 && blockIdx.x < 1024) {                                                                         \
    g_diag2[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                                                  \
  }
#else
#define DM_STAMP(k)
#endif

/* ldpc_tb_join_kernel's stamps (its tid) */
#ifdef LDPC_HIP_DIAG_TBJ
#define TBJ_STAMP(k)                                                                                                   \
  if (tid == 0 && blockIdx.x < 64) {                                                                                   \
    g_diag2[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                                                  \
  }
#else
#define TBJ_STAMP(k)
#endif
