/*
 * The uplink kernel family around the decoder and its host launchers (ldpc_hip_launch.h): rate dematching (and its
 * work-queue kernel), the transport-block join, soft demodulation, and descrambling / the packed-bit scrambler.
 * Needs the utility, work-queue and dematch headers only, nothing of the decoder. Compiled into the decode code object
 * (included by ldpc_hip_kernels.hip, which says why).
 */
#pragma once

#include "ldpc_block_item.h"
#include "ldpc_dematch_body.h"
#include "ldpc_device_util.h"
#include "ldpc_diag.h"
#include "ldpc_dwq_loop.h"
#include "ldpc_hip_launch.h"

namespace ldpc_hip {

/* the persistent work-queue kernel (ldpc_hip_dwq.cpp) of the dematch-only items */
__global__ void __launch_bounds__(DM_THREADS) ldpc_dwq_dematch_kernel(dwq_args a)
{
  dwq_loop(a, [&](const dwq_item& it) __attribute__((always_inline)) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    dematch_body(dm_plain(it.dm), *reinterpret_cast<const demod_tables*>(it.crc_tables + DTAB_OFFSET),
                 reinterpret_cast<int8_t*>(smem), *reinterpret_cast<demod_tables*>(smem + DM_STAGE));
  });
}
const void* dwq_kernel_dematch() { return reinterpret_cast<const void*>(&ldpc_dwq_dematch_kernel); }

/* ldpc_rate_dematcher_impl::rate_dematch, one workgroup per codeblock (ldpc_dematch_body.h dematch_body). */
__global__ void __launch_bounds__(DM_THREADS) ldpc_rate_dematch_kernel(const dematch_cb* __restrict__ cbs,
                                                                       dematch_cb one, demod_tables tab)
{
  __shared__ __attribute__((aligned(16))) int8_t s_in[DM_STAGE];
  __shared__ demod_tables                        s_dtab;
  dematch_body(cbs != nullptr ? cbs[blockIdx.x] : one, tab, s_in, s_dtab); /* nullptr: one CB, descriptor by value */
}


/* ---- transport-block join: pusch_decoder_impl::join_and_notify / concatenate_codeblocks (pusch_decoder_impl.cpp:
 * 384-497), one workgroup per TB. Each thread owns a contiguous run of TB bytes: it gathers them bit-exactly from the
 * CB messages (data bits only: K*Z - CRC - filler per CB) and folds their CRC24A remainder into the TB CRC with
 * CRC(A || B) = CRC(A) x^(8|B|) + CRC(B) mod G. ---- */
namespace {

/* bit i of a packed MSB-first message, as the low bit */
__device__ __forceinline__ uint32_t msg_bit(const uint8_t* m, uint32_t i) { return (m[i >> 3] >> (7 - (i & 7))) & 1U; }

/* 8 message bits starting at bit q (q + 8 <= message length + 8; the byte after the message is never consumed) */
__device__ __forceinline__ uint32_t msg_byte_at(const uint8_t* m, uint32_t q)
{
  const uint32_t b = q >> 3, sh = q & 7U;
  if (sh == 0) {
    return m[b];
  }
  return ((static_cast<uint32_t>(m[b]) << sh) | (static_cast<uint32_t>(m[b + 1]) >> (8 - sh))) & 0xffU;
}

} // namespace

/* Multi-workgroup TB join. The TB is front-padded with zero bytes to a whole number of 4 KiB chunks (leading zeros do
 * not change a zero-initialised CRC); workgroup (TB, chunk c) gathers its 4 KiB, each thread 16 bytes, computes the
 * chunk's CRC24A remainder as XOR_t crc_t * x^(8*16*(255-t)) mod G, and stores it. The last workgroup of the TB to
 * arrive (device-scope counter) combines the chunks as XOR_c crc_c * x^(8*4096*(n-1-c)) mod G, checks the checksum
 * carried by the last CB, writes the result and resets the TB's CB flags on a TB CRC failure (:423-428). The powers
 * of x come from the host (build_crc_tables). work: per TB TBJ_WORK_WORDS words (chunk CRCs, arrival counter; the
 * counter is zero between launches). blocks[b]: workgroup b's TB descriptor, TB index and chunk (one load, no search).
 * The kernel is a chain of dependent memory round trips, so every load that does not depend on another load's value
 * is issued as early as possible: the power of x for this thread, the checksum bits, and the chunk's message bytes
 * (gathered before the CB CRC flags are known; discarded when a CB failed). */
__global__ void __launch_bounds__(TBJ_THREADS)
    ldpc_tb_join_kernel(const tbj_block* __restrict__ blocks, const uint8_t* __restrict__ msgs,
                        ldpc_hip_cb_result* __restrict__ cb_res,
                        uint8_t* __restrict__ tb_base, ldpc_hip_tb_result* __restrict__ tb_res,
                        const uint32_t* __restrict__ crc_tables, uint32_t* __restrict__ work)
{
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_acc[4];
  __shared__ uint32_t s_wok[TBJ_THREADS / 64];
  const int              tid   = threadIdx.x;
  TBJ_STAMP(0);
  const uint32_t*        pw    = crc_tables + TBJ_POW_OFFSET;
  const uint32_t         pw_t  = pw[TBJ_THREADS - 1 - tid]; /* x^(8*16*(255-tid)) mod G */
  const tbj_block&       blk   = blocks[blockIdx.x];
  const uint32_t         t     = blk.tb;
  const uint32_t         chunk = blk.chunk;
  const ldpc_hip_tb_desc d     = blk.d;
  const uint32_t         C     = d.nof_cbs;
  const uint8_t*         m0    = msgs + d.msg_offset;
  uint8_t*               tb    = tb_base + d.tb_offset;
  const uint32_t         nb    = d.tbs / 8U;
  const uint32_t         nch   = (nb + TBJ_CHUNK - 1) / TBJ_CHUNK;
  const uint32_t         pad   = nch * TBJ_CHUNK - nb; /* leading zero bytes */
  constexpr uint32_t     G     = 0x1864cfbU;
  const uint32_t         kd    = d.cb_msg_bits - d.cb_crc_bits - d.nof_filler_bits; /* data bits per CB (:62-64) */
  /* the checksum: the 24 bits after the last CB's share of the TB (:486-490), loaded now, used by the last workgroup */
  uint32_t chksum = 0;
  if (tid == 0 && C > 1) {
    const uint32_t last = d.tbs - (C - 1U) * kd;
    const uint8_t* ml   = m0 + static_cast<size_t>(C - 1U) * d.msg_stride;
    for (uint32_t i = 0; i < 24U; ++i) {
      chksum = (chksum << 1) | msg_bit(ml, last + i);
    }
  }

  if (tid == 0) {
    s_acc[1] = 0;
  }
  const uint32_t* tab = crc_tables + LDPC_HIP_CRC24A * CRC_TABLE_SIZE;
  s_tab[tid]          = tab[tid];
  /* this thread's TB bytes: virtual positions v0 .. v0 + 15 of the padded TB, real byte = v - pad */
  const uint32_t v0 = chunk * TBJ_CHUNK + static_cast<uint32_t>(tid) * TBJ_BYTES;
  /* gather (C > 1): all loads first, then the CRC chain over registers; issued before the CB flags are known */
  uint32_t val[TBJ_BYTES] = {};
  if (C > 1 && (kd & 7U) == 0) {
    /* whole data bytes per CB (every TB the segmenter makes: TBS, CRC and filler bits are multiples of 8): byte
     * loads, the CB index and offset stepped without divisions, no branches around the loads */
    const uint32_t kdb   = kd >> 3;
    const uint32_t first = (v0 >= pad) ? v0 - pad : 0;
    uint32_t       r     = first / kdb;
    uint32_t       o     = first - r * kdb;
#pragma unroll
    for (int k = 0; k < TBJ_BYTES; ++k) {
      const bool real = v0 + k >= pad;
      const uint8_t x = m0[static_cast<size_t>(r) * d.msg_stride + o];
      val[k]          = real ? x : 0U;
      const bool step = real && o + 1U == kdb;
      o               = step ? 0U : o + (real ? 1U : 0U);
      r += step ? 1U : 0U;
    }
  } else if (C > 1) {
    const uint32_t first = (v0 >= pad) ? v0 - pad : 0;
    uint32_t       p     = 8U * first;
    uint32_t       r     = p / kd;
    uint32_t       q     = p - r * kd;
#pragma unroll
    for (int k = 0; k < TBJ_BYTES; ++k) {
      const uint32_t v = v0 + k;
      uint32_t       x = 0;
      if (v >= pad) {
        if (q + 8U <= kd) {
          x = msg_byte_at(m0 + static_cast<size_t>(r) * d.msg_stride, q);
        } else { /* straddles into the next CB */
          for (uint32_t i = 0; i < 8U; ++i) {
            const uint32_t qi = q + i;
            x = (x << 1) | ((qi < kd) ? msg_bit(m0 + static_cast<size_t>(r) * d.msg_stride, qi)
                                      : msg_bit(m0 + static_cast<size_t>(r + 1) * d.msg_stride, qi - kd));
          }
        }
        q += 8U;
        if (q >= kd) {
          q -= kd;
          ++r;
        }
      }
      val[k] = x;
    }
  }
  /* CBs whose CRC passed: per-thread count, wave sum by shuffles, one LDS word per wave (no zeroing barrier) */
  uint32_t myok = 0;
  for (uint32_t r = tid; r < C; r += TBJ_THREADS) {
    myok += (cb_res[d.result_index + r].crc_pass != 0) ? 1U : 0U;
  }
  for (int o = 32; o > 0; o >>= 1) {
    myok += __shfl_xor(myok, o);
  }
  if ((tid & 63) == 0) {
    s_wok[tid >> 6] = myok;
  }
  __syncthreads();
  TBJ_STAMP(1);
  uint32_t nok = 0;
  for (int w = 0; w < TBJ_THREADS / 64; ++w) {
    nok += s_wok[w];
  }

  if (C == 1) {
    /* the CB CRC is the TB CRC; copy the TB bytes only when it passed (:409-417) */
    if (nok == 1) {
      for (uint32_t k = 0; k < TBJ_BYTES; ++k) {
        const uint32_t v = v0 + k;
        if (v >= pad) {
          tb[v - pad] = m0[v - pad];
        }
      }
    }
    if (chunk == 0 && tid == 0) {
      tb_res[t] = ldpc_hip_tb_result{static_cast<uint8_t>(nok), static_cast<uint8_t>(nok), static_cast<uint16_t>(nok)};
    }
    return;
  }
  if (nok != C) { /* :418-420, nothing written */
    if (chunk == 0 && tid == 0) {
      tb_res[t] = ldpc_hip_tb_result{0, 0, static_cast<uint16_t>(nok)};
    }
    return;
  }
  uint32_t crc = 0;
#pragma unroll
  for (int k = 0; k < TBJ_BYTES; ++k) {
    crc = ((crc << 8) ^ s_tab[((crc >> 16) ^ val[k]) & 0xffU]) & 0xffffffU; /* crc_calculator_generic_impl.cpp */
  }
  crc = gf2_mulmod(crc, pw_t, 24, G);
  for (int o = 32; o > 0; o >>= 1) { /* wave XOR, then one LDS atomic per wave (same-address atomics serialise) */
    crc ^= __shfl_xor(crc, o);
  }
  if ((tid & 63) == 0) {
    atomicXor(&s_acc[1], crc);
  }
  __syncthreads();
  TBJ_STAMP(2);
  /* Hand-off to the TB's last workgroup without cache-wide fences (cdna_hip_programming.md Guideline 16, R1): the chunk
   * CRC is stored write-through (agent-scope atomic store), drained, then the arrival counter is bumped; the last
   * arriver reads the chunk CRCs with agent-scope (sc1) loads, which bypass the stale caches. */
  typedef __attribute__((address_space(1))) uint32_t gu32;
  gu32* wk = (gu32*)(uintptr_t)(work + static_cast<size_t>(t) * TBJ_WORK_WORDS); /* global, not flat */
  if (tid == 0) {
    __hip_atomic_store(&wk[chunk], s_acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_acc[2] = __hip_atomic_fetch_add(&wk[TBJ_MAX_CHUNKS], 1U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  TBJ_STAMP(3);
  /* the TB bytes, stored after the hand-off: no barrier or counter waits for their completion (vmcnt counts stores
   * too); the kernel's end makes them visible */
#pragma unroll
  for (int k = 0; k < TBJ_BYTES; ++k) {
    const uint32_t v = v0 + k;
    if (v >= pad) {
      tb[v - pad] = static_cast<uint8_t>(val[k]);
    }
  }
  if (s_acc[2] != nch - 1) {
    return; /* not the last workgroup of this TB */
  }
  if (tid == 0) {
    s_acc[3] = 0;
  }
  __syncthreads();
  if (static_cast<uint32_t>(tid) < ((nch + 63U) & ~63U)) { /* the waves holding chunks, whole */
    uint32_t x = 0;
    if (static_cast<uint32_t>(tid) < nch) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); /* keeps the sc1 loads below the counter read */
      const uint32_t c = __hip_atomic_load(&wk[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      x                = gf2_mulmod(c, pw[TBJ_THREADS + nch - 1 - tid], 24, G);
    }
    for (int o = 32; o > 0; o >>= 1) {
      x ^= __shfl_xor(x, o);
    }
    if ((tid & 63) == 0) {
      atomicXor(&s_acc[3], x);
    }
  }
  __syncthreads();
  if (tid == 0) {
    wk[TBJ_MAX_CHUNKS] = 0; /* counter back to zero for the next launch */
    s_acc[0]           = (s_acc[3] == chksum) ? 1U : 0U;
    tb_res[t] = ldpc_hip_tb_result{static_cast<uint8_t>(s_acc[0]), 1, static_cast<uint16_t>(nok)};
  }
  __syncthreads();
  TBJ_STAMP(4);
  if (s_acc[0] == 0) { /* reset_codeblocks_crc (:423-428): a false-positive CB is somewhere; decode all again */
    for (uint32_t r = tid; r < C; r += TBJ_THREADS) {
      cb_res[d.result_index + r].crc_pass = 0;
    }
  }
}

hipError_t launch_tb_join(const tbj_block* d_blocks, uint32_t nblocks, const uint8_t* msgs, ldpc_hip_cb_result* cb,
                          uint8_t* tb, ldpc_hip_tb_result* res, const uint32_t* d_crc, uint32_t* d_work,
                          hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_tb_join_kernel, dim3(nblocks), dim3(TBJ_THREADS), 0, stream, d_blocks, msgs, cb, tb, res,
                     d_crc, d_work);
  return hipGetLastError();
}

hipError_t launch_dematch(const dematch_cb* d_cbs, uint32_t n, const demod_tables& tab, hipStream_t stream,
                          const dematch_cb* host_one)
{
  if (n == 0) {
    return hipSuccess;
  }
  const bool       inl = host_one != nullptr && n == 1; /* one CB: descriptor by value */
  const dematch_cb one = inl ? *host_one : dematch_cb{};
  hipLaunchKernelGGL(ldpc_rate_dematch_kernel, dim3(n), dim3(DM_THREADS), 0, stream, inl ? nullptr : d_cbs, one, tab);
  return hipGetLastError();
}

/* ---- soft demodulation mapper -------------------------------------------------------------
 * demodulation_mapper::demodulate_soft (demodulation_mapper_impl.cpp:78-106) with the reference's portable scalar
 * per-symbol functions: BPSK / pi/2-BPSK (demodulation_mapper_impl.cpp:33-76), QPSK (demodulation_mapper_qpsk.cpp:
 * 133-169), 16-QAM (demodulation_mapper_qam16.cpp:201-273), 64-QAM and 256-QAM by interval functions
 * (demodulation_mapper_intervals.h:33-63, demodulation_mapper_qam64.cpp:382-463, demodulation_mapper_qam256.cpp:
 * 346-427), then log_likelihood_ratio::quantize (log_likelihood_ratio.cpp:88-97). Float arithmetic in the
 * reference's order without contraction, divisions correctly rounded (HIP's default), so the LLRs equal the CPU
 * restatement's bit for bit. One thread per symbol, Qm LLR bytes per thread: HBM-bound (8 + 4 B in, Qm B out). */
template <int MOD>
__device__ __forceinline__ void dm_segment(const demod_seg& sg, uint32_t i, const demod_tables& tab,
                                           const float2* __restrict__ sym_base, const float* __restrict__ nv_base,
                                           int8_t* __restrict__ llr_base)
{
  constexpr int QM = (MOD <= 1) ? 1 : MOD;
  int8_t        o[8];
  dm_symbol<MOD>(sym_base[sg.sym_offset + i], nv_base[sg.noise_offset + i], i, tab, o);
  int8_t*         out = llr_base + sg.llr_offset + static_cast<uint64_t>(i) * QM;
  const uintptr_t a   = reinterpret_cast<uintptr_t>(llr_base + sg.llr_offset); /* segment-uniform alignment */
  auto            b   = [&](int k) { return static_cast<uint32_t>(static_cast<uint8_t>(o[k])); };
  if constexpr (QM == 8) {
    if ((a & 7U) == 0) {
      *reinterpret_cast<uint2*>(out) = make_uint2(b(0) | b(1) << 8 | b(2) << 16 | b(3) << 24,
                                                  b(4) | b(5) << 8 | b(6) << 16 | b(7) << 24);
      return;
    }
  } else if constexpr (QM == 4) {
    if ((a & 3U) == 0) {
      *reinterpret_cast<uint32_t*>(out) = b(0) | b(1) << 8 | b(2) << 16 | b(3) << 24;
      return;
    }
  } else if constexpr (QM == 2 || QM == 6) {
    if ((a & 1U) == 0) {
#pragma unroll
      for (int k = 0; k < QM; k += 2) {
        reinterpret_cast<uint16_t*>(out)[k / 2] = static_cast<uint16_t>(b(k) | b(k + 1) << 8);
      }
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < QM; ++k) {
    out[k] = o[k];
  }
}

__global__ void __launch_bounds__(DEMOD_BLOCK)
    ldpc_demodulate_kernel(const demod_seg* __restrict__ segs, uint32_t nseg, demod_tables tab,
                           const float2* __restrict__ sym_base, const float* __restrict__ nv_base,
                           int8_t* __restrict__ llr_base)
{
  __shared__ demod_tables s_tab;
  constexpr int           NW = static_cast<int>(sizeof(demod_tables) / 4);
  static_assert(NW <= DEMOD_BLOCK, "tables copied one word per thread");
  if (threadIdx.x < NW) {
    reinterpret_cast<uint32_t*>(&s_tab)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&tab)[threadIdx.x];
  }
  const demod_seg sg = segs[block_item(segs, nseg)];
  __syncthreads();
  const uint32_t i = (blockIdx.x - sg.block0) * DEMOD_BLOCK + threadIdx.x;
  if (i >= sg.nof_symbols) {
    return;
  }
  switch (sg.modulation) { /* block-uniform */
    case 0: dm_segment<0>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
    case 1: dm_segment<1>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
    case 2: dm_segment<2>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
    case 4: dm_segment<4>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
    case 6: dm_segment<6>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
    default: dm_segment<8>(sg, i, s_tab, sym_base, nv_base, llr_base); break;
  }
}

hipError_t launch_demodulate(const demod_seg* d_segs, uint32_t nseg, uint32_t nblocks, const demod_tables& tab,
                             const float* d_sym, const float* d_nv, int8_t* d_llr, hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_demodulate_kernel, dim3(nblocks), dim3(DEMOD_BLOCK), 0, stream, d_segs, nseg, tab,
                     reinterpret_cast<const float2*>(d_sym), d_nv, d_llr);
  return hipGetLastError();
}

/* ---- PUSCH descrambling and the packed-bit scrambler (pseudo_random_generator_impl.cpp apply_xor / generate) --------
 * One thread per PRS_WORDS consecutive 32-bit sequence words of a segment (ldpc_dematch_body.h prs_jump_words, then
 * prs_next_word per word). BITS = false: a word covers 32 int8 LLRs, out = c ? -in : in (-128 stays -128); two 16-byte
 * loads and stores per whole word when the segment's input and output addresses are 16-byte aligned, byte accesses
 * for other segments and for the last, partial word. BITS = true: a word covers 4 bytes of bits packed MSB first,
 * out = in ^ c, the input read as zero for a generating segment; the bits of the last byte beyond the segment's length
 * keep their input value. A thread reads its bytes before it writes them, so a segment may run in place. */
template <bool BITS>
__global__ void __launch_bounds__(PRS_BLOCK)
    ldpc_prs_kernel(const prs_seg* __restrict__ segs, uint32_t nseg, const uint8_t* in_base, uint8_t* out_base)
{
  const prs_seg  sg = segs[block_item(segs, nseg)];
  const uint32_t nw = sg.length / 32U + (sg.length % 32U != 0U ? 1U : 0U);
  const uint32_t w0 = ((blockIdx.x - sg.block0) * PRS_BLOCK + threadIdx.x) * PRS_WORDS;
  if (w0 >= nw) {
    return;
  }
  uint32_t x1 = sg.x1, x2 = sg.x2;
  prs_jump_words(x1, x2, w0);
  const bool     gen = sg.in_offset == PRS_NO_INPUT;
  const uint8_t* in  = gen ? nullptr : in_base + sg.in_offset;
  uint8_t*       out = out_base + sg.out_offset;
  const uint32_t w1  = min(w0 + PRS_WORDS, nw);
  if constexpr (!BITS) {
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15U) == 0; /* uniform */
    for (uint32_t w = w0; w < w1; ++w) {
      const uint32_t c = prs_next_word(x1, x2);
      const uint64_t b = static_cast<uint64_t>(w) * 32U;
      if (vec && b + 32U <= sg.length) {
        uint4 a0 = reinterpret_cast<const uint4*>(in + b)[0], a1 = reinterpret_cast<const uint4*>(in + b)[1];
        prs_flip32(a0, a1, c);
        reinterpret_cast<uint4*>(out + b)[0] = a0;
        reinterpret_cast<uint4*>(out + b)[1] = a1;
      } else {
        const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(32U), sg.length - b));
        for (uint32_t i = 0; i < n; ++i) {
          const int8_t v = static_cast<int8_t>(in[b + i]);
          out[b + i]     = static_cast<uint8_t>(((c >> i) & 1U) != 0U ? static_cast<int8_t>(-v) : v);
        }
      }
    }
  } else {
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3U) == 0; /* uniform */
    for (uint32_t w = w0; w < w1; ++w) {
      /* sequence bit i of the word belongs in byte i / 8 at bit 7 - i % 8 */
      const uint32_t c = __builtin_bswap32(__builtin_bitreverse32(prs_next_word(x1, x2))); /* byte k in bits 8k.. */
      const uint64_t b = static_cast<uint64_t>(w) * 4U;
      if (vec && static_cast<uint64_t>(w) * 32U + 32U <= sg.length) {
        const uint32_t v = gen ? 0U : *reinterpret_cast<const uint32_t*>(in + b);
        *reinterpret_cast<uint32_t*>(out + b) = v ^ c;
      } else {
        const uint32_t bits = static_cast<uint32_t>(min(static_cast<uint64_t>(32U), sg.length - 32U * w));
        for (uint32_t k = 0; 8U * k < bits; ++k) {
          const uint32_t nb   = min(8U, bits - 8U * k);
          const uint32_t keep = (0xff00U >> nb) & 0xffU; /* the byte's first nb bits (MSB first) */
          const uint32_t v    = gen ? 0U : in[b + k];
          out[b + k]          = static_cast<uint8_t>(v ^ ((c >> (8U * k)) & keep));
        }
      }
    }
  }
}

hipError_t launch_prs(const prs_seg* d_segs, uint32_t nseg, uint32_t nblocks, bool bits, const uint8_t* d_in,
                      uint8_t* d_out, hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  if (bits) {
    hipLaunchKernelGGL(ldpc_prs_kernel<true>, dim3(nblocks), dim3(PRS_BLOCK), 0, stream, d_segs, nseg, d_in, d_out);
  } else {
    hipLaunchKernelGGL(ldpc_prs_kernel<false>, dim3(nblocks), dim3(PRS_BLOCK), 0, stream, d_segs, nseg, d_in, d_out);
  }
  return hipGetLastError();
}

} // namespace ldpc_hip
