/*
 * The modulation mapper's code object (downlink; nothing of the decoder or the uplink family is compiled here):
 * ldpc_modulate_kernel, the stand-alone mapper with the PDSCH scrambler in front, and ldpc_rate_match_modulate_kernel,
 * the rate matcher's bit selection followed by scrambler and mapper with no packed-bit round trip; their host launchers
 * (ldpc_hip_launch.h).
 *
 * modulation_mapper_lut_impl.cpp: symbol i takes bits b0 .. b(Qm-1) = input bits Qm i .. Qm i + Qm - 1 (MSB first),
 * s_k = 1 - 2 b_k, Re from the even-index bits and Im from the odd ones in the nested form of TS 38.211 5.1:
 *   QPSK (s0, s1); 16-QAM (s0 (2 - s2), s1 (2 - s3)); 64-QAM (s0 (4 - s2 (2 - s4)), ...);
 *   256-QAM (s0 (8 - s2 (4 - s4 (2 - s6))), ...); BPSK (s0, s0); pi/2-BPSK (s0, s0) at even symbols of the span and
 *   (-s0, s0) at odd ones.
 * ci8 output is these odd integers (the caller applies get_modulation_scaling); cf32 output is float(level) * scaling,
 * one float32 multiply per component (mod_scaling_bits, ldpc_hip_device.h).
 * The pdsch_modulator_impl.cpp:108-132 scrambling is apply_xor(bit_buffer) of the TS 38.211 5.2.1 sequence
 * (ldpc_prs_device.h) on the bits before they are mapped.
 *
 * A thread owns one chunk of its segment: 32 bits (96 for 64-QAM), which is a whole number of sequence words and of
 * symbols (32 / Qm, 16 for 64-QAM), held MSB first in one (three) registers. A full chunk whose segment starts on a
 * 16-byte boundary of the symbol buffer leaves in 16-byte stores (8 ci8 or 2 cf32 symbols each; the four ci8 symbols of
 * a 256-QAM chunk in one 8-byte store); other segments and the last, partial chunk in element stores. No LDS.
 */
#include "ldpc_block_item.h"
#include "ldpc_hip_launch.h"
#include "ldpc_prs_device.h"

namespace ldpc_hip {
namespace {

constexpr int mod_qm(int mod) { return mod <= 1 ? 1 : mod; }
constexpr int mod_chunk_words(int mod) { return static_cast<int>(mod_chunk_bits(mod_qm(mod)) / 32U); }
constexpr int mod_chunk_syms(int mod) { return static_cast<int>(mod_chunk_bits(mod_qm(mod))) / mod_qm(mod); }

/* One axis of a 2^(2 N)-QAM symbol from the bits of v at top, top - 2, ..: s_j = 1 - 2 bit(top - 2 j),
 * s_0 (2^(N-1) - s_1 (2^(N-2) - .. s_(N-1))). */
template <int N>
__device__ __forceinline__ int mod_axis(uint32_t v, int top)
{
  int t = 1 - 2 * static_cast<int>((v >> (top - 2 * (N - 1))) & 1U);
#pragma unroll
  for (int j = N - 2; j >= 0; --j) {
    t = (1 << (N - 1 - j)) - t;
    t = ((v >> (top - 2 * j)) & 1U) != 0U ? -t : t;
  }
  return t;
}

/* the integer levels of the symbol whose Qm bits are v (b0 the most significant); odd: an odd symbol of a pi/2-BPSK span */
template <int MOD>
__device__ __forceinline__ void mod_levels(uint32_t v, bool odd, int& re, int& im)
{
  if constexpr (MOD <= 1) {
    const int s = 1 - 2 * static_cast<int>(v & 1U);
    re          = (MOD == 0 && odd) ? -s : s;
    im          = s;
  } else {
    re = mod_axis<MOD / 2>(v, MOD - 1);
    im = mod_axis<MOD / 2>(v, MOD - 2);
  }
}

/* the Qm bits of symbol k of a chunk held MSB first in W (bit 31 of W[0] is the chunk's first bit) */
template <int MOD>
__device__ __forceinline__ uint32_t mod_symbol_bits(const uint32_t (&W)[mod_chunk_words(MOD)], int k)
{
  constexpr int QM = mod_qm(MOD);
  if constexpr (QM == 6) {
    const int      p  = 6 * k, w = p >> 5;
    const uint64_t hi = W[w], lo = W[w < 2 ? w + 1 : 2];
    return static_cast<uint32_t>(((hi << 32) | lo) >> (58 - (p & 31))) & 63U;
  } else {
    return (W[0] >> (32 - QM * (k + 1))) & ((1U << QM) - 1U);
  }
}

/* Maps the chunk W (already scrambled) to its first ns symbols, symbol s0 .. of the segment whose first symbol is at
 * seg_out; vec: seg_out is 16-byte aligned (segment-uniform). s0 is a multiple of the chunk's symbol count (even). */
template <int MOD, bool CI8>
__device__ __forceinline__ void mod_chunk(const uint32_t (&W)[mod_chunk_words(MOD)], uint32_t s0, uint32_t ns,
                                          uint8_t* __restrict__ seg_out, bool vec)
{
#pragma clang fp contract(off)
  constexpr int NSC = mod_chunk_syms(MOD);
  static_assert(NSC % 4 == 0, "a chunk is whole 8-byte groups of ci8 symbols and 16-byte pairs of cf32 symbols");
  const bool full = vec && ns == static_cast<uint32_t>(NSC);
  if constexpr (CI8) {
    int8_t* o = reinterpret_cast<int8_t*>(seg_out) + 2ULL * s0;
    if (full) {
      uint32_t pk[NSC / 2]; /* two symbols per word: re, im, re, im from the low byte */
#pragma unroll
      for (int k = 0; k < NSC; k += 2) {
        int r0, i0, r1, i1;
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k), false, r0, i0);
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k + 1), true, r1, i1);
        pk[k / 2] = (static_cast<uint32_t>(r0) & 0xffU) | (static_cast<uint32_t>(i0) & 0xffU) << 8 |
                    (static_cast<uint32_t>(r1) & 0xffU) << 16 | (static_cast<uint32_t>(i1) & 0xffU) << 24;
      }
      if constexpr (NSC == 4) {
        *reinterpret_cast<uint2*>(o) = make_uint2(pk[0], pk[1]);
      } else {
#pragma unroll
        for (int g = 0; g < NSC / 8; ++g) {
          reinterpret_cast<uint4*>(o)[g] = make_uint4(pk[4 * g], pk[4 * g + 1], pk[4 * g + 2], pk[4 * g + 3]);
        }
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NSC; ++k) {
      if (static_cast<uint32_t>(k) < ns) {
        int re, im;
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k), (k & 1) != 0, re, im);
        o[2 * k]     = static_cast<int8_t>(re);
        o[2 * k + 1] = static_cast<int8_t>(im);
      }
    }
  } else {
    const float sc = __uint_as_float(mod_scaling_bits(MOD));
    float*      o  = reinterpret_cast<float*>(seg_out) + 2ULL * s0;
    if (full) {
#pragma unroll
      for (int k = 0; k < NSC; k += 2) {
        int r0, i0, r1, i1;
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k), false, r0, i0);
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k + 1), true, r1, i1);
        reinterpret_cast<float4*>(o)[k / 2] = make_float4(static_cast<float>(r0) * sc, static_cast<float>(i0) * sc,
                                                          static_cast<float>(r1) * sc, static_cast<float>(i1) * sc);
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NSC; ++k) {
      if (static_cast<uint32_t>(k) < ns) {
        int re, im;
        mod_levels<MOD>(mod_symbol_bits<MOD>(W, k), (k & 1) != 0, re, im);
        o[2 * k]     = static_cast<float>(re) * sc;
        o[2 * k + 1] = static_cast<float>(im) * sc;
      }
    }
  }
}

/* the chunk's sequence words XORed in: sequence bit i of a word meets the word's bit 31 - i (MSB first) */
template <int NW>
__device__ __forceinline__ void mod_scramble(uint32_t (&W)[NW], uint32_t x1, uint32_t x2, uint32_t chunk)
{
  prs_jump_words(x1, x2, chunk * NW);
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    W[j] ^= __builtin_bitreverse32(prs_next_word(x1, x2));
  }
}

/* stand-alone: the chunk's bytes from the packed input, never past the segment's last byte */
template <int MOD, bool CI8>
__device__ __forceinline__ void mod_segment(const mod_seg& sg, uint32_t chunk, const uint8_t* __restrict__ bits_base,
                                            uint8_t* __restrict__ seg_out, bool vec)
{
  constexpr int      NW  = mod_chunk_words(MOD);
  constexpr uint32_t NSC = mod_chunk_syms(MOD);
  const uint32_t     s0  = chunk * NSC;
  if (s0 >= sg.nof_symbols) {
    return;
  }
  const uint32_t ns     = min(NSC, sg.nof_symbols - s0);
  const uint64_t nbytes = (static_cast<uint64_t>(sg.nof_symbols) * mod_qm(MOD) + 7U) / 8U;
  const uint8_t* in     = bits_base + sg.bit_offset;
  const bool     al     = (reinterpret_cast<uintptr_t>(in) & 3U) == 0; /* segment-uniform */
  uint32_t       W[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const uint64_t b = (static_cast<uint64_t>(chunk) * NW + j) * 4U;
    if (al && b + 4U <= nbytes) {
      W[j] = __builtin_bswap32(*reinterpret_cast<const uint32_t*>(in + b));
    } else {
      uint32_t w = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        if (b + k < nbytes) {
          w |= static_cast<uint32_t>(in[b + k]) << (24U - 8U * k);
        }
      }
      W[j] = w;
    }
  }
  if (sg.x1 != 0U) {
    mod_scramble<NW>(W, sg.x1, sg.x2, chunk);
  }
  mod_chunk<MOD, CI8>(W, s0, ns, seg_out, vec);
}

/* fused: the chunk's bits selected from the codeword as ldpc_rate_match_kernel selects them (ldpc_rate_matcher_impl.cpp
 * :36-160): symbol jj's bit i is selected bit i EQ + jj, so for each i the chunk's symbols read consecutive ranks of
 * the filler-free circular sequence: one division per (chunk, i), then a step with wrap-around per symbol. */
template <int MOD, bool CI8>
__device__ __forceinline__ void mod_rate_match(const rm_mod_cb& c, uint32_t chunk, const uint8_t* __restrict__ cw_base,
                                               uint8_t* __restrict__ seg_out, bool vec)
{
  constexpr int      NW  = mod_chunk_words(MOD);
  constexpr uint32_t NSC = mod_chunk_syms(MOD);
  constexpr uint32_t QM  = mod_qm(MOD);
  const ratematch_cb& d  = c.rm;
  const uint32_t      EQ = d.rm_length / QM;
  const uint32_t      s0 = chunk * NSC;
  if (s0 >= EQ) {
    return;
  }
  const uint32_t ns = min(NSC, EQ - s0);
  const uint8_t* cw = cw_base + d.cw_offset;
  const uint32_t fl = min(d.fill_lo, d.Ncb), fh = min(d.fill_hi, d.Ncb);
  const uint32_t L  = d.Ncb - (fh - fl); /* selectable bits in the circular buffer */
  uint32_t       k0 = d.k0;
  if (k0 >= fl && k0 < fh) {
    k0 = fh; /* select_bits: skip a filler start */
  }
  k0                = (k0 >= d.Ncb) ? 0 : k0;
  const uint32_t r0 = (k0 < fl) ? k0 : k0 - (fh - fl); /* rank of the first selected bit */
  uint32_t       W[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    W[j] = 0;
  }
#pragma unroll
  for (uint32_t i = 0; i < QM; ++i) {
    uint32_t r = (r0 + i * EQ + s0) % L; /* the host admits E < 2^31 */
#pragma unroll
    for (uint32_t k = 0; k < NSC; ++k) {
      if (k < ns) {
        const uint32_t p   = (r < fl) ? r : r + (fh - fl);
        const uint32_t bit = (cw[p >> 3] >> (7U - (p & 7U))) & 1U;
        const uint32_t q   = k * QM + i; /* the bit's place in the chunk */
        W[q >> 5] |= bit << (31U - (q & 31U));
        r = (r + 1U == L) ? 0U : r + 1U;
      }
    }
  }
  if (c.mod.x1 != 0U) {
    mod_scramble<NW>(W, c.mod.x1, c.mod.x2, chunk);
  }
  mod_chunk<MOD, CI8>(W, s0, ns, seg_out, vec);
}

} // namespace

template <bool CI8>
__global__ void __launch_bounds__(MOD_BLOCK)
    ldpc_modulate_kernel(const mod_seg* __restrict__ segs, uint32_t nseg, const uint8_t* __restrict__ bits_base,
                         uint8_t* __restrict__ sym_base)
{
  const mod_seg  sg    = segs[block_item(segs, nseg)];
  const uint32_t chunk = (blockIdx.x - sg.block0) * MOD_BLOCK + threadIdx.x;
  uint8_t*       out   = sym_base + sg.sym_offset * (CI8 ? 2U : 8U);
  const bool     vec   = (reinterpret_cast<uintptr_t>(out) & 15U) == 0;
  switch (sg.modulation) { /* block-uniform */
    case 0: mod_segment<0, CI8>(sg, chunk, bits_base, out, vec); break;
    case 1: mod_segment<1, CI8>(sg, chunk, bits_base, out, vec); break;
    case 2: mod_segment<2, CI8>(sg, chunk, bits_base, out, vec); break;
    case 4: mod_segment<4, CI8>(sg, chunk, bits_base, out, vec); break;
    case 6: mod_segment<6, CI8>(sg, chunk, bits_base, out, vec); break;
    default: mod_segment<8, CI8>(sg, chunk, bits_base, out, vec); break;
  }
}

template <bool CI8>
__global__ void __launch_bounds__(MOD_BLOCK)
    ldpc_rate_match_modulate_kernel(const rm_mod_cb* __restrict__ cbs, uint32_t ncb,
                                    const uint8_t* __restrict__ cw_base, uint8_t* __restrict__ sym_base)
{
  const rm_mod_cb c     = cbs[block_item(cbs, ncb, [](const rm_mod_cb& s) { return s.mod.block0; })];
  const uint32_t  chunk = (blockIdx.x - c.mod.block0) * MOD_BLOCK + threadIdx.x;
  uint8_t*        out   = sym_base + c.mod.sym_offset * (CI8 ? 2U : 8U);
  const bool      vec   = (reinterpret_cast<uintptr_t>(out) & 15U) == 0;
  switch (c.mod.modulation) { /* block-uniform; pi/2-BPSK is refused on the host */
    case 1: mod_rate_match<1, CI8>(c, chunk, cw_base, out, vec); break;
    case 2: mod_rate_match<2, CI8>(c, chunk, cw_base, out, vec); break;
    case 4: mod_rate_match<4, CI8>(c, chunk, cw_base, out, vec); break;
    case 6: mod_rate_match<6, CI8>(c, chunk, cw_base, out, vec); break;
    default: mod_rate_match<8, CI8>(c, chunk, cw_base, out, vec); break;
  }
}

hipError_t launch_modulate(const mod_seg* d_segs, uint32_t nseg, uint32_t nblocks, bool ci8, const uint8_t* d_bits,
                           void* d_sym, hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  uint8_t* out = static_cast<uint8_t*>(d_sym);
  if (ci8) {
    hipLaunchKernelGGL(ldpc_modulate_kernel<true>, dim3(nblocks), dim3(MOD_BLOCK), 0, stream, d_segs, nseg, d_bits, out);
  } else {
    hipLaunchKernelGGL(ldpc_modulate_kernel<false>, dim3(nblocks), dim3(MOD_BLOCK), 0, stream, d_segs, nseg, d_bits,
                       out);
  }
  return hipGetLastError();
}

hipError_t launch_rate_match_modulate(const rm_mod_cb* d_cbs, uint32_t ncb, uint32_t nblocks, bool ci8,
                                      const uint8_t* d_cws, void* d_sym, hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  uint8_t* out = static_cast<uint8_t*>(d_sym);
  if (ci8) {
    hipLaunchKernelGGL(ldpc_rate_match_modulate_kernel<true>, dim3(nblocks), dim3(MOD_BLOCK), 0, stream, d_cbs, ncb,
                       d_cws, out);
  } else {
    hipLaunchKernelGGL(ldpc_rate_match_modulate_kernel<false>, dim3(nblocks), dim3(MOD_BLOCK), 0, stream, d_cbs, ncb,
                       d_cws, out);
  }
  return hipGetLastError();
}

} // namespace ldpc_hip
