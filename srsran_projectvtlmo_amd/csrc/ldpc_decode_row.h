/*
 * The generic decoder's row update (row_update, row_dispatch) and the per-edge arithmetic it is made of: one lifted
 * check node of a row whose degree, columns and shifts come from tables at run time (decode_cb's generic step loop,
 * ldpc_decode_cb.h). The specialised decoders (ldpc_decode_body.h) have their own packed arithmetic.
 */
#pragma once

#include "ldpc_device_util.h"
#include "ldpc_diag.h"

namespace ldpc_hip {
namespace {

/* Check-to-variable storage. c2v is kept per edge, as the reference keeps it (ldpc_decoder_impl.h:224-226), but
 * only for the edges that exist: int8 c2v[e][t] for graph edge e and lifted check node t (edge-major, stride Z, so
 * a wave's 64 consecutive check nodes read 64 consecutive bytes). BG1 Z=384: 316 * 384 = 121,344 B. An all-zero c2v
 * is the "not yet initialised" state: soft (-) 0 = soft, the first-iteration copy of
 * update_variable_to_check_messages (impl.cpp:196-200).
 *
 * Soft bits inside the decoder hold [-120, 120] for finite LLRs and +-121 for +-infinity (the reference's +-127,
 * llr.h:238): with infinity one step above the finite range, "promotion_sum overflows to infinity" is a single
 * clamp to +-121 and x = s - clamp(s, +-120) is the infinity indicator (+-1 or 0). Only the sign and the zero test of
 * a soft bit ever leave the decoder (hard_decision), and both are unchanged by the encoding. */

/* scale_llr (ldpc_decoder_generic.cpp:70-79) for a finite magnitude m in [0, 120]: round(float(m) * sf), half away
 * from zero. v_mul_f32 is correctly rounded and llvm.round is exact, so this equals the host std::round. */
template <bool SF08>
__device__ __forceinline__ int scale_mag(int m, float sf)
{
  if (SF08) {
    /* sf = 0.8f (the PHY default, ldpc_decoder.h:50): round(0.8 m) = floor((4m + 2) / 5) = (52432 m + 26216) >> 16
     * for m in [0, 120] (checked exhaustively against the float formula) */
    return static_cast<int>((__umul24(static_cast<uint32_t>(m), 52432U) + 26216U) >> 16);
  }
  return static_cast<int>(__builtin_roundf(static_cast<float>(m) * sf));
}

/* Partner lane (lane ^ 32) value through v_permlane32_swap. */
__device__ __forceinline__ uint32_t partner32(uint32_t v, int half)
{
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return half ? r[0] : r[1];
}

/* ---- per-edge and per-row arithmetic of the row update (see row_update) ---- */

/* v2c = soft (-) c2v with the infinity push: med3(s - c, +-120) + 512 x, x = s - med3(s, +-120). */
__device__ __forceinline__ int v2c_of(int s, int c)
{
  const int x = s - med3i(s, -LLR_MAX, LLR_MAX); /* infinity indicator: +-1 or 0 */
  return (x << 9) + med3i(s - c, -LLR_MAX, LLR_MAX); /* v_lshl_add_u32 */
}

/* Two-minimum scan step: m2 = min(m2, max(m1, a)) as one v_med3_u32 (the compiler otherwise emits max + min). */
__device__ __forceinline__ void scan_edge(uint32_t& m1, uint32_t& m2, int a)
{
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m2) : "v"(m1), "v"(a), "v"(m2));
  m1 = min(m1, static_cast<uint32_t>(a));
}

/* End of pass 1: merge a split row's halves (P = 2), then the two scaled magnitudes with the parity sign folded in:
 * p1 for edges with |v2c| != min, p2 for |v2c| == min (see row_update). m1 is returned merged. */
template <int P, bool SF08>
__device__ __forceinline__ void row_scale(uint32_t& m1, uint32_t m2, uint32_t sx, int half, float sf, int& p1, int& p2)
{
  if (P == 2) {
    const uint32_t oth = partner32(m1 | (m2 << 8), half);
    const uint32_t o1 = oth & 0xffU, o2 = oth >> 8;
    m2                = min(min(m2, o2), max(m1, o1));
    m1                = min(m1, o1);
    sx ^= partner32(sx, half);
  }
  const int n1  = scale_mag<SF08>(static_cast<int>(m1), sf);
  const int n2  = scale_mag<SF08>(static_cast<int>(m2), sf);
  const int neg = static_cast<int>(sx) >> 31;
  p1            = (n1 ^ neg) - neg;
  p2            = (n2 ^ neg) - neg;
  /* opaque to the optimiser: otherwise it sinks the scaling into every edge as select + rescale */
  asm volatile("" : "+v"(p1), "+v"(p2));
}

/* Sign mask (0 / -1) and magnitude of v2c. The mask stays opaque, so the magnitude is v_xor + v_sub (not the abs
 * idiom's v_sub + v_max) and pass 2 reuses the mask instead of shifting again. */
__device__ __forceinline__ int sign_mask(int v)
{
  int sv = v >> 31;
  asm("" : "+v"(sv));
  return sv;
}

/* c2v' of an edge with v2c sign mask sv and |v2c| a. */
__device__ __forceinline__ int c2v_new(int sv, int a, uint32_t m1, int p1, int p2)
{
  const int ms = (a == static_cast<int>(m1)) ? p2 : p1;
  return (ms ^ sv) - sv;
}

/* soft' = promotion_sum(c2v', v2c). */
__device__ __forceinline__ int soft_new(int c, int v) { return med3i(c + v, -LLR_INTERNAL_INF, LLR_INTERNAL_INF); }

/* One lifted check node t of a row of degree D -- update_variable_to_check_messages,
 * update_check_to_variable_messages and update_soft_bits (ldpc_decoder_impl.cpp:176-308) restricted to Z-lane t,
 * with the generic kernels' arithmetic (ldpc_decoder_generic.cpp:30-120).
 *
 * P = 1: one lane owns the check node and scans all D edges in order.
 * P = 2: lanes l and l ^ 32 share the check node; the lower half scans edges [0, D0), the upper half [D0, D), and
 *        the partial (min1, min2, sign parity) are merged across the pair: min1 = min(A, B), min2 = min(min2_A,
 *        min2_B, max(min1_A, min1_B)) -- the two smallest of the multiset, as the sequential scan finds them.
 * Edge words (shift | col * Z << 16) come from the LDS edge table; the upper half's slot starts at edge D0.
 *
 * LLR special cases with the internal encoding above (c2v is never infinite: |c2v| <= round(120 sf) <= 120):
 *   v2c   = isinf(s) ? s : clamp(s - c2v, +-120)           (llr.cpp:56-71 operator-)
 *           computed as clamp(s - c2v, +-120) + 512 x: an infinite v2c keeps its sign and a magnitude above 512,
 *           which the two-minimum scan treats exactly like the reference's +-127 (min and min2 start at 120 and
 *           only a magnitude strictly below them is taken; |v2c| == min never holds for it);
 *   soft' = promotion_sum(c2v', v2c) = clamp(c2v' + v2c, +-121)   (llr.cpp:73-86): a finite sum saturates to
 *           infinity past +-120, and an infinite v2c (|v2c| > 512 > 121 + |c2v'|) stays infinite. */
template <int D, int P, bool SF08>
__device__ __forceinline__ void row_update(int t, int half, const uint32_t* s_slot, int8_t* s_soft,
                                           int8_t* s_c2v_row, float sf, int Z, int trash, uint64_t* ph)
{
  PHASE(0);
  constexpr int DP = (P == 1) ? D : (D + 1) / 2; /* edges scanned by this lane */
  constexpr int D0 = DP;                         /* first edge of the upper half (P = 2) */
  const int     kb = (P == 2 && half) ? D0 : 0;
  int8_t*       cq = s_c2v_row + t + kb * Z;     /* this lane's c2v of local edge kk: cq + kk * Z */

  lds_i8* sp[DP]; /* soft bit of edge kk at the cyclic shift */
  int8_t* cp[DP]; /* c2v of edge kk */
  int     vc[DP]; /* v2c */
#pragma unroll
  for (int kk = 0; kk < DP; ++kk) {
    /* edge word shift | col * Z << 16 (wave-uniform, step_task); with splitting the two halves select per lane */
    const bool dummy = (P == 2 && D0 + kk >= D && half); /* upper half of an odd-degree row has one edge less */
    const uint32_t ew   = s_slot[kk];   /* this lane's edge (the upper half's slot starts at edge D0) */
    const uint32_t sh   = ew & 0xffffU;
    const uint32_t colz = ew >> 16;
    const uint32_t j0   = static_cast<uint32_t>(t) + sh;
    const uint32_t j    = min(j0, j0 - static_cast<uint32_t>(Z)); /* (t + shift) mod Z */
    sp[kk]              = lds_byte(colz + j); /* a dummy edge points at the scratch bytes */
    cp[kk]              = dummy ? s_soft + trash : cq;
    cq += Z; /* incremental: keeps the c2v addresses single VOP2 adds */
  }
  PHASE(1);
  int      av[DP];                     /* |v2c| */
  int      sg[DP];                     /* sign mask of v2c */
  uint32_t m1 = LLR_MAX, m2 = LLR_MAX; /* the reference's min and min2 (gen.cpp:46-68) */
  uint32_t sx = 0;                     /* sign parity of all v2c (bit 31) */
#pragma unroll
  for (int kk = 0; kk < DP; ++kk) {
    const bool dummy = (P == 2 && D0 + kk >= D && half);
    const int  v     = v2c_of(*sp[kk], *cp[kk]);
    vc[kk]           = v;
    const int sv     = sign_mask(v);
    sg[kk]           = sv;
    const int a      = dummy ? 0xfff : (v ^ sv) - sv;
    av[kk]           = a;
    scan_edge(m1, m2, a);
    sx ^= dummy ? 0U : static_cast<uint32_t>(v);
  }
  PHASE(2);
  /* c2v' of edge k = sign(v2c_k) * sign(parity) * (k == idx ? n2 : n1) (gen.cpp:93-105). The reference's idx is
   * the first edge with |v2c| == min; any other edge with |v2c| == min makes min2 == min, so "k == idx" can be
   * replaced by "|v2c_k| == min" without changing a single output, and no edge index is tracked. The parity's sign
   * is folded into the two magnitudes once per row. */
  int p1, p2;
  row_scale<P, SF08>(m1, m2, sx, half, sf, p1, p2);
  PHASE(3);
#pragma unroll
  for (int kk = 0; kk < DP; ++kk) {
    const int c = c2v_new(sg[kk], av[kk], m1, p1, p2);
    *cp[kk]     = static_cast<int8_t>(c);
    *sp[kk]     = static_cast<int8_t>(soft_new(c, vc[kk]));
  }
  PHASE(4);
}

/* Dispatch on the (wave-uniform) row degree. BG1 degrees: 3..10, 19; BG2: 3..10 (ldpc_luts_impl.cpp:4383-4519). */
template <int P, bool SF08>
__device__ __forceinline__ void row_dispatch(int deg, int t, int half, const uint32_t* s_slot, int8_t* s_soft,
                                             int8_t* c2v_row, float sf, int Z, int trash, uint64_t* ph)
{
  switch (deg) {
    case 3: row_update<3, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 4: row_update<4, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 5: row_update<5, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 6: row_update<6, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 7: row_update<7, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 8: row_update<8, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 9: row_update<9, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    case 10: row_update<10, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
    default: row_update<19, P, SF08>(t, half, s_slot, s_soft, c2v_row, sf, Z, trash, ph); break;
  }
}

} // namespace
} // namespace ldpc_hip
