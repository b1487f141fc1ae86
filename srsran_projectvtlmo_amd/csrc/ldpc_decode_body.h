/*
 * The specialised decoders' bodies: sp::dec (a whole iteration unrolled at compile time from a spec::sgraph) and
 * sp::qdec (the lane-split decoder of the one-wave graphs, spec::qgraph). decode_cb (ldpc_decode_cb.h) runs them; the
 * shared helpers, the generic row update, the work-queue loop and the diagnostics, which this header used to hold as
 * well, are in ldpc_device_util.h, ldpc_decode_row.h, ldpc_dwq_loop.h and ldpc_diag.h.
 */
#pragma once

#include <utility>

#include "ldpc_device_util.h"
#include "ldpc_diag.h"
#include "ldpc_spec.h"

namespace ldpc_hip {
namespace {

/* ---- specialised decoder: the whole iteration unrolled at compile time (ldpc_spec.h) ---------------------------
 * The step sequence and every row's degree, columns and shifts are constants, so a row needs no table reads, no
 * degree dispatch and no task fetch: its soft addresses are three VALU ops per edge (t + shift wrapped modulo Z), the
 * column offset being the LDS instruction's immediate. Split rows (P = 2) select the upper half's column and shift
 * per lane with a mask.
 *
 * Check-to-variable messages live in VGPRs, two edges per register (16-bit halves). A lane updates the same (row,
 * check node, edge pairs) in every iteration, so its c2v words never leave it: pair slot q of a row is register q of
 * the lane (srole::q0; the two wave groups' rows take slots independently, BG1 Z=384: 87 registers).
 *
 * A step's work sits inside its wave group's branch (addresses, soft reads, update, writes). Only the early part of a
 * pipelined single-row chain (ldpc_spec.h) crosses a barrier: its registers go through a fresh, undefined carry on
 * every other path, so no path keeps copies of them. */
namespace sp {

using spec::MAX_POS;

template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F& f, std::integer_sequence<int, I...>)
{
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f)
{
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

/* t, hmask and the address bases pass through opaque asm once per step: every address derived from them is
 * iteration-invariant, and without this the compiler hoists all of them out of the iteration loop (hundreds of live
 * registers, spilled). */
__device__ __forceinline__ uint32_t opaque(uint32_t x)
{
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint32_t opaque_s(uint32_t x)
{
  asm volatile("" : "+s"(x));
  return x;
}

/* Two 16-bit lanes per register (v_pk_* instructions: one issue for two edges of a check node). */
typedef short          s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 as_s(uint32_t x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u16x2 as_u(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t bits(s16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t bits(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ s16x2 splat(int v) { return s16x2{static_cast<short>(v), static_cast<short>(v)}; }
__device__ __forceinline__ u16x2 splatu(unsigned v)
{
  return u16x2{static_cast<unsigned short>(v), static_cast<unsigned short>(v)};
}

/* lane constants of the iteration */
struct lanes {
  uint32_t t1[2];   /* P = 1, wave group g: t = 64 * (wave - g W) + lane */
  uint32_t t2;      /* P = 2: t = 32 * wave + (lane & 31)                 */
  uint32_t hmask;   /* P = 2: 0 for lanes 0-31, ~0 for lanes 32-63        */
  int      wave, lane, nof_layers;
  uint32_t one2;    /* 0x00010001 as an SGPR constant (pass1's v_or: VOP2 with an SGPR source, not a 32-bit literal) */
  uint32_t abase;   /* LDS byte address of this lane's first word of the split-address table (lay.c2v + 4 tid) */
  uint32_t act[3];  /* wave-uniform role masks (SGPRs): bit S of act[0] / act[1] / act[2] set when this wave runs the
                       step's first role / second role / the next row's early part (dec::role_masks) */
};

/* Soft bits: int8 (ds_read_i8 / ds_write_b8), column c at c * Z; edge k of check node t reads and writes
 * c * Z + (t + shift) mod Z, the modulo as min(t + shift, t + shift - Z) in unsigned arithmetic. */
__device__ __forceinline__ int rd8(uint32_t base, uint32_t imm) { return *(lds_byte(base) + imm); }
__device__ __forceinline__ void wr8(uint32_t base, uint32_t imm, uint32_t v)
{
  *(lds_byte(base) + imm) = static_cast<int8_t>(v);
}
/* +infinity (the dummy position of an odd row, the scratch column) */
constexpr int SOFT_INF = 121;

/* pack the two sign-extended soft bits of an edge pair: [lo.b0, lo.b1, hi.b0, hi.b1]. One half-rate v_perm_b32. The
 * alternative without it, ds_read_i8_d16 / ds_read_i8_d16_hi (each zeroes the other half with SRAM ECC on) and one
 * full-rate v_or_b32, was built and lost: the compiler does not emit d16 loads for this target, and as inline asm with
 * their own s_waitcnt lgkmcnt(0) they are a block that the address arithmetic and the first pair's pass 1 no longer
 * overlap with (C2 +3 us, BG1 Z=128 +6.7 us against this form, profiles/r10/ab_pair_pack.txt). */
__device__ __forceinline__ uint32_t pack_pair(int lo, int hi)
{
  return __builtin_amdgcn_perm(static_cast<uint32_t>(hi), static_cast<uint32_t>(lo), 0x05040100U);
}
/* the two-minimum scan's start: 120 (strict <: infinity and +-120 never change it) */
constexpr unsigned MIN_START = 120U;

/* Pass 1 of an edge pair: v2c = soft (-) c2v per half, its magnitude a (+infinity -> 241) and the per-half
 * two-minimum and parity updates. Arithmetic note at pass2. */
__device__ __forceinline__ void pass1(uint32_t S, uint32_t C, u16x2& M1, u16x2& M2, uint32_t& SX, uint32_t& G,
                                      uint32_t& A, uint32_t one2)
{
  const s16x2 s  = as_s(S);
  const s16x2 d  = s - as_s(C);                               /* s - c                          */
  uint32_t    gb = bits(d >> 15) | one2; /* sign of v2c, +-1 (pass 2 uses it) */
  asm("" : "+v"(gb)); /* keeps |d| = d g: the compiler would rewrite it as max(d, -d), one instruction more */
  const s16x2 g  = as_s(gb);
  const s16x2 af = __builtin_elementwise_min(d * g, splat(120)); /* |clamp(s - c)|  */
  const s16x2 iv = s * s - splat(14400);                      /* 241 iff |s| = 121              */
  const u16x2 a  = as_u(bits(__builtin_elementwise_max(af, iv)));
  M2             = __builtin_elementwise_min(M2, __builtin_elementwise_max(M1, a));
  M1             = __builtin_elementwise_min(M1, a);
  SX ^= bits(g);
  G = bits(g);
  A = bits(a);
}

/* Pass 2 of an edge pair.
 * Arithmetic (int8 LLRs, llr.cpp:39-97; ldpc_decoder_generic.cpp:30-120), with the decoder-internal soft encoding of
 * +-121 for the reference's +-infinity (+-127):
 *   v2c   = isinf(s) ? s : clamp(s - c, +-120): its sign g is the sign of d = s - c in every case (|c| <= 96 < 121),
 *           and a = |v2c| = min(d g, 120) for a finite s, 241 for an infinite one (s^2 - 14400 > 0 only at |s| = 121);
 *           in the two-minimum scan (start 120, strict <) 241 behaves exactly like the reference's 127;
 *   the reference gives min2 to the first edge with |v2c| == min1 and min1 to the others; any other edge with
 *           |v2c| == min1 implies min2 == min1. With n = round(0.8 m) and every a >= m1 (a >= m2 unless a == m1):
 *           f = (a == m1) ? n2 : n1 = max(n1, n2 + m1 - a): for a >= m2 > m1, n2 - n1 <= floor(0.8 (m2 - m1) + 1)
 *           <= m2 - m1 <= a - m1;
 *   c2v'  = sign(v2c) * P * f   (P = +-1, the check node's sign parity);
 *   soft' = promotion_sum(c2v', v2c) = sign(v2c) * min(a + P f, 121): a + P f >= -96, and an infinite v2c (a = 241)
 *           stays at 121. */
__device__ __forceinline__ void pass2(uint32_t G, uint32_t A, s16x2 N1, s16x2 CC, s16x2 PP, uint32_t& Cnew,
                                      uint32_t& Snew)
{
  const s16x2 a  = as_s(A);
  const s16x2 g  = as_s(G);
  const s16x2 f  = __builtin_elementwise_max(N1, CC - a);
  const s16x2 pf = f * PP;
  const s16x2 u  = __builtin_elementwise_min(a + pf, splat(121));
  Snew           = bits(u * g);
  Cnew           = bits(pf * g);
}

/* the row's pass-2 constants as the words they are computed in: n = round(0.8 m) = (52432 m + 26216) >> 16 exactly for
 * m in [0, 120] (gen.cpp:70-79 with sf = 0.8f), cc = n2 + m1, and the check node's sign pp = +-1, which is valid in its
 * low half only (fold_halves). pass2 reads them through lo_splat (the packed instructions' op_sel: no instruction),
 * ext_update reads their low halves directly. */
__device__ __forceinline__ void row_consts(uint32_t m1, uint32_t m2, uint32_t sx, uint32_t& n1, uint32_t& cc, uint32_t& pp)
{
  n1                = (__umul24(m1, 52432U) + 26216U) >> 16;
  const uint32_t n2 = (__umul24(m2, 52432U) + 26216U) >> 16;
  cc                = n2 + m1;
  pp                = sx;
}
__device__ __forceinline__ s16x2 lo_splat(uint32_t w) { return splat(static_cast<short>(w)); }

/* full-rate 16-bit minimum of two words' low halves (the upper half of the result is zero); the compiler's own choice
 * for a three-way minimum is a shift, the half-rate v_min3_u16 and a mask */
__device__ __forceinline__ uint32_t min_lo16(uint32_t a, uint32_t b)
{
  uint32_t r;
  asm("v_min_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

/* The check node's two minima and parity from the per-half ones: min1 = min(A, B), min2 = min(min2_A, min2_B,
 * max(min1_A, min1_B)) -- the two smallest of the multiset, as the sequential scan finds them. Parity: each half of SX
 * is the XOR of +-1 values (0x0001 / 0xffff), so bits 1-15 of lo ^ hi all equal the parity of the negative signs, and
 * bit 0 the parity of the number of values. A row that XORed an odd number of them (an extension edge's sign and its
 * pairs) has the check node's sign, +-1, in the low 16 bits of sx as it is; any other row ORs 1 into it (sign_word). */
__device__ __forceinline__ void fold_halves(u16x2 M1, u16x2 M2, uint32_t SX, uint32_t& m1, uint32_t& m2, uint32_t& sx)
{
  m1 = __builtin_elementwise_min(M1.x, M1.y);
  m2 = min_lo16(__builtin_elementwise_min(M2.x, M2.y), __builtin_elementwise_max(M1.x, M1.y));
  sx = SX ^ (SX >> 16);
}
template <bool ODD>
__device__ __forceinline__ uint32_t sign_word(uint32_t sx)
{
  return ODD ? sx : (sx | 1U);
}

/* Merge of a split row's halves (lanes l and l ^ 32) through v_permlane32_swap: after the swap each lane holds its
 * own and its partner's values, so the merge is symmetric and needs no select. */
__device__ __forceinline__ void merge_partner(uint32_t& m1, uint32_t& m2, uint32_t& sx)
{
  const uint32_t pk = m1 | (m2 << 16);
  const auto     r  = __builtin_amdgcn_permlane32_swap(pk, pk, false, false);
  const auto     rs = __builtin_amdgcn_permlane32_swap(sx, sx, false, false);
  fold_halves(u16x2{static_cast<unsigned short>(r[0]), static_cast<unsigned short>(r[1])},
              u16x2{static_cast<unsigned short>(r[0] >> 16), static_cast<unsigned short>(r[1] >> 16)}, 0U, m1, m2, sx);
  sx = rs[0] ^ rs[1];
}

template <const spec::sgraph& G>
struct dec {
  static constexpr uint32_t Z       = static_cast<uint32_t>(G.Z); /* column stride: one int8 soft bit per byte */
  static constexpr int      NCR     = G.slots;
  static constexpr int      KC      = G.K + 4;                             /* first extension column */
  static constexpr uint32_t SCRATCH = static_cast<uint32_t>(G.N_full) * Z; /* dummy edges: soft +infinity */
  static constexpr int      P2_WAVES = (G.Z + 31) / 32;
  static_assert(G.valid && 2 * G.W <= 12 && P2_WAVES <= 12, "specialised schedule");

  using cr_t = uint32_t[NCR];

  /* byte offset of the column of edge e of row r (the ds immediate of its accesses); a dummy edge (e < 0) uses the
   * scratch column */
  static constexpr uint32_t off(int r, int e)
  {
    return e < 0 ? SCRATCH : static_cast<uint32_t>(G.rows[r].col[e]) * Z;
  }
  static constexpr uint32_t shift(int r, int e) { return e < 0 ? 0U : static_cast<uint32_t>(G.rows[r].sh[e]); }
  /* extension edge: a degree-1 column (>= K + 4) with shift 0, read and written by this row only */
  static constexpr bool     ext(int r, int e) { return e >= 0 && G.rows[r].col[e] >= KC && G.rows[r].sh[e] == 0; }
  static_assert(SCRATCH + Z <= 65535U, "column offsets are ds immediates");

  /* (t + sh) mod Z = min(t + sh, t + sh - Z) as unsigned (t < Z, sh < Z). v_min_u32 is a half-rate instruction; the
   * 16-bit VOP2 v_min_u16 issues at full rate and zeroes the upper half of its result (tools/ubench/README.md), and
   * x, x - Z mod 2^16 order the same way as in 32 bits (x < 2Z <= 2^16) */
  static __device__ __forceinline__ uint32_t wrap(uint32_t x)
  {
    uint32_t r;
    asm("v_min_u16_e32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(x - Z));
    return r;
  }

  template <int P, int GRP>
  static __device__ __forceinline__ bool lane_active(const lanes& L)
  {
    if constexpr (Z % 64 == 0) {
      return true;
    } else if constexpr (P == 2) {
      return L.t2 < Z;
    } else {
      return L.t1[GRP] < Z;
    }
  }

  /* address base and immediate of position j of a role */
  template <const spec::srole& RO, int J>
  static __device__ __forceinline__ uint32_t pos_base(const lanes& L)
  {
    constexpr int e0 = J < RO.npos ? RO.e0[J] : -1;
    if constexpr (RO.p == 1) {
      constexpr uint32_t sh = shift(RO.row, e0);
      return sh == 0 ? L.t1[RO.grp] : wrap(L.t1[RO.grp] + sh);
    } else {
      constexpr int      e1  = J < RO.npos ? RO.e1[J] : -1;
      constexpr uint32_t sh0 = shift(RO.row, e0), sh1 = shift(RO.row, e1);
      uint32_t           x   = L.t2;
      if constexpr (sh0 != 0 || sh1 != 0) {
        x = wrap(x + sh0 + (sh1 != sh0 ? (L.hmask & (sh1 - sh0)) : 0U));
      }
      constexpr uint32_t o0 = off(RO.row, e0), o1 = off(RO.row, e1);
      return o1 == o0 ? x : x + (L.hmask & (o1 - o0)); /* upper half: its own column */
    }
  }
  template <const spec::srole& RO, int J>
  static constexpr uint32_t pos_imm()
  {
    return off(RO.row, J < RO.npos ? RO.e0[J] : -1);
  }

  /* ---- extension edges kept in registers (ldpc_spec.h, ext_reg_edge) ----
   * State word X of a converted row, in the c2v slot its dropped pair left (srole: q0 + npos / 2): the low half is
   * a = |v2c| of the extension edge (0..120, or >= 241 once infinite), the high half its sign g (0x0001 / 0xffff),
   * which never changes. The v2c of a degree-1 column is the same at every visit until promotion_sum(c2v', v2c)
   * overflows, and +-infinity with the same sign from then on, so no soft bit and no c2v are kept for the edge and
   * nothing is written back: after the iterations nothing reads an extension column from LDS (the hard decision and
   * the early-stop check read soft[0, K Z) only; grep s_soft).
   * No compare and no select: 16-bit and 32-bit VOP2 operations, left to the compiler where it picks them itself. */
  /* full rate; the compiler fuses the product into a 64-bit multiply-add otherwise. Reads the low halves of its
   * sources and zeroes the high half of its result. */
  static __device__ __forceinline__ uint32_t mul_u16(uint32_t a, uint32_t b)
  {
    uint32_t r;
    asm("v_mul_lo_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }

  /* The state of an extension edge from its soft bit s (the prologue's LDS byte, +-121 = infinity): a = |s|, 241 for
   * an infinite one; g = +1 for s >= 0 (the sign of d = s - 0 in pass1). */
  static __device__ __forceinline__ uint32_t ext_state(int s)
  {
    const int      sv = s >> 31;
    const uint32_t a  = static_cast<uint32_t>((s ^ sv) - sv);
    return (a > static_cast<uint32_t>(LLR_MAX) ? 241U : a) | (static_cast<uint32_t>(sv | 1) << 16);
  }
  /* Before the first iteration (after the prologue's barrier): every converted row's state into its slot, from the
   * extension column's byte at the lane's own check node. A lane belongs to one wave group and loads that group's. */
  template <int S, int RI>
  static __device__ __forceinline__ void ext_init_role(cr_t& cr, const lanes& L)
  {
    static constexpr spec::srole ro = G.steps[S].r[RI];
    if constexpr (ro.row >= 0 && ro.xe >= 0) {
      static_assert(ro.p == 1 && (ro.npos & 1) == 0 && ro.q0 + ro.npos / 2 < NCR &&
                        ext(ro.row, ro.xe) && ro.xcol == G.rows[ro.row].col[ro.xe],
                    "extension edge in a register");
      if (L.t1[ro.grp] < Z) {
        cr[ro.q0 + ro.npos / 2] = ext_state(rd8(L.t1[ro.grp], static_cast<uint32_t>(ro.xcol) * Z));
      }
    }
  }
  template <int... Ss>
  static __device__ __forceinline__ void ext_init(cr_t& cr, const lanes& L, std::integer_sequence<int, Ss...>)
  {
    ((ext_init_role<Ss, 0>(cr, L), ext_init_role<Ss, 1>(cr, L)), ...);
  }
  static __device__ __forceinline__ void ext_init(cr_t& cr, const lanes& L)
  {
    ext_init(cr, L, std::make_integer_sequence<int, G.n_steps>{});
  }
  /* The extension edge in the row's scan. Its sign starts the parity (ext_seed); its magnitude joins the two minima
   * after the fold (ext_fold: the two smallest of a multiset do not depend on the order), as min(a, 120): an infinite
   * edge moves neither minimum. Seeding the packed scan with it instead (M1.lo = min(a, 120)) took the first pair's
   * shortcut away (a scan from the start value is one packed minimum, from a seed three) and two 32-bit literals. */
  static __device__ __forceinline__ void ext_seed(uint32_t X, uint32_t& SX) { SX = X >> 16; }
  static __device__ __forceinline__ void ext_fold(uint32_t X, uint32_t& m1, uint32_t& m2)
  {
    using u16 = unsigned short;
    const u16 a = __builtin_elementwise_min(static_cast<u16>(X), static_cast<u16>(MIN_START));
    m2          = __builtin_elementwise_min(static_cast<u16>(m2), __builtin_elementwise_max(static_cast<u16>(m1), a));
    m1          = __builtin_elementwise_min(static_cast<u16>(m1), a);
  }
  /* The visit's update from the row's pass-2 constants (row_consts: n1, n2 + m1 and P = +-1, the low halves of the
   * words row_consts leaves: no register beyond pass 2's and no splat): f = max(n1, n2 + m1 - a), u = a + P f, and a
   * becomes infinite when u >= 121, i.e. when promotion_sum(c2v', v2c) overflows (pass2's note; an infinite a gives
   * f = n1 and u >= 145, so it stays). The overflow ORs 255 into a, and a marker of 255 behaves like ext_state's 241
   * in every use: min(a, 120) = 120, n2 + m1 - a < 0 <= n1, u >= 145.
   * Plain 16-bit arithmetic but for the product: operations the compiler sees need no s_nop between them (after an
   * inline-asm result it inserts one before every dependent use), and it takes n1 from the high half of its
   * multiply-add by SDWA instead of shifting it down. */
  static __device__ __forceinline__ void ext_update(uint32_t& X, uint32_t n1, uint32_t cc, uint32_t pp)
  {
    const unsigned short a  = static_cast<unsigned short>(X);
    const short          f  = __builtin_elementwise_max(static_cast<short>(n1), static_cast<short>(cc - a));
    const uint32_t       pf = mul_u16(static_cast<uint32_t>(static_cast<unsigned short>(f)), pp);
    const unsigned short u  = static_cast<unsigned short>(a + pf);
    /* 120 - u is in [-231, 216]: upper byte 0xff when negative, else 0 */
    X |= static_cast<uint32_t>(static_cast<unsigned short>(120 - u) >> 8);
  }

  /* A row's pass-1 state kept in registers across the step barrier (pipelined single-row chains, ldpc_spec.h):
   * addresses, signs and v2c magnitudes of the early pairs, and the partial minima and parity. */
  struct carry {
    uint32_t base[MAX_POS];
    uint32_t gs[MAX_POS / 2], a[MAX_POS / 2];
    u16x2    m1, m2;
    uint32_t sx;
  };

  /* Split rows (P = 2): the upper half's column and shift differ from the lower half's at every position, so an
   * address costs 6-7 VALU ops (per-half deltas, wrap, column) against 3 on an unsplit row. BG1's four split rows have
   * 40 positions per lane whose addresses never change during a decode: they are computed once per context
   * (write_split_table) and kept as 16-bit halves of words (every LDS address is below 64 KiB).
   * Round 2 kept rows 0-1's pairs in 20 registers (the Z=384 kernel was at 168 VGPRs with 8 B/lane of spills; rows 0-1
   * against none: 149.1 -> 147.8 us, profiles/r02/split_addr.txt). Round 3 moved all four rows' pairs to the LDS table
   * below (152 VGPRs, no spill), which is what lets the kernel carry a second iteration loop (iteration_partial)
   * without spilling; the table words are read a step ahead (load_pf), so C2 is unchanged within 0.5%
   * (profiles/r03/partial_ab.txt).
   * Split rows [0, LDPC_SPEC_SPLIT_LDS_ROWS) keep their precomputed address pairs in LDS (one 32-bit word per pair and
   * lane, lane-contiguous: one conflict-free ds_read_b32 and two full-rate unpack ops per pair, against 6-7 VALU ops
   * per position computed in the step, and no registers held across the iteration). The table sits in the specialised
   * layout's c2v region (lay.c2v, unused there: c2v lives in registers); make_lds_layout reserves it
   * (spec::SPLIT_LDS_PAIRS). The prologue copies it from the context's global copy. Only BG1 graphs have the tables
   * (write_split_tables); split rows of BG2 graphs compute their addresses in the step. */
  static constexpr uint32_t WG = static_cast<uint32_t>(G.waves) * 64U; /* table stride: lanes per workgroup */
  static constexpr int lds_pairs_before(int S)
  {
    int n = 0;
    for (int s = 0; s < S; ++s) {
      const spec::srole& r = G.steps[s].r[0];
      n += (G.bg == 1 && r.p == 2 && r.row < LDPC_SPEC_SPLIT_LDS_ROWS) ? (r.npos + 1) / 2 : 0;
    }
    return n;
  }
  static_assert(lds_pairs_before(G.n_steps) <= spec::SPLIT_LDS_PAIRS, "make_lds_layout reserves the table");
  static_assert(static_cast<uint32_t>(spec::SPLIT_LDS_PAIRS) * WG * 4U <= 65536U, "table offsets are ds immediates");
  template <const spec::srole& RO>
  static constexpr bool pre_lds()
  {
    return G.bg == 1 && RO.p == 2 && RO.row < LDPC_SPEC_SPLIT_LDS_ROWS;
  }
  static_assert(lds_pairs_before(G.n_steps) * static_cast<int>(WG) <= SPLIT_TAB_STRIDE, "global split-table stride");
  static constexpr int LDS_PAIRS = lds_pairs_before(G.n_steps);

  /* The LDS-table words of a split step's address pairs, read one step ahead (at the start of the previous step,
   * whose barrier then covers their latency; step 0's at the end of the previous iteration or before the loop). */
  using pf_t = uint32_t[5];
  template <int S>
  static __device__ __forceinline__ void load_pf(pf_t& pf, const lanes& L)
  {
    if constexpr (S >= 0 && S < G.n_steps) {
      static constexpr spec::srole ro = G.steps[S].r[0];
      if constexpr (pre_lds<ro>()) {
        static_assert((ro.npos + 1) / 2 <= 5, "five address pairs per split row");
        constexpr int K0 = lds_pairs_before(S);
        static_for<(ro.npos + 1) / 2>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          pf[i]           = *lds_word(L.abase + static_cast<uint32_t>(K0 + i) * WG * 4U);
        });
      }
    }
  }

  /* The role's lane words pass through opaque asm once per step: every address is a function of them and
   * iteration-invariant, and is to be computed in the step, not hoisted. */
  template <const spec::srole& RO>
  static __device__ __forceinline__ lanes role_lanes(const lanes& L0)
  {
    lanes L = L0;
    if constexpr (RO.p == 2) {
      /* the upper half's per-position address deltas are iteration-invariant: computed here, not hoisted */
      L.t2    = opaque(L0.t2);
      L.hmask = opaque(L0.hmask);
    } else {
      L.t1[RO.grp] = opaque(L0.t1[RO.grp]);
    }
    return L;
  }

  /* The early part of the next step's row (sstep::e): reads and pass 1 of its first nearly positions. */
  template <int S>
  static __device__ __forceinline__ void role_early(cr_t& cr, carry& cy, const lanes& L0)
  {
    static constexpr spec::srole ro = G.steps[S].e;
    constexpr int                Q0 = ro.q0;
    constexpr int                NP = (ro.npos + 1) / 2;
    constexpr int                NE = ro.nearly / 2;
    const lanes                  L  = role_lanes<ro>(L0);
    if (!lane_active<1, ro.grp>(L)) {
      return;
    }
    int lo[NE], hi[NE];
    static_for<NE>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      cy.base[2 * i]     = pos_base<ro, 2 * i>(L);
      cy.base[2 * i + 1] = pos_base<ro, 2 * i + 1>(L);
      lo[i]              = rd8(cy.base[2 * i], pos_imm<ro, 2 * i>());
      hi[i]              = rd8(cy.base[2 * i + 1], pos_imm<ro, 2 * i + 1>());
    });
    /* the late positions' addresses too (no data dependency): off the completing waves' path in the next step */
    static_for<NP - NE>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = NE + decltype(ic)::value;
      cy.base[2 * i]     = pos_base<ro, 2 * i>(L);
      cy.base[2 * i + 1] = pos_base<ro, 2 * i + 1>(L);
    });
    u16x2    M1 = splatu(MIN_START), M2 = splatu(MIN_START);
    uint32_t SX = 0;
    if constexpr (ro.xe >= 0) { /* the parity starts with the sign of the extension edge kept in a register */
      ext_seed(cr[Q0 + NP], SX);
    }
    static_for<NE>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      pass1(pack_pair(lo[i], hi[i]), cr[Q0 + i], M1, M2, SX, cy.gs[i], cy.a[i], L.one2);
    });
    cy.m1 = M1;
    cy.m2 = M2;
    cy.sx = SX;
  }

  /* One role of step S: reads, pass 1 per edge pair (after the early pairs of the previous step, if any), the check
   * node's minima (and the split-row merge), the scaled magnitudes, pass 2 per pair and the soft-bit writes. */
  template <int S, int RI>
  static __device__ __forceinline__ void role(cr_t& cr, carry& cy, const lanes& L0, const pf_t& pf)
  {
    static constexpr spec::srole ro = G.steps[S].r[RI];
    constexpr int                Q0 = ro.q0;
    constexpr int                NP = (ro.npos + 1) / 2; /* pairs */
    constexpr int                NE = ro.nearly / 2;     /* pairs run early */
    constexpr bool               PRE = pre_lds<ro>(); /* split row: addresses precomputed, in the LDS table */
    const lanes                  L  = role_lanes<ro>(L0);
    if (!lane_active<ro.p, ro.grp>(L)) {
      return;
    }
    uint32_t base[2 * NP], Sx[NP], Gs[NP], A[NP];
    int      lo[NP], hi[NP];
    u16x2    M1 = splatu(MIN_START), M2 = splatu(MIN_START);
    uint32_t SX = 0;
    if constexpr (ro.xe >= 0 && NE == 0) { /* with early pairs, role_early seeded the parity */
      ext_seed(cr[Q0 + NP], SX);
    }
    if constexpr (NE > 0) {
      M1 = cy.m1;
      M2 = cy.m2;
      SX = cy.sx;
      static_for<NE>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        base[2 * i]     = cy.base[2 * i];
        base[2 * i + 1] = cy.base[2 * i + 1];
        Gs[i]           = cy.gs[i];
        A[i]            = cy.a[i];
      });
    }
    static_for<NP - NE>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = NE + decltype(ic)::value;
      if constexpr (NE > 0) { /* computed by the early role */
        base[2 * i]     = cy.base[2 * i];
        base[2 * i + 1] = cy.base[2 * i + 1];
      } else if constexpr (PRE) { /* full addresses from the LDS table, read ahead (load_pf); immediate 0 */
        const uint32_t w = pf[i];
        base[2 * i]      = w & 0xffffU;
        base[2 * i + 1]  = w >> 16;
      } else {
        base[2 * i]     = pos_base<ro, 2 * i>(L);
        base[2 * i + 1] = pos_base<ro, 2 * i + 1>(L);
      }
      lo[i]           = rd8(base[2 * i], PRE ? 0U : pos_imm<ro, 2 * i>());
      /* a position past the role's last (both halves dummy): +infinity without a read */
      hi[i] = (2 * i + 1 < ro.npos) ? rd8(base[2 * i + 1], PRE ? 0U : pos_imm<ro, 2 * i + 1>()) : SOFT_INF;
    });
    static_for<NP - NE>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = NE + decltype(ic)::value;
      Sx[i] = pack_pair(lo[i], hi[i]);
      if constexpr (i == NE) {
        SPEC_STAMP_FULL(S, 1);
      }
      pass1(Sx[i], cr[Q0 + i], M1, M2, SX, Gs[i], A[i], L.one2);
    });
    SPEC_STAMP_FULL(S, 2);
    uint32_t m1, m2, sx;
    fold_halves(M1, M2, SX, m1, m2, sx);
    if constexpr (ro.p == 2) {
      merge_partner(m1, m2, sx);
    }
    if constexpr (ro.xe >= 0) {
      ext_fold(cr[Q0 + NP], m1, m2);
    }
    /* n = round(0.8 m) (gen.cpp:70-79 with sf = 0.8f), n2 + m1, the sign parity; a row with an extension edge has
     * XORed 2 NP + 1 signs */
    uint32_t n1w, ccw, ppw;
    row_consts(m1, m2, sign_word<ro.xe >= 0 && ro.p == 1>(sx), n1w, ccw, ppw);
    const s16x2 N1 = lo_splat(n1w), CC = lo_splat(ccw), PP = lo_splat(ppw);
    SPEC_STAMP_FULL(S, 3);
    /* no soft bit and no c2v for the extension edge: its sticky infinity only. Its dependent operations come first
     * in program order: after the last pair's writes they were a chain of s_nop, one per operation */
    if constexpr (ro.xe >= 0) {
      ext_update(cr[Q0 + NP], n1w, ccw, ppw);
    }
    /* Graphs with one wave per row group (Z <= 64): every pair's pass 2 before any of its writes, so the scheduler
     * can interleave the pairs' chains (a packed op reading the previous one's result otherwise waits an s_nop); the
     * step is a latency chain there (BG2 Z=36: 65.8 -> 63.5 us per 128-CB batch). Larger graphs keep pass 2 and the
     * writes pair by pair (batched: BG1 Z=384 +1.5%, profiles/r03/p2_batch_ab.txt). */
    constexpr bool P2B = G.W == 1;
    uint32_t       snv[NP];
    if constexpr (P2B) {
      static_for<NP>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        pass2(Gs[i], A[i], N1, CC, PP, cr[Q0 + i], snv[i]);
      });
    }
    static_for<NP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      uint32_t      sn;
      if constexpr (P2B) {
        sn = snv[i];
      } else {
        pass2(Gs[i], A[i], N1, CC, PP, cr[Q0 + i], sn);
      }
      constexpr uint32_t i0 = PRE ? 0U : pos_imm<ro, 2 * i>(), i1 = PRE ? 0U : pos_imm<ro, 2 * i + 1>();
      wr8(base[2 * i], i0, sn);
      if constexpr (2 * i + 1 < ro.npos) { /* else a dummy: nothing to write */
        wr8(base[2 * i + 1], i1, sn >> 16);
      }
    });
  }

  /* Wave priority (s_setprio) on graphs with W >= 3 waves per group: in a pipelined chain the group completing a row
   * is on the step's critical path and the group running the next row's early part is not, so the arbiter issues the
   * completing waves first when both compete for a SIMD. C2 batch 150.4 -> 148.9 us, BG1 Z = 256 119.2 -> 116.8 us;
   * on BG2 Z = 128 (W = 2) it was 1% slower, so the smaller graphs keep equal priorities
   * (profiles/r02/prio.txt). */
  static constexpr bool WAVE_PRIO = true;
  template <int PR>
  static __device__ __forceinline__ void set_prio()
  {
    if constexpr (WAVE_PRIO && G.W >= 3) {
      __builtin_amdgcn_s_setprio(PR);
    }
  }

  /* cy: the state the early part of this step's row left (read by its role); on return, the state this step's early
   * role leaves for the next step. nx starts undefined, so on every path but the early role's the carried registers
   * are dead across the step (no copies to keep a value no later role on that wave reads). */
  template <int S, bool WRAP>
  static __device__ __forceinline__ void step(cr_t& cr, carry& cy, const lanes& L0, pf_t& pf)
  {
    pf_t cur;
    for (int i = 0; i < 5; ++i) {
      cur[i] = pf[i];
    }
    load_pf<(S + 1 < G.n_steps) ? S + 1 : (WRAP ? 0 : -1)>(pf, L0); /* the next split step's table words */
    SPEC_STAMP(S, 0);
    constexpr spec::sstep st = G.steps[S];
    carry                 nx;
    /* What this wave does in step S: at most one role (a wave belongs to one group; rows beyond the adaptive layer
     * count, impl.cpp:103-114, are skipped). One scalar bit test per role (role_masks). */
    constexpr uint32_t bit = 1U << S;
    /* the masks pass through opaque asm in every step: the tests are loop-invariant, and hoisted out of the iteration
     * loop they would hold one SGPR pair per step and role (spilled) */
    if ((opaque_s(L0.act[0]) & bit) != 0U) {
      set_prio<(st.r[0].p == 1 && (st.r[0].nearly > 0 || st.e.row >= 0)) ? 2 : 1>(); /* a chain row's completion */
      role<S, 0>(cr, cy, L0, cur);
    } else if constexpr (st.r[1].row >= 0) {
      if ((opaque_s(L0.act[1]) & bit) != 0U) {
        set_prio<1>();
        role<S, 1>(cr, cy, L0, cur);
      }
    } else if constexpr (st.e.row >= 0) {
      if ((opaque_s(L0.act[2]) & bit) != 0U) {
        set_prio<0>(); /* the early role has slack until the barrier: the completing group issues first */
        role_early<S>(cr, nx, L0);
      }
    }
    if constexpr (st.e.row >= 0 || st.r[0].nearly > 0) {
      cy = nx;
    }
#ifdef LDPC_HIP_DIAG_FULL
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    SPEC_STAMP(S, 4);
#endif
    __syncthreads();
    SPEC_STAMP(S, 5);
  }

  template <int... S>
  static __device__ __forceinline__ void iteration_impl(cr_t& cr, const lanes& L, pf_t& pf,
                                                        std::integer_sequence<int, S...>)
  {
    carry cy;
    (step<S, true>(cr, cy, L, pf), ...);
  }

  /* one full iteration; pf holds step 0's table words on entry (load_pf<0> before the loop) and on exit */
  static __device__ __forceinline__ void iteration(cr_t& cr, const lanes& L, pf_t& pf)
  {
    iteration_impl(cr, L, pf, std::make_integer_sequence<int, G.n_steps>{});
  }

  /* Codeblocks with few layers (high code rate: impl.cpp:103-114 adapts the layer count to the codeblock length, a
   * 6-layer BG1 Z=384 CB in C4's large TB). Steps run in row order, so once a step's first row is beyond the layer
   * count every later step is empty too; an empty step still costs every wave its scalar role checks (about 20 SALU
   * instructions per wave and step on the CU's one scalar unit: a 4-layer BG1 Z=384 iteration spent 6.0 us, 2.2 of
   * them in its 28 empty steps). Codeblocks with at most PARTIAL_LAYERS layers run this iteration instead: the first
   * PARTIAL_STEPS steps, ending at the first empty one. Full-length codeblocks keep the unchecked iteration (the
   * checks in every step cost C2 1-2%, profiles/r03/exit_ab.txt). */
  static constexpr int PARTIAL_LAYERS = 12;
  static constexpr int partial_steps()
  {
    int n = 0;
    while (n < G.n_steps && G.steps[n].r[0].row < PARTIAL_LAYERS) {
      ++n;
    }
    return n;
  }
  static constexpr int PARTIAL_STEPS = partial_steps();
  static constexpr bool HAS_PARTIAL  = PARTIAL_LAYERS > 0 && PARTIAL_STEPS < G.n_steps;
  template <int S>
  static __device__ __forceinline__ bool step_more(cr_t& cr, carry& cy, const lanes& L, pf_t& pf)
  {
    step<S, false>(cr, cy, L, pf);
    if constexpr (S + 1 < PARTIAL_STEPS) {
      return G.steps[S + 1].r[0].row < L.nof_layers;
    } else {
      return false;
    }
  }
  template <int... S>
  static __device__ __forceinline__ void partial_impl(cr_t& cr, const lanes& L, pf_t& pf,
                                                      std::integer_sequence<int, S...>)
  {
    carry cy;
    (void)(step_more<S>(cr, cy, L, pf) && ...);
  }
  static __device__ __forceinline__ void iteration_partial(cr_t& cr, const lanes& L)
  {
    pf_t pf;
    load_pf<0>(pf, L);
    partial_impl(cr, L, pf, std::make_integer_sequence<int, PARTIAL_STEPS>{});
  }

  /* Per-wave role masks, computed once per decode from the wave's group and the layer count. Deciding a step's role
   * from the wave index and the rows' layer tests in every step cost each wave about 20 scalar instructions per step,
   * and a CU has one scalar unit for its 12 waves. */
  static_assert(G.n_steps <= 32, "one mask bit per step");
  /* The masks from a few constexpr step masks and the layer count: rows are in step order, so the steps whose
   * first row is below nl are a prefix [0, n0(nl)) (n0 a constexpr table read with one scalar load); a step's
   * second row r + 1 is below nl iff r < nl - 1, and an early role runs the next step's first row. */
  struct mask_tab {
    uint32_t r0g[2], r1g[2], eg[2], p2;
    uint8_t  n0[64];
  };
  static constexpr mask_tab make_mask_tab()
  {
    mask_tab t{};
    for (int S = 0; S < G.n_steps; ++S) {
      const spec::sstep& st = G.steps[S];
      if (st.r[0].p == 2) {
        t.p2 |= 1U << S;
      } else {
        t.r0g[st.r[0].grp] |= 1U << S;
        if (st.r[1].row >= 0) {
          t.r1g[st.r[1].grp] |= 1U << S;
        }
        if (st.e.row >= 0) {
          t.eg[st.e.grp] |= 1U << S;
        }
      }
    }
    for (int nl = 0; nl < 64; ++nl) {
      int n = 0;
      while (n < G.n_steps && G.steps[n].r[0].row < nl) {
        ++n;
      }
      t.n0[nl] = static_cast<uint8_t>(n);
    }
    return t;
  }
  static constexpr mask_tab MT = make_mask_tab();
  static __device__ __forceinline__ uint32_t prefix(int n) { return n >= 32 ? ~0U : ((1U << n) - 1U); }
  static __device__ __forceinline__ void role_masks(lanes& L)
  {
    const mask_tab&           t   = MT;
    const int                 nl  = L.nof_layers < 63 ? L.nof_layers : 63;
    const int                 n0  = t.n0[nl];
    const int                 n0m = t.n0[nl > 0 ? nl - 1 : 0];
    const uint32_t            pre0 = prefix(n0), pre1 = prefix(n0m), pree = prefix(n0 > 0 ? n0 - 1 : 0);
    uint32_t                  a0 = (L.wave < P2_WAVES) ? (t.p2 & pre0) : 0U, a1 = 0, ae = 0;
    if (L.wave < 2 * G.W) {
      const int grp = L.wave < G.W ? 0 : 1;
      a0 |= t.r0g[grp] & pre0;
      a1 = t.r1g[grp] & pre1;
      ae = t.eg[grp] & pree;
    }
    L.act[0] = opaque_s(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a0))));
    L.act[1] = opaque_s(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a1))));
    L.act[2] = opaque_s(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ae))));
  }

  static __device__ __forceinline__ lanes make_lanes(int wave, int lane, int nof_layers, uint32_t abase)
  {
    lanes L{};
    L.abase      = abase;
    L.wave       = wave;
    L.lane       = lane;
    L.nof_layers = nof_layers;
    L.one2       = opaque_s(0x00010001U);
    for (int i = 0; i < 2; ++i) { /* byte offsets of the lane's check node */
      L.t1[i] = static_cast<uint32_t>((wave - i * G.W) * 64 + lane);
    }
    L.t2    = static_cast<uint32_t>(wave * 32 + (lane & 31));
    L.hmask = (lane >= 32) ? 0xffffffffU : 0U;
    role_masks(L);
    return L;
  }

  /* The split-row address table of this graph into global memory (ldpc_split_table_kernel, once per context): word
   * (pair index) * WG + tid holds the full LDS addresses of the lane's positions 2 i and 2 i + 1 of a split row, so a
   * codeblock's prologue copies them instead of computing them (about 300 VALU instructions per lane, 1.1 us per
   * codeblock at Z = 384). */
  template <int S>
  static __device__ __forceinline__ void write_split_step(uint32_t* __restrict__ gdst, const lanes& L)
  {
    static constexpr spec::srole ro = G.steps[S].r[0];
    if constexpr (pre_lds<ro>()) {
      constexpr int K0 = lds_pairs_before(S);
      static_for<(ro.npos + 1) / 2>([&](auto ic) __attribute__((always_inline)) {
        constexpr int  i  = decltype(ic)::value;
        const uint32_t lo = pos_base<ro, 2 * i>(L) + pos_imm<ro, 2 * i>();
        const uint32_t hi = (2 * i + 1 < ro.npos) ? pos_base<ro, 2 * i + 1>(L) + pos_imm<ro, 2 * i + 1>() : 0U;
        if (L.wave < P2_WAVES) {
          gdst[static_cast<uint32_t>(K0 + i) * WG + static_cast<uint32_t>(L.wave * 64 + L.lane)] =
              (lo & 0xffffU) | (hi << 16);
        }
      });
    }
  }
  static __device__ __forceinline__ void write_split_table(uint32_t* gdst, int wave, int lane)
  {
    const lanes L = make_lanes(wave, lane, 64, 0U);
    static_for<G.n_steps>([&](auto sc) __attribute__((always_inline)) {
      write_split_step<decltype(sc)::value>(gdst, L);
    });
  }
};

/* ---- lane-split decoder of the one-wave graphs (spec::qgraph, ldpc_spec.h) ----------------------------------------
 * Step S: a two-row step runs row r[0] on waves [0, WH) and row r[1] on waves [WH, 2 WH), P2 lanes per check node
 * (lane i of a group: check node i / P2, edges i % P2 + P2 j); a single-row step runs its row on every wave, 2 P2
 * lanes per check node. Per lane and step: its address pairs and c2v pairs sit in the step's register slots [q0, q0 + nq)
 * (the same slots for both roles of a step: each lane runs one role), the reads, pass 1 of each edge pair, the merge of
 * the check node's partial minima and parity across its lanes (DPP), the scaled magnitudes, pass 2 and the writes,
 * then the step barrier. Positions without an edge address the scratch column held at +infinity. */
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v)
{
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false));
}

/* merge of two lanes' (min1, min2, parity): the two smallest of the multiset and the XOR of the parities */
template <int CTRL>
__device__ __forceinline__ void merge_lanes(uint32_t& m1, uint32_t& m2, uint32_t& sx)
{
  const uint32_t o1 = dpp_mov<CTRL>(m1), o2 = dpp_mov<CTRL>(m2), os = dpp_mov<CTRL>(sx);
  m2 = min(min(m2, o2), max(m1, o1));
  m1 = min(m1, o1);
  sx ^= os;
}

template <const spec::sgraph& G, const spec::qgraph& Q>
struct qdec {
  static constexpr int      Z       = G.Z;
  static constexpr int      NS      = Q.slots;
  static constexpr uint32_t WG      = static_cast<uint32_t>(Q.waves) * 64U; /* table stride: lanes per workgroup */
  static constexpr uint32_t SCRATCH = static_cast<uint32_t>(G.N_full) * static_cast<uint32_t>(Z);
  static_assert(Q.valid && SCRATCH + Z <= 65535U, "lane-split schedule: 16-bit LDS addresses");
  using cr_t = uint32_t[NS];

  struct qlanes {
    uint32_t one2; /* lanes::one2 */
    int      nof_layers, grp;
    bool     act2, act1; /* this lane's check node exists (t < Z) in a two-row / a single-row step */
  };
  static __device__ __forceinline__ qlanes make_lanes(int wave, int lane, int nof_layers)
  {
    qlanes L{};
    L.one2       = opaque_s(0x00010001U);
    L.nof_layers = nof_layers;
    L.grp        = wave < Q.WH ? 0 : 1;
    L.act2       = ((wave - L.grp * Q.WH) * 64 + lane) / Q.P2 < Z;
    L.act1       = (wave * 64 + lane) / (2 * Q.P2) < Z;
    return L;
  }

  /* The address table (ldpc_split_table_kernel, once per context): word (q0 + i) * WG + tid holds the LDS addresses
   * of the lane's positions 2 i and 2 i + 1 in the step's role, soft[col][(t + shift) mod Z] (scratch: no edge). */
  template <int S>
  static __device__ __forceinline__ void write_table_step(uint32_t* dst, int wave, int lane)
  {
    constexpr spec::qstep st   = Q.steps[S];
    constexpr bool        pair = st.r[1].row >= 0;
    const int             ri   = (pair && wave >= Q.WH) ? 1 : 0;
    const int             P    = pair ? Q.P2 : 2 * Q.P2;
    const int             i    = pair ? (wave - ri * Q.WH) * 64 + lane : wave * 64 + lane;
    const int             t = i / P, k = i % P;
    int                   col[spec::MAX_DEG], sh[spec::MAX_DEG], deg = 0, npos = 0;
    static_for<2>([&](auto rc) __attribute__((always_inline)) {
      constexpr int R = decltype(rc)::value;
      if constexpr (R == 0 || pair) {
        constexpr spec::srow row = G.rows[st.r[R].row];
        if (ri == R) {
          deg  = row.deg;
          npos = st.r[R].npos;
          static_for<spec::MAX_DEG>([&](auto ec) __attribute__((always_inline)) {
            constexpr int e = decltype(ec)::value;
            col[e]          = row.col[e];
            sh[e]           = row.sh[e];
          });
        }
      }
    });
    for (int q = 0; q < st.nq; ++q) {
      uint32_t a[2];
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * q + h, e = k + P * j;
        a[h]        = SCRATCH;
        if (t < Z && j < npos && e < deg) {
          a[h] = static_cast<uint32_t>(col[e] * Z + (t + sh[e]) % Z);
        }
      }
      dst[static_cast<uint32_t>(st.q0 + q) * WG + static_cast<uint32_t>(wave * 64 + lane)] = a[0] | (a[1] << 16);
    }
  }
  template <int... Ss>
  static __device__ __forceinline__ void write_table(uint32_t* dst, int wave, int lane, std::integer_sequence<int, Ss...>)
  {
    (write_table_step<Ss>(dst, wave, lane), ...);
  }

  template <int S, int RI>
  static __device__ __forceinline__ void role(cr_t& cr, const cr_t& tab, const qlanes& L)
  {
    constexpr spec::qstep st = Q.steps[S];
    constexpr spec::qrole ro = st.r[RI];
    constexpr int         NP = (ro.npos + 1) / 2;
    constexpr int         Q0 = st.q0;
    if (!(ro.P == Q.P2 ? L.act2 : L.act1)) {
      return;
    }
    uint32_t base[2 * NP], Gs[NP], A[NP];
    int      lo[NP], hi[NP];
    static_for<NP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int  i = decltype(ic)::value;
      const uint32_t w = opaque(tab[Q0 + i]); /* read in the step: not hoisted out of the iteration loop */
      base[2 * i]      = w & 0xffffU;
      base[2 * i + 1]  = w >> 16;
      lo[i]            = rd8(base[2 * i], 0);
      hi[i]            = (2 * i + 1 < ro.npos) ? rd8(base[2 * i + 1], 0) : SOFT_INF;
    });
    SPEC_STAMP_FULL(S, 1);
    u16x2    M1 = splatu(MIN_START), M2 = splatu(MIN_START);
    uint32_t SX = 0;
    static_for<NP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      pass1(pack_pair(lo[i], hi[i]), cr[Q0 + i], M1, M2, SX, Gs[i], A[i], L.one2);
    });
    uint32_t m1, m2, sx;
    fold_halves(M1, M2, SX, m1, m2, sx);
    merge_lanes<0xb1>(m1, m2, sx); /* quad_perm [1, 0, 3, 2]: the lane pair */
    if constexpr (ro.P >= 4) {
      merge_lanes<0x4e>(m1, m2, sx); /* quad_perm [2, 3, 0, 1]: the other pair of the quad */
    }
    if constexpr (ro.P >= 8) {
      merge_lanes<0x141>(m1, m2, sx); /* row_half_mirror: the other quad of the eight lanes */
    }
    static_assert(ro.P == 2 || ro.P == 4 || ro.P == 8, "lanes per check node");
    SPEC_STAMP_FULL(S, 2);
    uint32_t n1w, ccw, ppw; /* round(0.8 m), gen.cpp:70-79; n2 + m1; the sign parity */
    row_consts(m1, m2, sign_word<false>(sx), n1w, ccw, ppw);
    const s16x2 N1 = lo_splat(n1w), CC = lo_splat(ccw), PP = lo_splat(ppw);
    SPEC_STAMP_FULL(S, 3);
    uint32_t snv[NP];
    static_for<NP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      pass2(Gs[i], A[i], N1, CC, PP, cr[Q0 + i], snv[i]);
    });
    static_for<NP>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      wr8(base[2 * i], 0, snv[i]);
      if constexpr (2 * i + 1 < ro.npos) {
        wr8(base[2 * i + 1], 0, snv[i] >> 16);
      }
    });
  }

  /* false when the step's first row is beyond the codeblock's layers (impl.cpp:103-114): rows go in step order, so
   * this and every later step of the iteration are empty */
  template <int S>
  static __device__ __forceinline__ bool step(cr_t& cr, const cr_t& tab, const qlanes& L)
  {
    constexpr spec::qstep st = Q.steps[S];
    if (st.r[0].row >= L.nof_layers) {
      return false;
    }
    SPEC_STAMP(S, 0);
    if constexpr (st.r[1].row >= 0) {
      if (L.grp == 0) {
        role<S, 0>(cr, tab, L);
      } else if (st.r[1].row < L.nof_layers) {
        role<S, 1>(cr, tab, L);
      }
    } else {
      role<S, 0>(cr, tab, L);
    }
#ifdef LDPC_HIP_DIAG_FULL
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    SPEC_STAMP(S, 4);
#endif
    __syncthreads();
    SPEC_STAMP(S, 5);
    return true;
  }
  template <int... S>
  static __device__ __forceinline__ void iteration_impl(cr_t& cr, const cr_t& tab, const qlanes& L,
                                                        std::integer_sequence<int, S...>)
  {
    (void)(step<S>(cr, tab, L) && ...);
  }
  static __device__ __forceinline__ void iteration(cr_t& cr, const cr_t& tab, const qlanes& L)
  {
    iteration_impl(cr, tab, L, std::make_integer_sequence<int, Q.n_steps>{});
  }
};

} // namespace sp

} // namespace
} // namespace ldpc_hip
