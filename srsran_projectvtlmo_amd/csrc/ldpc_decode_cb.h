/*
 * gfx950 (MI355X, CDNA4) decoder kernels of the 5G-NR PUSCH LDPC decode path.
 *
 *  ldpc_decode_kernel          layered normalised min-sum decoder, one workgroup per codeblock with the whole decoder
 *                              state resident in LDS: int8 soft bits (N_full x Z) and one compressed check-to-variable
 *                              record per lifted check node (BG1 Z=384: 26 KiB + 75 KiB). Bit-exact with
 *                              ldpc_decoder_generic (lib/phy/upper/channel_coding/ldpc/ldpc_decoder_impl.cpp:60-308,
 *                              ldpc_decoder_generic.cpp:30-128) including the CRC early stop.
 *
 * Work mapping of the decoder. A base-graph row m lifts to Z independent check nodes t. A 64-lane wave takes 64 (or,
 * with edge splitting, 32) consecutive check nodes of one row, so the row -- degree, edge list, shifts -- is
 * wave-uniform and read through the scalar unit, while the Zc cyclic shift is a per-lane LDS byte gather
 * soft[col][(t + shift) mod Z]. The two-minimum search of a check node runs over the row's edges in the reference's
 * order with its strict '<' (first edge wins). Consecutive rows that share no variable node form one step and are
 * updated concurrently, one barrier per step: they read and write disjoint soft bits, so the result is identical to
 * the layer-serial order of ldpc_decoder_impl.cpp:116-123.
 */
#pragma once

#include "ldpc_decode_row.h"
#include "ldpc_decode_body.h"
#include "ldpc_dematch_body.h" /* dematch_body: the decode kernels' fused first phase */
#include "ldpc_dwq_loop.h"

namespace ldpc_hip {

namespace {

/* hard_decision (log_likelihood_ratio.cpp:226-252) of soft[0, K*Z) into LDS packed bytes.
 * Returns true (block-uniform) iff no soft bit is zero. Eight soft bits per thread come in with one 8-byte LDS read
 * (the soft region extends past K*Z, so the last read stays inside it). The block-wide "any zero" goes through the
 * LDS word *s_flag, which holds the token of the last call that found a zero: token must differ between calls, so
 * the flag never needs a reset (and the kernel's LDS stays all dynamic). ZC: Z when it is a compile-time constant
 * (specialised kernel), else 0. */
/* Per byte of four soft bits: t = (w & 0x7f..) + 0x7f.. has a byte's bit 7 set iff its low seven bits are not all
 * zero, so (w | ~t) & 0x80.. marks s <= 0 (the hard bit) and ~(w | t) & 0x80.. marks s == 0. gather4 packs the four
 * marks (bits 7, 15, 23, 31) into a nibble, soft bit 0 first: (m >> 7) * 0x80402010 puts mark j at bit 31 - j and
 * every cross term at a bit of its own below 28 or above 31 (no carries). */
__device__ __forceinline__ uint32_t gather4(uint32_t m) { return ((m >> 7) * 0x80402010U) >> 28; }

template <int ZC = 0>
__device__ __forceinline__ bool block_hard_decision(const int8_t* soft, uint8_t* hb, int KZ, uint32_t* s_flag,
                                                    uint32_t token, int Z = 0, int stride = 0, int read_off = 0)
{
  const int nb   = (KZ + 7) / 8;
  bool      zero = false;
  const int zc = ZC > 0 ? ZC : Z;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    int pos = 8 * b;
    if (stride != 0) {
      /* column-strided copies (specialised kernel, Z % 8 == 0: the 8 bits of a byte share a column) */
      const int col = pos / zc;
      pos           = col * stride + read_off + (pos - col * zc);
    }
    const uint2    w     = *reinterpret_cast<const uint2*>(soft + pos);
    const uint32_t keep  = 0xff00U >> min(8, KZ - 8 * b); /* valid bits of the last byte */
    const uint32_t tx    = (w.x & 0x7f7f7f7fU) + 0x7f7f7f7fU, ty = (w.y & 0x7f7f7f7fU) + 0x7f7f7f7fU;
    const uint32_t hard  = (gather4((w.x | ~tx) & 0x80808080U) << 4) | gather4((w.y | ~ty) & 0x80808080U);
    const uint32_t zeros = (gather4(~(w.x | tx) & 0x80808080U) << 4) | gather4(~(w.y | ty) & 0x80808080U);
    zero                 = zero || (zeros & keep) != 0;
    hb[b]                = static_cast<uint8_t>(hard & keep);
  }
  if (__builtin_amdgcn_ballot_w64(zero) != 0 && (threadIdx.x & 63) == 0) {
    *reinterpret_cast<volatile uint32_t*>(s_flag) = token;
  }
  __syncthreads();
  return *reinterpret_cast<volatile uint32_t*>(s_flag) != token;
}

} // namespace

/* Lifted graphs of every (BG, Z), indexed by slot = (BG - 1) * 51 + lifting position; slot 102 + s holds graph s
 * with the narrow step schedule (ldpc_graph.h NARROW_SLOT_BASE). Constant memory: all row, step and edge words are
 * read with scalar loads (the row a wave works on is uniform). One copy per translation unit (static): the one
 * ldpc_hip_kernels.hip uploads serves the generic and mixed kernels; the specialised kernels compiled elsewhere
 * (ldpc_spec_unit.hip) take every graph field from their compile-time schedule and never read it. */
static __constant__ graph_desc c_graphs[204];

/* Graph fields of the generic body (this unit's c_graphs). */
__device__ __forceinline__ int graph_field_Z(int slot) { return c_graphs[slot].Z; }
__device__ __forceinline__ int graph_field_K(int slot) { return c_graphs[slot].K; }
__device__ __forceinline__ int graph_field_N(int slot) { return c_graphs[slot].N_full; }
__device__ __forceinline__ int graph_field_task_waves(int slot) { return c_graphs[slot].task_waves; }

/* One codeblock per workgroup (the body of ldpc_decode_kernel and ldpc_decode_mixed_kernel). The generic body also
 * runs in workgroups wider than its schedule (mixed launches): waves at or beyond graph->task_waves only take part in
 * the block-wide phases and the step barriers. */
template <bool SF08, int SPEC_ID>
__device__ __forceinline__ void decode_cb(const dec_cb& d, int graph_slot, const step_task* __restrict__ tasks,
                                          const lds_layout& lay, const int8_t* llr_base,
                                          uint8_t* __restrict__ out_base, ldpc_hip_cb_result* __restrict__ res_base,
                                          const uint32_t* __restrict__ crc_tables, const dematch_cb* dm_cbs,
                                          const dematch_cb& dm_one)
{
#define graph (&c_graphs[graph_slot])
  constexpr bool SPEC = SPEC_ID >= 0; /* specialised body: spec::k_specs[SPEC_ID] */
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int8_t*   s_soft = reinterpret_cast<int8_t*>(smem); /* lay.soft == 0: column offsets are LDS addresses */
  if (static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_i8*)s_soft)) != 0U || lay.soft != 0U) {
    __builtin_trap(); /* lds_byte() would address the wrong bytes */
  }
  int8_t*   s_c2v  = reinterpret_cast<int8_t*>(smem + lay.c2v);
  uint8_t*  s_hb   = smem + lay.hard;
  uint32_t* s_red  = reinterpret_cast<uint32_t*>(smem + lay.red);
  uint32_t* s_crct = reinterpret_cast<uint32_t*>(smem + lay.crct);

  CB_STAMP_ENTRY(); /* diagnostic build (ldpc_diag.h): before a fused dematcher */
  if (dm_cbs != nullptr || dm_one.soft != nullptr) {
    /* fused rate dematching (ldpc_hip_dematch_decode_launch, the HAL batch): this CB's dematcher runs first, into the
     * soft buffer the prologue then loads (llr_base + d.llr_offset); its LDS staging and table copy sit in the
     * decoder's dynamic LDS (the launch reserves DM_FUSED_LDS), free again after the barrier. A workgroup's own
     * global stores are visible to its loads after the barrier. */
    dematch_body(dm_cbs != nullptr ? dm_cbs[blockIdx.x] : dm_one,
                 *reinterpret_cast<const demod_tables*>(crc_tables + DTAB_OFFSET), reinterpret_cast<int8_t*>(smem),
                 *reinterpret_cast<demod_tables*>(smem + DM_STAGE));
    __syncthreads();
  }
  if (d.keep_passed != 0 && res_base != nullptr && res_base[d.result_index].crc_pass != 0) {
    return; /* HARQ: CRC passed in an earlier transmission; message and result stay (pusch_decoder_impl.cpp:336-346) */
  }
  const int     tid    = threadIdx.x;
  const int     nthr   = blockDim.x;
  const int     lane   = tid & 63;
  const int     wave   = __builtin_amdgcn_readfirstlane(tid >> 6);
  /* the specialised bodies take every graph field from their compile-time schedule: they may be compiled in a unit
   * whose c_graphs copy is never uploaded (ldpc_spec_unit.hip) */
  using SG             = spec::spec_graph<SPEC ? SPEC_ID : 0>;
  const int     Z      = SPEC ? SG::g.Z : graph_field_Z(graph_slot);
  const int     K      = SPEC ? SG::g.K : graph_field_K(graph_slot);
  const int     N_full = SPEC ? SG::g.N_full : graph_field_N(graph_slot);
  const int     KZ     = K * Z;
  const int     L      = static_cast<int>(d.llr_length);
  const int8_t* llr    = llr_base + d.llr_offset;
  uint8_t*      out    = out_base + d.out_offset;
  const float   sf     = d.scaling_factor;

  CB_STAMP(0);
  /* ---- prologue: soft bits (load_soft_bits, impl.cpp:149-174), CRC tables, zeroed c2v records ----
   * Every global load a thread needs is issued before any of them is used (the LLRs, up to PRO_U 16-byte loads per
   * thread and pass, then the CRC tables), so their latencies overlap instead of adding up loop trip by loop trip;
   * the last non-zero LLR index is reduced per wave (DPP) into s_red[wave], so no barrier is needed before it. */
  int       last_local = 0;
  const int total      = N_full * Z;
  const bool vec16     = (reinterpret_cast<uintptr_t>(llr) & 15U) == 0 && ((2 * Z) & 15) == 0 && (L & 15) == 0;
  constexpr int PRO_U  = 4;
  const int z4 = (2 * Z) / 16, l4 = L / 16, t4 = (total + 15) / 16;
  const uint4* g4 = reinterpret_cast<const uint4*>(llr);
  uint4        pv[PRO_U];
  int          base4 = 0;
  if (vec16) { /* first pass's loads: [0, 2Z) zero, [2Z, 2Z + L) LLRs, rest zero */
#pragma unroll
    for (int u = 0; u < PRO_U; ++u) {
      const int i = tid + u * nthr;
      pv[u]       = (i >= z4 && i < z4 + l4 && i < t4) ? g4[i - z4] : make_uint4(0, 0, 0, 0);
    }
  }
  /* BG1 split-row address table (specialised kernel): the context's global copy, 16 bytes per load, its loads in
   * flight with the LLRs'; stored into the c2v region before the prologue barrier (a thread writes other lanes' words) */
  using SD                = sp::dec<SG::g>;
  /* one-wave graphs: the lane-split decoder (sp::qdec); its address table comes into registers here, its loads in
   * flight with the LLRs' (the same words for every codeblock of a launch: L2-resident after the first) */
  constexpr bool QUAD     = SPEC && spec::is_quad(SG::g);
  constexpr int  QN       = QUAD ? SG::q.slots : 1;
  using QD                = sp::qdec<SG::g, SG::q>;
  uint32_t      qtab[QN];
  if constexpr (QUAD) {
    const uint32_t* gq = crc_tables + lay.split_tab;
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      qtab[q] = gq[static_cast<uint32_t>(q) * QD::WG + static_cast<uint32_t>(tid)];
    }
  }
  constexpr int SPLIT_U4  = (SPEC && !QUAD) ? SD::LDS_PAIRS * static_cast<int>(SD::WG) / 4 : 0;
  constexpr int SPLIT_PER = 5; /* loads per thread: LDS_PAIRS / 4 at the decoder's own width */
  uint4         stv[SPLIT_PER];
  if constexpr (SPLIT_U4 > 0) {
    const uint4* gs = reinterpret_cast<const uint4*>(crc_tables + lay.split_tab);
#pragma unroll
    for (int u = 0; u < SPLIT_PER; ++u) {
      const int i = tid + u * nthr;
      stv[u]      = i < SPLIT_U4 ? gs[i] : make_uint4(0, 0, 0, 0);
    }
  }
  /* CRC tables for the LDS copy (T_0, T_1..T_3, x^(32 e) mod G: 324 16-byte chunks, every source 16-byte aligned):
   * issued here with the LLRs' and the split table's loads, stored after the LLRs. Round 4 had a loop of two 4-byte
   * loads per trip before the LLR loads: five dependent trips in a 128-thread workgroup (BG2 Z=36), most of its
   * 5 us prologue on the work-queue path. */
  constexpr int   CRC_U4  = CRC_LDS_WORDS / 4;
  constexpr int   CRC_PER = 3; /* loads per thread in flight: every chunk at 108 threads or more */
  static_assert(CRC_LDS_WORDS % 4 == 0 && 256 % 4 == 0 && CRC_TABLE_SIZE % 4 == 0 && CRC_SLICE_OFFSET % 4 == 0 &&
                    CRC_SLICE_WORDS % 4 == 0,
                "CRC tables copied in 16-byte chunks");
  const bool      crc_on = d.crc_mode != LDPC_HIP_CRC_MODE_NONE;
  const uint4*    tab4   = reinterpret_cast<const uint4*>(crc_tables + static_cast<int>(d.crc_poly) * CRC_TABLE_SIZE);
  const uint4*    slc4 =
      reinterpret_cast<const uint4*>(crc_tables + CRC_SLICE_OFFSET + static_cast<int>(d.crc_poly) * CRC_SLICE_WORDS);
  auto crc_chunk = [&](int j) { return j < 64 ? tab4[j] : (j < 256 ? slc4[j - 64] : tab4[j - 192]); };
  uint4 crcv[CRC_PER];
  if (crc_on) {
#pragma unroll
    for (int u = 0; u < CRC_PER; ++u) {
      const int j = tid + u * nthr;
      crcv[u]     = j < CRC_U4 ? crc_chunk(j) : make_uint4(0, 0, 0, 0);
    }
  }
  {
    uint4*    c2v4 = reinterpret_cast<uint4*>(s_c2v);
    int       n16  = 0; /* specialised: c2v in registers */
    if constexpr (!SPEC) {
      n16 = (static_cast<int>(graph->c2v_bytes) + 15) / 16;
    }
    for (int i = tid; i < n16; i += nthr) {
      c2v4[i] = make_uint4(0, 0, 0, 0);
    }
    const int nhb = static_cast<int>(lay.red - lay.hard) / 4;
    for (int i = tid; i < nhb; i += nthr) {
      reinterpret_cast<uint32_t*>(s_hb)[i] = 0;
    }
  }
  if constexpr (SPEC) {
    /* dummy edges of odd split rows read and write a scratch column held at +infinity (+121): never a minimum, no
     * sign, and promotion_sum keeps it there (namespace sp) */
    const int n4 = (static_cast<int>(lay.soft_stride) + 3) / 4; /* whole column (the layout leaves 64 bytes of slack) */
    int*      sc = reinterpret_cast<int*>(s_soft + static_cast<int>(lay.soft_stride) * N_full);
    for (int i = tid; i < n4; i += nthr) {
      sc[i] = 0x79797979; /* 121 = 0x79 in every byte */
    }
  } else {
    /* edge table: per row EDGE_SLOT words shift | (col * Z) << 16, padded with dummy edges at the scratch bytes after
     * the soft columns */
    uint32_t*      s_edges = reinterpret_cast<uint32_t*>(smem + lay.edges);
    const uint32_t dummy   = static_cast<uint32_t>(graph->N_full) * graph->Z << 16;
    for (int i = tid; i < graph->M * EDGE_SLOT; i += nthr) {
      const int      r   = i / EDGE_SLOT, k = i - r * EDGE_SLOT;
      const uint32_t rw  = graph->rows[r];
      uint32_t       w   = dummy;
      if (k < static_cast<int>(rw >> 16)) {
        const uint32_t ew = graph->edges[(rw & 0xffffU) + k];
        w = (ew >> 16) | ((ew & 0xffffU) << 16);
      }
      s_edges[i] = w;
    }
  }
  if (tid == 0) {
    s_red[30] = 0; /* block_hard_decision's flag */
  }
  if constexpr (SPLIT_U4 > 0) {
    uint4*       st = reinterpret_cast<uint4*>(smem + lay.c2v);
    const uint4* gs = reinterpret_cast<const uint4*>(crc_tables + lay.split_tab);
#pragma unroll
    for (int u = 0; u < SPLIT_PER; ++u) {
      const int i = tid + u * nthr;
      if (i < SPLIT_U4) {
        st[i] = stv[u];
      }
    }
    for (int i = tid + SPLIT_PER * nthr; i < SPLIT_U4; i += nthr) { /* narrower workgroups only */
      st[i] = gs[i];
    }
  }
  if (vec16) {
    uint4* s4 = reinterpret_cast<uint4*>(s_soft);
    while (true) {
#pragma unroll
      for (int u = 0; u < PRO_U; ++u) {
        const int i = base4 + tid + u * nthr;
        if (i >= t4) {
          continue;
        }
        uint4 v = pv[u];
        if (i >= z4 && i < z4 + l4) {
          const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 3; q >= 0; --q) {
            if (wv[q] != 0) {
              const int hi = 31 - __builtin_clz(wv[q]); /* highest set bit -> byte index */
              last_local   = max(last_local, (i - z4) * 16 + q * 4 + hi / 8 + 1);
              break;
            }
          }
          v = make_uint4(clamp_inf4(v.x), clamp_inf4(v.y), clamp_inf4(v.z), clamp_inf4(v.w));
        }
        s4[i] = v;
      }
      base4 += PRO_U * nthr;
      if (base4 >= t4) {
        break;
      }
#pragma unroll
      for (int u = 0; u < PRO_U; ++u) { /* the next pass's loads (blocks narrower than t4 / PRO_U threads) */
        const int i = base4 + tid + u * nthr;
        pv[u]       = (i >= z4 && i < z4 + l4 && i < t4) ? g4[i - z4] : make_uint4(0, 0, 0, 0);
      }
    }
  } else if ((reinterpret_cast<uintptr_t>(llr) & 15U) == 0) {
    /* 16-byte loads whatever the alignment of 2Z and L (Z % 8 != 0, e.g. BG2 Z=36, or shortened lengths): the chunks
     * land at soft + 2Z + 16 k through 4-byte (Z even) or 2-byte LDS writes, the last L % 16 LLRs by byte loads, and
     * a thread issues all its loads of a pass (and the tail's) before storing any. A loop of byte loads instead paid
     * one memory round trip per trip (BG2 Z=36, 128 threads: 15 trips, a 22 us prologue from pinned host memory). */
    const int lc = L >> 4, lt = L & 15;
    int8_t    tv = 0;
    if (tid < lt) {
      tv = llr[16 * lc + tid];
    }
    for (int i = tid; i < 2 * Z; i += nthr) {
      s_soft[i] = 0;
    }
    for (int i = 2 * Z + L + tid; i < total; i += nthr) {
      s_soft[i] = 0;
    }
    for (int c0 = 0; c0 < lc; c0 += PRO_U * nthr) {
      uint4 w[PRO_U];
#pragma unroll
      for (int u = 0; u < PRO_U; ++u) {
        const int k = c0 + tid + u * nthr;
        w[u]        = k < lc ? g4[k] : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < PRO_U; ++u) {
        const int k = c0 + tid + u * nthr;
        if (k >= lc) {
          continue;
        }
        const uint32_t wv[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
        for (int q = 3; q >= 0; --q) {
          if (wv[q] != 0) {
            const int hi = 31 - __builtin_clz(wv[q]);
            last_local   = max(last_local, k * 16 + q * 4 + hi / 8 + 1);
            break;
          }
        }
        int8_t* dst = s_soft + 2 * Z + 16 * k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t c = clamp_inf4(wv[q]);
          if ((Z & 1) == 0) {
            reinterpret_cast<uint32_t*>(dst)[q] = c;
          } else {
            reinterpret_cast<uint16_t*>(dst)[2 * q]     = static_cast<uint16_t>(c);
            reinterpret_cast<uint16_t*>(dst)[2 * q + 1] = static_cast<uint16_t>(c >> 16);
          }
        }
      }
    }
    if (tid < lt) {
      const int li = 16 * lc + tid;
      if (tv != 0) {
        last_local = max(last_local, li + 1);
      }
      s_soft[2 * Z + li] = static_cast<int8_t>(med3i(tv, -LLR_INTERNAL_INF, LLR_INTERNAL_INF));
    }
  } else {
    for (int i = tid; i < total; i += nthr) {
      int8_t    v  = 0;
      const int li = i - 2 * Z;
      if (li >= 0 && li < L) {
        v = llr[li];
        if (v != 0) {
          last_local = max(last_local, li + 1);
        }
        v = static_cast<int8_t>(med3i(v, -LLR_INTERNAL_INF, LLR_INTERNAL_INF));
      }
      s_soft[i] = v;
    }
  }
  CB_STAMP(7); /* diagnostic build: the soft bits' loads have returned and are stored */
  if (crc_on) {
    uint4* s4 = reinterpret_cast<uint4*>(s_crct);
#pragma unroll
    for (int u = 0; u < CRC_PER; ++u) {
      const int j = tid + u * nthr;
      if (j < CRC_U4) {
        s4[j] = crcv[u];
      }
    }
    for (int j = tid + CRC_PER * nthr; j < CRC_U4; j += nthr) { /* workgroups of fewer than 108 threads */
      s4[j] = crc_chunk(j);
    }
  }
  {
    const int wl = wave_max(last_local);
    if (lane == 0) {
      s_red[wave] = static_cast<uint32_t>(wl);
    }
  }
  __syncthreads();
  CB_STAMP(1);
  /* lane i reads wave i's maximum (one LDS read per lane), then a wave maximum: uniform */
  const int last = wave_max(lane < (nthr + 63) / 64 ? static_cast<int>(s_red[lane]) : 0);
  const int nb   = (KZ + 7) / 8;
  const int Lsig = KZ - static_cast<int>(d.nof_filler_bits);

  int  has_value  = 0;
  int  iterations = d.max_iterations;
  bool write_out  = true;

  if (last == 0) {
    /* All-zero LLRs (impl.cpp:86-94): no CRC -> message of ones; with a CRC -> untouched, nullopt. */
    if (d.crc_mode == LDPC_HIP_CRC_MODE_EARLY_STOP) {
      write_out = false;
    } else {
      for (int b = tid; b < nb; b += nthr) {
        const int nbits = min(8, KZ - 8 * b);
        s_hb[b]         = static_cast<uint8_t>((0xff00U >> nbits) & 0xffU);
      }
      __syncthreads();
      if (d.crc_mode == LDPC_HIP_CRC_MODE_CHECK_AFTER) {
        has_value = (block_crc(s_hb, Lsig, d.crc_poly, s_crct,
                               s_red, crc_tables + CRC_MCOL_OFFSET + d.crc_poly * CRC_MCOL_WORDS) == 0);
      }
    }
  } else {
    /* Codeblock length and number of layers (impl.cpp:103-114). */
    int cb_len = max(last + 2 * Z, (K + 4) * Z);
    cb_len     = ((cb_len + Z - 1) / Z) * Z;
    const int nof_layers = cb_len / Z - K;
    const int half  = lane >> 5;
    const int trash = N_full * Z; /* scratch bytes after the soft bits take the dummy-edge stores */
    /* steps whose first row is a layer beyond nof_layers are skipped; a step's own rows are checked per task */
    int n_steps = 0; /* generic body only */
    if constexpr (!SPEC) {
      n_steps = graph->n_steps;
      for (int s = 0; s < n_steps; ++s) {
        if (graph->step_row0[s] >= nof_layers) {
          n_steps = s;
          break;
        }
      }
    }
    /* This wave's task of step s is the step_task at tasks[s * tw + wave]. It is fetched one step ahead, lane i
     * loading word i (a vector load, so the step barrier does not wait for it), and read out with v_readlane. */
    const int        tw   = SPEC ? 1 : graph_field_task_waves(graph_slot);
    const bool       idle = wave >= tw; /* wider workgroup than the schedule (mixed launch): barriers only */
    const step_task* tk   = tasks + (idle ? 0 : wave); /* this wave's task of step s: tk[s * tw] (scalar loads) */

    bool     hb_current = false;
#ifdef LDPC_HIP_DIAG
    int diag_n = 1;
    if (blockIdx.x == 0 && tid == 0) {
      g_diag[0] = __builtin_amdgcn_s_memtime();
    }
#endif
    step_task nxt = tk[0]; /* fetched one step ahead: the scalar load overlaps the previous step's row update */
    typename SD::cr_t cr; /* specialised kernel: this lane's c2v bytes, all zero = not yet initialised */
    for (auto& q : cr) {
      q = 0;
    }
    sp::lanes sl{};
    if constexpr (!QUAD) {
      sl = SD::make_lanes(wave, lane, __builtin_amdgcn_readfirstlane(nof_layers),
                                        lay.c2v + 4U * static_cast<uint32_t>(tid));
    }
    typename SD::pf_t pf = {0, 0, 0, 0, 0};
    if constexpr (SPEC && !QUAD) {
      SD::template load_pf<0>(pf, sl);
      SD::ext_init(cr, sl); /* the extension edges kept in registers: their state from the soft bits, once */
    }
    uint32_t qcr[QN]; /* lane-split decoder: this lane's c2v pairs */
    for (auto& q : qcr) {
      q = 0;
    }
    const auto ql = [&] {
      if constexpr (QUAD) {
        return QD::make_lanes(wave, lane, __builtin_amdgcn_readfirstlane(nof_layers));
      } else {
        return 0;
      }
    }();
    /* the iteration loop; with a partial form (few-layer codeblocks: dec::iteration_partial) in two copies, the
     * branch between them taken once per codeblock, outside the loop */
    CB_STAMP(2);
    auto run_iterations = [&](auto partial) __attribute__((always_inline)) {
    for (int it = 0; it < d.max_iterations; ++it) {
      if constexpr (QUAD) {
        QD::iteration(qcr, qtab, ql);
      } else if constexpr (SPEC) {
        if constexpr (decltype(partial)::value) {
          SD::iteration_partial(cr, sl);
        } else {
          SD::iteration(cr, sl, pf);
        }
      }
      for (int g = 0; g < (SPEC ? 0 : n_steps); ++g) {
#ifdef LDPC_HIP_DIAG
        if (blockIdx.x == 0 && lane == 0 && it == d.max_iterations - 1) {
          g_diag2[(g * 16 + wave) * 2] = __builtin_amdgcn_s_memtime();
        }
#endif
        uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        PHASE(7);
        const step_task cur = nxt;
        nxt                 = tk[(g + 1 < n_steps ? g + 1 : 0) * tw];
        const uint32_t  h   = cur.w[0];
        const int      row = static_cast<int>((h >> 8) & 0xffU);
        if ((h & 64U) != 0U && row < nof_layers && !idle) {
          const int deg     = static_cast<int>(h & 31U);
          const int t0      = static_cast<int>(h >> 16);
          int8_t*         c2v_row = s_c2v + cur.w[1];
          const uint32_t* s_slot  = reinterpret_cast<const uint32_t*>(smem + cur.w[2]);
          if ((h & 32U) != 0U) {
            const int t = t0 + (lane & 31);
            if (t < Z) {
              row_dispatch<2, SF08>(deg, t, half, s_slot + (half ? (deg + 1) / 2 : 0), s_soft, c2v_row, sf, Z,
                                   trash, ph);
            }
          } else {
            const int t = t0 + lane;
            if (t < Z) {
              row_dispatch<1, SF08>(deg, t, 0, s_slot, s_soft, c2v_row, sf, Z, trash, ph);
            }
          }
        }
#ifdef LDPC_HIP_DIAG_PHASE
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PHASE(5);
        __syncthreads();
        PHASE(6);
        if (blockIdx.x == 0 && lane == 0 && it == d.max_iterations - 1) {
          for (int q = 0; q < 8; ++q) {
            g_diag2[(g * 16 + wave) * 8 + q] = ph[q];
          }
        }
#endif
#ifdef LDPC_HIP_DIAG
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (blockIdx.x == 0 && lane == 0 && it == d.max_iterations - 1) {
          g_diag2[(g * 16 + wave) * 2 + 1] = __builtin_amdgcn_s_memtime();
        }
#endif
        __syncthreads();
#ifdef LDPC_HIP_DIAG
        if (blockIdx.x == 0 && tid == 0 && diag_n < 4000) {
          g_diag[diag_n++] = __builtin_amdgcn_s_memtime();
        }
#endif
      }
      hb_current = false;
      if (d.crc_mode == LDPC_HIP_CRC_MODE_EARLY_STOP) {
        const bool ok =
            block_hard_decision<SPEC ? SG::g.Z : 0>(s_soft, s_hb, KZ, &s_red[30], static_cast<uint32_t>(it) + 1U, Z,
                                                    SPEC ? static_cast<int>(lay.soft_stride) : 0,
                                                    static_cast<int>(lay.soft_read));
        hb_current    = true;
        if (ok && block_crc(s_hb, Lsig, d.crc_poly, s_crct,
                            s_red, crc_tables + CRC_MCOL_OFFSET + d.crc_poly * CRC_MCOL_WORDS) == 0) {
          has_value  = 1;
          iterations = it + 1;
          break;
        }
      }
    }
    };
    if constexpr (SPEC && !QUAD && SD::HAS_PARTIAL) {
      if (__builtin_expect(nof_layers <= SD::PARTIAL_LAYERS, 0)) {
        run_iterations(std::true_type{});
      } else {
        run_iterations(std::false_type{});
      }
    } else {
      run_iterations(std::false_type{});
    }
    CB_STAMP(3);
    if (!hb_current) {
      block_hard_decision<SPEC ? SG::g.Z : 0>(s_soft, s_hb, KZ, &s_red[30], 0xffffffffU, Z,
                                              SPEC ? static_cast<int>(lay.soft_stride) : 0,
                                              static_cast<int>(lay.soft_read));
    }
    if (d.crc_mode == LDPC_HIP_CRC_MODE_CHECK_AFTER) {
      has_value = (block_crc(s_hb, Lsig, d.crc_poly, s_crct,
                             s_red, crc_tables + CRC_MCOL_OFFSET + d.crc_poly * CRC_MCOL_WORDS) == 0);
    }
  }

  CB_STAMP(4);
  if (write_out) {
    for (int b = tid; b < nb; b += nthr) {
      out[b] = s_hb[b];
    }
  }
  if (tid == 0 && res_base != nullptr) {
    ldpc_hip_cb_result r;
    r.crc_pass               = static_cast<uint8_t>(has_value);
    r.nof_iterations         = static_cast<uint8_t>(iterations);
    r.status                 = write_out ? LDPC_HIP_STATUS_OUTPUT_WRITTEN : 0;
    res_base[d.result_index] = r;
  }
  CB_STAMP(5);
#undef graph
}

/* threads per workgroup at most: the generic body 16 waves, a specialised one 12 (up to 168 VGPRs) */
template <int SPEC_ID>
constexpr int decode_max_threads()
{
  return SPEC_ID < 0 ? 1024 : 768;
}

template <bool SF08, int SPEC_ID>
__global__ void __launch_bounds__(decode_max_threads<SPEC_ID>())
    ldpc_decode_kernel(const dec_cb* __restrict__ cbs, dec_cb one, int graph_slot, const step_task* __restrict__ tasks,
                       lds_layout lay, const int8_t* llr_base, uint8_t* __restrict__ out_base,
                       ldpc_hip_cb_result* __restrict__ res_base, const uint32_t* __restrict__ crc_tables,
                       const dematch_cb* dm_cbs, dematch_cb dm_one)
{
  /* cbs == nullptr: a one-CB launch whose descriptor came by value in the kernel arguments (no dependent load from
   * the descriptor table before the first LLR load; the HAL's zero-copy tables are in host memory).
   * llr_base is not __restrict__: with the fused dematcher (dm_cbs / dm_one) the workgroup first writes the soft
   * buffer it then reads through llr_base, through the dematch descriptor's pointer. */
  decode_cb<SF08, SPEC_ID>(cbs != nullptr ? cbs[blockIdx.x] : one, graph_slot, tasks, lay, llr_base, out_base, res_base,
                           crc_tables, dm_cbs, dm_one);
}

/* The work-queue kernels: one per specialised graph (its fused dematch + decode body only) and one for dematch-only
 * items, so each has the register allocation of its own body. Round 4 first had one kernel per translation unit that
 * dispatched on it.spec among the unit's 4-10 bodies: the union spilled 24-137 VGPRs to scratch and 189-518 SGPRs
 * (the launched kernels of the same bodies spill none), and its bodies ran up to 1.5x slower than launched ones. */
template <int SPEC_ID>
__global__ void __launch_bounds__(decode_max_threads<SPEC_ID>()) ldpc_dwq_decode_kernel(dwq_args a)
{
  dwq_loop(a, [&](const dwq_item& it) __attribute__((always_inline)) {
    decode_cb<true, SPEC_ID>(it.cb, 0, nullptr, it.lay, it.llr_base, it.out_base, it.res_base, it.crc_tables, nullptr,
                             dm_plain(it.dm));
  });
}


/* dwq_kernel_<unit>(id): the work-queue kernel of specialised graph id of the unit's list, nullptr for other ids */
#define LDPC_DWQ_KERNEL_CASE(id, bg, z, ils)                                                                           \
  case id: return reinterpret_cast<const void*>(&ldpc_dwq_decode_kernel<id>);
#define LDPC_DWQ_KERNELS(NAME, LIST)                                                                                   \
  const void* NAME(int id)                                                                                             \
  {                                                                                                                    \
    switch (id) {                                                                                                      \
      LIST(LDPC_DWQ_KERNEL_CASE)                                                                                       \
    default: return nullptr;                                                                                           \
    }                                                                                                                  \
  }

/* The split-row address table of specialised graph SPEC_ID into dst (dec::write_split_table), or for a one-wave graph
 * its lane-split decoder's address table (qdec::write_table): one workgroup of the decoder's width, launched once per
 * context (ldpc_hip_kernels.hip write_split_tables). */
template <int SPEC_ID>
__global__ void __launch_bounds__(768) ldpc_split_table_kernel(uint32_t* __restrict__ dst)
{
  using SG = spec::spec_graph<SPEC_ID>;
  using SD = sp::dec<SG::g>;
  if constexpr (spec::is_quad(SG::g)) { /* the lane-split decoder's address table (sp::qdec) */
    sp::qdec<SG::g, SG::q>::write_table(dst, static_cast<int>(threadIdx.x >> 6), static_cast<int>(threadIdx.x & 63),
                                        std::make_integer_sequence<int, SG::q.n_steps>{});
  } else if constexpr (SD::LDS_PAIRS > 0) {
    SD::write_split_table(dst, static_cast<int>(threadIdx.x >> 6), static_cast<int>(threadIdx.x & 63));
  }
}


} // namespace ldpc_hip
