/*
 * The downlink code object: the LDPC encoder, the PDSCH encoder (encoder and rate matcher in one workgroup), the rate
 * matcher, the work-queue kernels of the encoder queue and of the HAL's early copy, and their host launchers
 * (ldpc_hip_launch.h). Nothing of the decoder is compiled here.
 */
#include "ldpc_device_util.h"
#include "ldpc_dwq_loop.h"
#include "ldpc_hip_launch.h"

namespace ldpc_hip {

/* This code object's copy of the lifted graphs (the encoder reads rows and edges, slot = (BG - 1) * 51 + lifting
 * position; ldpc_decode_cb.h has the decode object's): upload_graphs fills both. */
static __constant__ graph_desc c_graphs[204];

hipError_t upload_encoder_graphs(const graph_desc* graphs, int n)
{
  return hipMemcpyToSymbol(HIP_SYMBOL(c_graphs), graphs, sizeof(graph_desc) * static_cast<size_t>(n));
}

/* ---- LDPC encoder: ldpc_encoder_impl::encode + ldpc_encoder_generic (ldpc_encoder_impl.cpp:47-81,
 * ldpc_encoder_generic.cpp:32-230), one 256-thread workgroup per codeblock, bit-packed in LDS. SURVEY.md section 8 f2.
 * Every lifted column of Z bits is a run of 32-bit words, LSB first (bit j of a column at word j / 32, bit j % 32). A
 * check row of the base graph with edge (c, s) reads column c rotated by s: 32 of its bits starting at (s + 32 w) mod
 * Z, which is one funnel shift (v_alignbit) of two words of the column's doubled copy (its bits repeated to 2 Z + 64),
 * so a row's 32 check nodes cost two LDS reads and one XOR per edge instead of 32 byte reads (the previous kernel:
 * one byte per bit, 81.5 us for a 128-CB BG1 Z=384 TB, profiles/r04/hal_kernel_trace.txt).
 *   message: K Z bits from the packed (MSB first) source at a bit offset, data_bits of them, zeros after; with crc_at
 *            = S > 0 the CRC24B of bits [0, S) goes to bits [S, S + 24) (TS 38.212 5.2.2: the codeblock CRC of a
 *            segmented TB, which the accelerator attaches in TB mode, hw_accelerator_pdsch_enc.h), computed by the
 *            slicing tables and the x^(32 e) mod G columns of the context's CRC tables (the decoder's block_crc)
 *   preprocess_systematic_bits (generic.cpp:57-101): aux rows 0-3 and the extension parity words from the message
 *   high-rate region (generic.cpp:133-230): the four core parity columns from the aux rows
 *   extension region (generic.cpp:103-120): each extension parity column ^= the row's rotated core parity columns
 *   write_codeblock: codeword bits [2Z, 2Z + cw_length), packed MSB first (bit-reversed words). ---- */
constexpr int ENC_ZW      = MAX_Z / 32;          /* words of one column                           */
constexpr int ENC_ZS      = ENC_ZW + 1;          /* its stride (a funnel shift reads one word on) */
constexpr int ENC_WC      = 2 * ENC_ZW + 2;      /* words of a doubled column                     */
constexpr int ENC_MW      = 22 * MAX_Z / 32 + 2; /* message words                                 */
constexpr int ENC_RAW     = 22 * MAX_Z / 8 + 16; /* message source bytes (bit offset, window)     */

/* 32 bits of the LSB-first bit string v from bit o */
__device__ __forceinline__ uint32_t enc_get32(const uint32_t* v, uint32_t o)
{
  return __builtin_amdgcn_alignbit(v[(o >> 5) + 1], v[o >> 5], o & 31U);
}

/* word q of the doubled copy of a Z-bit column whose bit j is bit base + j of v: bit t = column bit (32 q + t) mod Z */
__device__ __forceinline__ uint32_t enc_dbl(const uint32_t* v, uint32_t base, uint32_t q, uint32_t Z)
{
  if (Z >= 32) { /* at most one wrap in a word */
    const uint32_t o = (32U * q) % Z;
    const uint32_t a = Z - o;
    uint32_t       w = enc_get32(v, base + o);
    if (a < 32) {
      w = (w & ((1U << a) - 1U)) | (enc_get32(v, base) << a);
    }
    return w;
  }
  uint32_t w = 0;
  for (uint32_t t = 0; t != 32; ++t) {
    const uint32_t i = base + (32U * q + t) % Z;
    w |= ((v[i >> 5] >> (i & 31U)) & 1U) << t;
  }
  return w;
}

/* The encoder's LDS state: the codeword's columns, bit-packed. */
constexpr int ENC_OBUF = 4096; /* rate-matched bytes staged per chunk (pdsch_rate_match) */
struct enc_lds {
  uint4    obuf[ENC_OBUF / 16];
  uint8_t  raw[ENC_RAW];
  uint32_t m[ENC_MW];                  /* the message, K Z bits                     */
  uint32_t d[(22 + 5) * ENC_WC];       /* doubled: message columns, p0..p3, aux sum */
  uint32_t a[4 * ENC_ZS];              /* aux rows 0-3                              */
  uint32_t p[4 * ENC_ZS];              /* core parity columns K .. K+3              */
  uint32_t x[(MAX_ROWS - 4) * ENC_ZS]; /* extension parity columns K+4 ..           */
  uint32_t s[ENC_ZS];                  /* aux row sum                               */
  uint32_t rows[MAX_ROWS];
  uint32_t edge[MAX_EDGES];            /* (column << 16) | shift                    */
  uint32_t red[ENC_THREADS / 64];
};

struct enc_geom {
  uint32_t Z, K, NF;
  /* codeword column c's bits: bit j at bit base + j of the returned LSB-first string */
  __device__ __forceinline__ const uint32_t* col(const enc_lds& L, uint32_t c, uint32_t& base) const
  {
    base = 0;
    if (c < K) {
      base = c * Z;
      return L.m;
    }
    return c < K + 4 ? L.p + (c - K) * ENC_ZS : L.x + (c - K - 4) * ENC_ZS;
  }
};

/* Encodes codeblock d into L (every column of the codeword up to the layers d.cw_length needs); block-uniform. */
__device__ __forceinline__ enc_geom enc_build(const enc_cb& d, const uint8_t* __restrict__ msg_base,
                                              const uint32_t* __restrict__ crc_tables, enc_lds& L)
{
  uint8_t*  s_raw  = L.raw;
  uint32_t* s_m    = L.m;
  uint32_t* s_d    = L.d;
  uint32_t* s_a    = L.a;
  uint32_t* s_p    = L.p;
  uint32_t* s_x    = L.x;
  uint32_t* s_s    = L.s;
  uint32_t* s_rows = L.rows;
  uint32_t* s_edge = L.edge;
  uint32_t* s_red  = L.red;

  const graph_desc* gr  = &c_graphs[d.graph_slot];
  const uint32_t    tid = threadIdx.x;
  const uint32_t    Z = gr->Z, K = gr->K, NF = gr->N_full, M = gr->M;
  const uint32_t    ZW = (Z + 31) / 32, WC = 2 * ZW + 2;
  const uint8_t*    msg = msg_base + d.msg_offset;

  /* codeblock length: max(output + 2Z, (K + 4) Z), a multiple of Z (ldpc_encoder_impl.cpp:68-77) */
  uint32_t cb_len = max(d.cw_length + 2 * Z, (K + 4) * Z);
  cb_len          = (cb_len + Z - 1) / Z * Z;
  const uint32_t nof_layers = cb_len / Z - K;

  /* the source bytes (one load per byte, all issued before any is used: the source may be pinned host memory read
   * over PCIe), the graph's rows and edges */
  const uint32_t nbytes = (d.msg_bit_off + d.data_bits + 7) / 8;
  constexpr int  NRAW   = (ENC_RAW + ENC_THREADS - 1) / ENC_THREADS;
  constexpr int  NEDGE  = (MAX_EDGES + ENC_THREADS - 1) / ENC_THREADS;
  static_assert(MAX_ROWS <= ENC_THREADS, "one row word per thread");
  uint32_t raw[NRAW], edge[NEDGE], row = 0;
  /* every load issued before any is stored (a loop of load -> LDS store waited for each over PCIe) */
#pragma unroll
  for (int k = 0; k < NRAW; ++k) {
    const uint32_t i = tid + k * ENC_THREADS;
    raw[k]           = i < nbytes ? msg[i] : 0U;
  }
#pragma unroll
  for (int k = 0; k < NEDGE; ++k) {
    const uint32_t e = tid + k * ENC_THREADS;
    edge[k]          = e < gr->n_edges ? gr->edges[e] : 0U;
  }
  if (tid < M) {
    row = gr->rows[tid];
  }
#pragma unroll
  for (int k = 0; k < NRAW; ++k) {
    const uint32_t i = tid + k * ENC_THREADS;
    if (i < static_cast<uint32_t>(ENC_RAW)) {
      s_raw[i] = static_cast<uint8_t>(raw[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < NEDGE; ++k) {
    const uint32_t e = tid + k * ENC_THREADS;
    if (e < gr->n_edges) {
      s_edge[e] = (((edge[k] & 0xffffU) / Z) << 16) | (edge[k] >> 16);
    }
  }
  if (tid < M) {
    s_rows[tid] = row;
  }
  __syncthreads();
  /* message words: 32 source bits from bit 32 u + msg_bit_off (a 40-bit big-endian window), bit-reversed to LSB first;
   * bits from data_bits on are 0 (a short last segment, the CRC and filler positions) */
  for (uint32_t u = tid; u < static_cast<uint32_t>(ENC_MW); u += ENC_THREADS) {
    uint32_t w = 0;
    if (32 * u < d.data_bits) {
      const uint32_t b = 4 * u;
      const uint64_t x = (static_cast<uint64_t>(s_raw[b]) << 32) | (static_cast<uint64_t>(s_raw[b + 1]) << 24) |
                         (static_cast<uint64_t>(s_raw[b + 2]) << 16) | (static_cast<uint64_t>(s_raw[b + 3]) << 8) |
                         s_raw[b + 4];
      w                 = __builtin_bitreverse32(static_cast<uint32_t>(x >> (8 - d.msg_bit_off)));
      const uint32_t nv = d.data_bits - 32 * u;
      if (nv < 32) {
        w &= (1U << nv) - 1U;
      }
    }
    s_m[u] = w;
  }
  __syncthreads();
  if (d.crc_at != 0) {
    /* CRC24B of bits [0, S): front-padded to nw words (leading zeros do not change a zero-init CRC); word w's CRC by
     * four slicing-table lookups, times x^(32 (nw - 1 - w)) mod G as the XOR of precomputed columns (block_crc) */
    const uint32_t  S    = d.crc_at;
    const uint32_t  nw   = (S + 31) / 32, pad = 32 * nw - S;
    const uint32_t* t0   = crc_tables + LDPC_HIP_CRC24B * CRC_TABLE_SIZE;
    const uint32_t* t1   = crc_tables + CRC_SLICE_OFFSET + LDPC_HIP_CRC24B * CRC_SLICE_WORDS;
    const uint32_t* mcol = crc_tables + CRC_MCOL_OFFSET + LDPC_HIP_CRC24B * CRC_MCOL_WORDS;
    uint32_t        acc  = 0;
    for (uint32_t w = tid; w < nw; w += ENC_THREADS) {
      const uint32_t  v    = (w == 0) ? (s_m[0] << pad) : enc_get32(s_m, 32 * w - pad);
      const uint32_t  W    = __builtin_bitreverse32(v); /* MSB first */
      const uint32_t  crc  = (t1[2 * 256 + (W >> 24)] ^ t1[256 + ((W >> 16) & 0xffU)] ^ t1[(W >> 8) & 0xffU] ^
                            t0[W & 0xffU]) & 0xffffffU;
      const uint32_t* col  = mcol + (nw - 1 - w) * 24;
      uint32_t        prod = 0;
      for (int i = 0; i < 24; ++i) {
        prod ^= col[i] & (0U - ((crc >> i) & 1U));
      }
      acc ^= prod;
    }
    acc = wave_xor(acc);
    if ((tid & 63) == 0) {
      s_red[tid >> 6] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t crc = 0;
      for (int i = 0; i < ENC_THREADS / 64; ++i) {
        crc ^= s_red[i];
      }
      const uint32_t v = __builtin_bitreverse32(crc << 8); /* CRC bit 23 (sent first) at bit 0 */
      const uint32_t s = S & 31U;
      s_m[S >> 5] |= v << s;
      if (s > 8) {
        s_m[(S >> 5) + 1] |= v >> (32 - s);
      }
    }
    __syncthreads();
  }
  /* doubled message columns */
  for (uint32_t i = tid; i < K * WC; i += ENC_THREADS) {
    const uint32_t c = i / WC, q = i - c * WC;
    s_d[c * ENC_WC + q] = enc_dbl(s_m, c * Z, q, Z);
  }
  __syncthreads();
  /* preprocess_systematic_bits: each row's systematic edges */
  for (uint32_t i = tid; i < nof_layers * ZW; i += ENC_THREADS) {
    const uint32_t m = i / ZW, w = i - m * ZW;
    const uint32_t rw = s_rows[m], e0 = rw & 0xffffU, deg = rw >> 16;
    uint32_t       x  = 0;
    for (uint32_t k = 0; k < deg; ++k) {
      const uint32_t ed = s_edge[e0 + k], col = ed >> 16;
      if (col < K) {
        x ^= enc_get32(s_d + col * ENC_WC, (ed & 0xffffU) + 32 * w);
      }
    }
    (m < 4 ? s_a + m * ENC_ZS : s_x + (m - 4) * ENC_ZS)[w] = x;
  }
  __syncthreads();
  /* high-rate region (generic.cpp:133-230): p0 = the aux sum rotated by r, then p1..p3 from the aux rows and p0 or p0
   * rotated by one */
  const bool     bg1     = gr->bg == 1;
  const bool     special = bg1 ? (gr->ils == 6) : (gr->ils == 3 || gr->ils == 7);
  const uint32_t r       = (special && bg1) ? (Z - 105 % Z) % Z : ((!special && !bg1) ? Z - 1 : 0);
  uint32_t*      dsum    = s_d + (K + 4) * ENC_WC;
  for (uint32_t w = tid; w < static_cast<uint32_t>(ENC_ZS); w += ENC_THREADS) {
    s_s[w] = w < ZW ? (s_a[w] ^ s_a[ENC_ZS + w] ^ s_a[2 * ENC_ZS + w] ^ s_a[3 * ENC_ZS + w]) : 0U;
  }
  __syncthreads();
  for (uint32_t q = tid; q < WC; q += ENC_THREADS) {
    dsum[q] = enc_dbl(s_s, 0, q, Z);
  }
  __syncthreads();
  for (uint32_t w = tid; w < static_cast<uint32_t>(ENC_ZS); w += ENC_THREADS) {
    s_p[w] = w < ZW ? enc_get32(dsum, r + 32 * w) : 0U;
  }
  __syncthreads();
  for (uint32_t q = tid; q < WC; q += ENC_THREADS) {
    s_d[K * ENC_WC + q] = enc_dbl(s_p, 0, q, Z);
  }
  __syncthreads();
  for (uint32_t w = tid; w < static_cast<uint32_t>(ENC_ZS); w += ENC_THREADS) {
    uint32_t p1 = 0, p2 = 0, p3 = 0;
    if (w < ZW) {
      const uint32_t a0 = s_a[w], a1 = s_a[ENC_ZS + w], a2 = s_a[2 * ENC_ZS + w], a3 = s_a[3 * ENC_ZS + w];
      const uint32_t p0 = s_p[w], p0r = enc_get32(s_d + K * ENC_WC, 32 * w + 1); /* p0[k], p0[k + 1 mod Z] */
      if (bg1) {
        const uint32_t qv = special ? p0 : p0r;
        p1                = a0 ^ qv;
        p3                = a3 ^ qv;
        p2                = a2 ^ p3;
      } else {
        const uint32_t qv = special ? p0r : p0;
        p1                = a0 ^ qv;
        p2                = a1 ^ p1;
        p3                = a3 ^ qv;
      }
    }
    s_p[ENC_ZS + w]     = p1;
    s_p[2 * ENC_ZS + w] = p2;
    s_p[3 * ENC_ZS + w] = p3;
  }
  __syncthreads();
  for (uint32_t i = tid; i < 3 * WC; i += ENC_THREADS) {
    const uint32_t j = i / WC, q = i - j * WC;
    s_d[(K + 1 + j) * ENC_WC + q] = enc_dbl(s_p + (1 + j) * ENC_ZS, 0, q, Z);
  }
  __syncthreads();
  /* extension region (generic.cpp:103-120): the rows' core parity edges */
  for (uint32_t i = tid; i < (nof_layers - 4) * ZW; i += ENC_THREADS) {
    const uint32_t m = 4 + i / ZW, w = i - (m - 4) * ZW;
    const uint32_t rw = s_rows[m], e0 = rw & 0xffffU, deg = rw >> 16;
    uint32_t       x  = 0;
    for (uint32_t k = 0; k < deg; ++k) {
      const uint32_t ed = s_edge[e0 + k], col = ed >> 16;
      if (col >= K && col < K + 4) {
        x ^= enc_get32(s_d + col * ENC_WC, (ed & 0xffffU) + 32 * w);
      }
    }
    s_x[(m - 4) * ENC_ZS + w] ^= x;
  }
  __syncthreads();
  return enc_geom{Z, K, NF};
}

/* write_codeblock: output bit i = codeword bit 2Z + i, in column (2Z + i) / Z; packed MSB first */
__device__ __forceinline__ void enc_write_codeblock(const enc_cb& d, const enc_lds& L, const enc_geom& g,
                                                    uint8_t* __restrict__ cw)
{
  const uint32_t Z = g.Z, NF = g.NF;
  const uint32_t nb = (d.cw_length + 7) / 8;
  for (uint32_t u = threadIdx.x; u < (d.cw_length + 31) / 32; u += ENC_THREADS) {
    const uint32_t p = 2 * Z + 32 * u;
    uint32_t       w = 0;
    if (Z >= 32) { /* at most two columns in a word */
      const uint32_t  c = p / Z, off = p - c * Z, a = Z - off;
      uint32_t        base;
      const uint32_t* v = g.col(L, c, base);
      w                 = enc_get32(v, base + off);
      if (a < 32) {
        w &= (1U << a) - 1U;
        if (c + 1 < NF) {
          const uint32_t* v2 = g.col(L, c + 1, base);
          w |= enc_get32(v2, base) << a;
        }
      }
    } else {
      for (uint32_t t = 0; t != 32; ++t) {
        const uint32_t c = (p + t) / Z;
        if (c < NF) {
          uint32_t        base;
          const uint32_t* v = g.col(L, c, base);
          const uint32_t  j = base + (p + t - c * Z);
          w |= ((v[j >> 5] >> (j & 31U)) & 1U) << t;
        }
      }
    }
    const uint32_t nv = d.cw_length - 32 * u;
    if (nv < 32) {
      w &= (1U << nv) - 1U;
    }
    const uint32_t y = __builtin_bitreverse32(w); /* MSB first: byte 0 = bits 31..24 */
    for (uint32_t k = 0; k != 4; ++k) {
      if (4 * u + k < nb) {
        cw[4 * u + k] = static_cast<uint8_t>(y >> (24 - 8 * k));
      }
    }
  }
}

__global__ void __launch_bounds__(ENC_THREADS) ldpc_encode_kernel(const enc_cb* __restrict__ cbs,
                                                                  const uint8_t* __restrict__ msg_base,
                                                                  uint8_t* __restrict__ cw_base,
                                                                  const uint32_t* __restrict__ crc_tables)
{
  __shared__ enc_lds L;
  const enc_cb       d = cbs[blockIdx.x];
  const enc_geom     g = enc_build(d, msg_base, crc_tables, L);
  enc_write_codeblock(d, L, g, cw_base + d.cw_offset);
}

/* ldpc_rate_matcher_impl::rate_match of codeblock d (ldpc_rate_match_kernel's arithmetic, below) from the codeword in
 * L: one output bit per thread and round, each wave's 64 bits packed by a ballot */
__device__ __forceinline__ void pdsch_rate_match(const ratematch_cb& d, enc_lds& L, const enc_geom& g,
                                                 uint8_t* __restrict__ out_base)
{
  uint8_t*             out = out_base + d.out_offset;
  const uint32_t       fl = min(d.fill_lo, d.Ncb), fh = min(d.fill_hi, d.Ncb);
  const uint32_t       Ls = d.Ncb - (fh - fl);
  uint32_t             k0 = d.k0;
  if (k0 >= fl && k0 < fh) {
    k0 = fh;
  }
  k0                = (k0 >= d.Ncb) ? 0 : k0;
  const uint32_t r0 = (k0 < fl) ? k0 : k0 - (fh - fl);
  const uint32_t E  = d.rm_length, Qm = d.Qm;
  const uint32_t EQ = E / Qm;
  const uint32_t nb = (E + 7) / 8;
  const uint32_t qs = Qm == 8 ? 3U : (Qm == 4 ? 2U : (Qm == 2 ? 1U : 0U));
  /* x / y for x < 2^21 from a float reciprocal (|error| < 1/2 before the correction); exact division above */
  const bool  fast   = r0 + E < (1U << 21);
  const float inv_ls = 1.0f / static_cast<float>(Ls), inv_z = 1.0f / static_cast<float>(g.Z);
  auto        fdiv   = [](uint32_t x, uint32_t y, float inv) {
    uint32_t  q  = static_cast<uint32_t>(static_cast<float>(x) * inv);
    const int rr = static_cast<int>(x - q * y);
    return rr < 0 ? q - 1 : (rr >= static_cast<int>(y) ? q + 1 : q);
  };
  /* one output bit per thread and round; each wave's 64 bits packed by a ballot, lanes 0-7 put its 8 bytes into LDS;
   * each chunk of ENC_OBUF bytes then leaves in 16-byte stores (the output is often pinned host memory: byte stores
   * went out as one small PCIe write each) */
  const uint32_t lane = threadIdx.x & 63U;
  uint8_t*       ob   = reinterpret_cast<uint8_t*>(L.obuf);
  for (uint32_t c0 = 0; c0 < E; c0 += 8 * ENC_OBUF) {
    const uint32_t cend = min(E, c0 + 8U * ENC_OBUF);
    for (uint32_t o0 = c0; o0 < cend; o0 += ENC_THREADS) {
      const uint32_t o   = o0 + threadIdx.x;
      uint32_t       bit = 0;
      if (o < E) {
        /* interleave_bits: output bit jj Qm + i takes selected bit i EQ + jj */
        const uint32_t  jj = Qm == 6 ? o / 6U : o >> qs;
        const uint32_t  i  = o - jj * Qm;
        const uint32_t  x  = r0 + i * EQ + jj;
        const uint32_t  r  = fast ? x - fdiv(x, Ls, inv_ls) * Ls : x % Ls;
        const uint32_t  p  = ((r < fl) ? r : r + (fh - fl)) + 2 * g.Z; /* codeword bit */
        const uint32_t  cc = fdiv(p, g.Z, inv_z);
        uint32_t        base;
        const uint32_t* src = g.col(L, cc, base);
        const uint32_t  j   = base + (p - cc * g.Z);
        bit                 = (src[j >> 5] >> (j & 31U)) & 1U;
      }
      const uint64_t m  = __ballot(bit != 0U);
      const uint32_t b0 = (o0 + (threadIdx.x & ~63U)) / 8;
      if (lane < 8 && b0 + lane < nb) {
        /* output bit 8 k + t is ballot bit 8 k + t of this wave, sent MSB first */
        ob[b0 + lane - c0 / 8] =
            static_cast<uint8_t>(__builtin_bitreverse32((static_cast<uint32_t>(m >> (8 * lane)) & 0xffU)) >> 24);
      }
    }
    __syncthreads();
    const uint32_t nbc = min(nb - c0 / 8, static_cast<uint32_t>(ENC_OBUF));
    uint8_t*       dst = out + c0 / 8;
    /* a destination off the 16-byte grid leaves in bytes only (n16 = 0). The encoder queue aligns every codeblock's
     * output to 16 bytes and a chunk is 4096 bytes, so that path is not reached through it and no test runs it; a last
     * chunk shorter than 16 bytes also has n16 = 0 and is tested (tests/rm_grid.py, row e_65576) */
    const uint32_t n16 = (reinterpret_cast<uintptr_t>(dst) & 15U) == 0 ? nbc / 16 : 0U;
    for (uint32_t k = threadIdx.x; k < n16; k += ENC_THREADS) {
      reinterpret_cast<uint4*>(dst)[k] = L.obuf[k];
    }
    for (uint32_t k = 16 * n16 + threadIdx.x; k < nbc; k += ENC_THREADS) {
      dst[k] = ob[k];
    }
    __syncthreads();
  }
}

/* The PDSCH encoder queue's batch (ldpc_hip_enc_queue.cpp): encoder and rate matcher in one workgroup per codeblock,
 * the rate matcher reading the codeword's bits from LDS (no codeword buffer, one launch per batch). Descriptors by
 * value for one codeblock (cbs == nullptr), else from the queue's pinned buffer. The rate matcher's arithmetic is
 * ldpc_rate_match_kernel's (below), bit for bit. */
__global__ void __launch_bounds__(ENC_THREADS) ldpc_pdsch_encode_kernel(const pdsch_enc_cb* cbs, pdsch_enc_cb one,
                                                                        const uint8_t* __restrict__ msg_base,
                                                                        uint8_t* __restrict__ out_base,
                                                                        const uint32_t* __restrict__ crc_tables)
{
  __shared__ enc_lds   L;
  const pdsch_enc_cb   c = cbs != nullptr ? cbs[blockIdx.x] : one;
  const enc_geom       g = enc_build(c.enc, msg_base, crc_tables, L);
  pdsch_rate_match(c.rm, L, g, out_base);
}

/* The PDSCH encoder queue's work-queue kernel (ldpc_hip_dwq.h key DWQ_KEY_ENC): a small batch's codeblocks as items of
 * the resident grid, no launch per batch (the payload, dwq_enc_payload, in the item's first words). */
__global__ void __launch_bounds__(ENC_THREADS) ldpc_dwq_encode_kernel(dwq_args a)
{
  __shared__ enc_lds L;
  dwq_loop(a, [&](const dwq_item& it) __attribute__((always_inline)) {
    dwq_enc_payload pl;
    __builtin_memcpy(&pl, &it, sizeof(pl));
    const enc_geom g = enc_build(pl.c.enc, pl.msg_base, pl.crc_tables, L);
    pdsch_rate_match(pl.c.rm, L, g, pl.out_base);
  });
}
const void* dwq_kernel_encode() { return reinterpret_cast<const void*>(&ldpc_dwq_encode_kernel); }

/* The HAL decoder's early copy (ldpc_hip_hal.cpp hal_copy_staged): each item moves one piece of a large batch's staged
 * LLRs from pinned host memory into HBM while the caller is still enqueueing, COPY_UNROLL 16-byte loads per thread in
 * flight before any store (one PCIe round trip per 64 KiB per workgroup), so the batch kernel reads HBM. */
__global__ void __launch_bounds__(COPY_THREADS) ldpc_dwq_copy_kernel(dwq_args a)
{
  dwq_loop(a, [&](const dwq_item& it) __attribute__((always_inline)) {
    dwq_copy_payload pl;
    __builtin_memcpy(&pl, &it, sizeof(pl));
    for (uint64_t k0 = 0; k0 < pl.n16; k0 += COPY_THREADS * COPY_UNROLL) {
      uint4 v[COPY_UNROLL];
#pragma unroll
      for (int u = 0; u < COPY_UNROLL; ++u) {
        const uint64_t k = k0 + static_cast<uint64_t>(u) * COPY_THREADS + threadIdx.x;
        v[u]             = k < pl.n16 ? reinterpret_cast<const uint4*>(pl.src)[k] : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < COPY_UNROLL; ++u) {
        const uint64_t k = k0 + static_cast<uint64_t>(u) * COPY_THREADS + threadIdx.x;
        if (k < pl.n16) {
          reinterpret_cast<uint4*>(pl.dst)[k] = v[u];
        }
      }
    }
  });
}
const void* dwq_kernel_copy() { return reinterpret_cast<const void*>(&ldpc_dwq_copy_kernel); }


/* ---- rate matcher: ldpc_rate_matcher_impl::rate_match (ldpc_rate_matcher_impl.cpp:36-160): bit selection from k0
 * around the circular buffer [0, Ncb) skipping the filler range, then the Qm interleaver. Every output bit is computed
 * independently from its rank in the filler-free circular sequence. ---- */
__global__ void __launch_bounds__(256) ldpc_rate_match_kernel(const ratematch_cb* __restrict__ cbs,
                                                              const uint8_t* __restrict__ cw_base,
                                                              uint8_t* __restrict__ out_base)
{
  const ratematch_cb d  = cbs[blockIdx.x];
  const uint8_t*     cw = cw_base + d.cw_offset;
  uint8_t*           out = out_base + d.out_offset;
  const uint32_t     fl = min(d.fill_lo, d.Ncb), fh = min(d.fill_hi, d.Ncb);
  const uint32_t     L  = d.Ncb - (fh - fl);             /* selectable bits in the circular buffer */
  uint32_t           k0 = d.k0;
  if (k0 >= fl && k0 < fh) {
    k0 = fh;                                              /* select_bits: skip a filler start */
  }
  k0                 = (k0 >= d.Ncb) ? 0 : k0;
  const uint32_t r0  = (k0 < fl) ? k0 : k0 - (fh - fl);   /* rank of the first selected bit */
  const uint32_t EQ  = d.rm_length / d.Qm;
  const uint32_t nb  = (d.rm_length + 7) / 8;
  for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) {
    uint32_t v = 0;
    for (uint32_t q = 0; q < 8; ++q) {
      const uint32_t o = 8 * b + q;
      if (o < d.rm_length) {
        /* interleave_bits (:162-): output bit o = jj * Qm + i takes selected bit i * EQ + jj */
        const uint32_t jj = o / d.Qm, i = o - jj * d.Qm;
        const uint32_t e  = i * EQ + jj;
        const uint32_t r  = (r0 + e) % L;
        const uint32_t p  = (r < fl) ? r : r + (fh - fl);
        v |= ((cw[p >> 3] >> (7 - (p & 7))) & 1U) << (7 - q);
      }
    }
    out[b] = static_cast<uint8_t>(v);
  }
}

hipError_t launch_encode(const enc_cb* d_cbs, uint32_t n, const uint8_t* msg, uint8_t* cw, const uint32_t* d_crc,
                         hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_encode_kernel, dim3(n), dim3(ENC_THREADS), 0, stream, d_cbs, msg, cw, d_crc);
  return hipGetLastError();
}

hipError_t launch_pdsch_encode(const pdsch_enc_cb* d_cbs, const pdsch_enc_cb* host_one, uint32_t n,
                               const uint8_t* msg, uint8_t* out, const uint32_t* d_crc, hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  const bool inl = host_one != nullptr && n == 1;
  hipLaunchKernelGGL(ldpc_pdsch_encode_kernel, dim3(n), dim3(ENC_THREADS), 0, stream, inl ? nullptr : d_cbs,
                     inl ? *host_one : pdsch_enc_cb{}, msg, out, d_crc);
  return hipGetLastError();
}

hipError_t launch_rate_match(const ratematch_cb* d_cbs, uint32_t n, const uint8_t* cw, uint8_t* out,
                             hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_rate_match_kernel, dim3(n), dim3(256), 0, stream, d_cbs, cw, out);
  return hipGetLastError();
}

} // namespace ldpc_hip
