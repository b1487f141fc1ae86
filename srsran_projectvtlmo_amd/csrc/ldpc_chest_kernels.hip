/*
 * The PUSCH DM-RS channel estimator's code object (uplink, ahead of the equalizer; nothing of the decoder, the uplink
 * family, the mapper, the equalizer, the precoder or the PDSCH DM-RS generator is compiled here): ldpc_chest_kernel
 * and its host launcher (ldpc_chest.h).
 *
 * dmrs_pusch_estimator_impl.cpp:71-212 generates layer 0's pilots per DM-RS symbol ((float)M_SQRT1_2, reference point
 * 0, the sequence of ldpc_dmrs_kernels.hip's c_init), copies them to the other layers and negates the odd pilots of an
 * odd layer; port_channel_estimator_average_impl.cpp:215-408, 467-582, 608-720 then works per (rx port, layer) plane.
 * So does one workgroup here, operand by operand (no contraction in this file):
 *   received pilot = the cbf16 grid element of subcarrier 12 n + 2 j + layer / 2, widened exactly;
 *   prod_s = rx_s conj(x_s) as (ac - b(-d), a(-d) + bc); lse = prod_0, lse += prod_s in symbol order, then both
 *   components times 1.0F / ((float)nsym scaling);
 *   EPRE per symbol sum |rx|^2, the CFO dot sum prod_1 conj(prod_0), RSRP sum |filtered|^2, noise per symbol
 *   sum |(filtered (-beta + 0j)) x_s + rx_s|^2; a per-symbol sum S enters as (S / n) n, as average_power(x) x.size();
 *   smoothing `none`: filtered = lse. `filter`: at most 12 virtual pilots per side from a least-squares line through
 *   hypotf and the unwrapped atan2f of the outermost true pilots (std::polar: rho cosf, rho sinf), then every true
 *   pilot's full-overlap sum ((0 + x[m - T/2] y[T-1]) + x[m - T/2 + 1] y[T-2]) + ... of convolution_same (every true
 *   pilot is a full-overlap output, the virtual pilots being at least T/2 per side);
 *   interpolation: out[0 .. offset] = in[0], then per pilot gap jump = (in[k+1] - in[k]) / 2, out[o+1] = out[o] + jump,
 *   out[o+2] = out[o+1] + jump, carried on from the computed value; in[last] after the last pilot;
 *   cf32 to cbf16 as bf16.h:38-55, Re in the low half, to every symbol of the range at the allocated RBs.
 * Everything elementwise is bit-identical to the reference. The sums are a fixed-shape tree (a thread's pilots in index
 * order, then the lanes of a wave, then the waves), so equal on every run, and differ from the reference's sequential
 * sums by the order alone. With `filter` the three library functions above are the device's.
 *
 * The interpolation is one serial float32 recurrence per component: lane c of wave 0 runs component c, the jumps
 * precomputed by all threads into LDS.
 *
 * LDS per workgroup, sized for 275 RBs: the LS sums with 12 slots of margin each side (13,392 B; the jumps reuse them),
 * the filtered pilots (13,200 B; the cbf16 words of the result reuse them), the 12 n_rb interpolated cf32 values
 * (26,400 B), the pilots' sequence bits per DM-RS symbol (2,208 B), the allocated RBs' indices (552 B), the virtual
 * pilots' scratch (192 B) and the waves' partial sums (16 B): 55,960 bytes, 55,968 with the compiler's alignment
 * padding.
 */
#include "ldpc_block_item.h"
#include "ldpc_chest.h"
#include "ldpc_prs_device.h"

#pragma clang fp contract(off)

namespace ldpc_hip {
namespace {

constexpr uint32_t CH_PILOTS = CHEST_DPR * CHEST_MAX_RB;
constexpr uint32_t CH_A      = 0x3f3504f3U; /* (float)M_SQRT1_2 */

struct ch_cf {
  float re, im;
};

/* std::complex<float>'s product without the NaN recovery: (ac - bd, ad + bc) */
__device__ __forceinline__ ch_cf ch_mul(ch_cf a, ch_cf b)
{
  return ch_cf{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ ch_cf ch_conj(ch_cf a) { return ch_cf{a.re, -a.im}; }
/* Re(x conj(x)) */
__device__ __forceinline__ float ch_norm(ch_cf a) { return a.re * a.re - a.im * (-a.im); }

__device__ __forceinline__ uint32_t ch_bf16(float x)
{
  uint32_t u = __float_as_uint(x);
  u += 0x7fffU + ((u >> 16) & 1U);
  return u >> 16;
}

/* the block's sum of v: the lanes of each wave, then the waves in order; every thread gets it */
__device__ __forceinline__ float ch_block_sum(float v, float* red)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v += __shfl_down(v, off, 64);
  }
  if ((threadIdx.x & 63U) == 0U) {
    red[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < CHEST_BLOCK / 64; ++w) {
    r += red[w];
  }
  __syncthreads();
  return r;
}

/* pilot j's value on DM-RS symbol bits `bits` (the RB's 12 sequence bits); flip: both sign bits of an odd layer's odd
 * pilot */
__device__ __forceinline__ ch_cf ch_pilot(uint32_t bits, uint32_t j, uint32_t flip)
{
  return ch_cf{__uint_as_float(CH_A ^ (((bits >> (2U * j)) & 1U) << 31) ^ flip),
               __uint_as_float(CH_A ^ (((bits >> (2U * j + 1U)) & 1U) << 31) ^ flip)};
}

__device__ __forceinline__ ch_cf ch_rx(const uint32_t* __restrict__ grid, uint64_t e)
{
  const uint32_t g = grid[e];
  return ch_cf{__uint_as_float(g << 16), __uint_as_float(g & 0xffff0000U)};
}

/* compute_v_pilots (port_channel_estimator_average_impl.cpp:651-720) of one side, by one lane: base the nv outermost
 * true pilots, out the nv virtual ones, ab / ar nv floats of scratch each */
__device__ void ch_vpilots(float2* out, const float2* base, uint32_t nv, bool start, float* ab, float* ar)
{
  const float width = 3.14159274101257324219F; /* (float)M_PI */
  for (uint32_t i = 0; i != nv; ++i) {
    ab[i] = hypotf(base[i].x, base[i].y);
    ar[i] = atan2f(base[i].y, base[i].x);
  }
  /* unwrap_list (unwrap.cpp:42-61) */
  float k = 0.0F;
  for (uint32_t i = 0; i + 1 != nv; ++i) {
    const float old_a = ar[i], next_a = ar[i + 1];
    ar[i]             = old_a + 2.0F * k * width;
    const float jump  = next_a - old_a;
    if (fabsf(jump) > width) {
      k = k - copysignf(1.0F, jump);
    }
  }
  ar[nv - 1] += 2.0F * k * width;

  const float fnv       = static_cast<float>(nv);
  const float mean_x    = static_cast<float>(nv * (nv - 1U)) / 2.0F / fnv;
  const float norm_x_sq = static_cast<float>((nv - 1U) * nv * (2U * nv - 1U)) / 6.0F;
  const float den       = norm_x_sq - fnv * mean_x * mean_x;
  float       slope[2], icpt[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float* in  = q == 0 ? ab : ar;
    float        sum = 0.0F, dot = 0.0F;
    for (uint32_t i = 0; i != nv; ++i) {
      sum += in[i];
      dot = dot + in[i] * static_cast<float>(i);
    }
    const float mean = sum / fnv;
    dot -= mean_x * mean * fnv;
    dot /= den;
    slope[q] = dot;
    icpt[q]  = mean - dot * mean_x;
  }
  const int v_offset = start ? -static_cast<int>(nv) : static_cast<int>(nv);
  for (uint32_t i = 0; i != nv; ++i) {
    const float iv  = static_cast<float>(static_cast<int>(i) + v_offset);
    const float rho = slope[0] * iv + icpt[0], theta = slope[1] * iv + icpt[1];
    float       s, c;
    sincosf(theta, &s, &c);
    out[i] = make_float2(rho * c, rho * s);
  }
}

} // namespace

template <bool CF32>
__global__ void __launch_bounds__(CHEST_BLOCK)
    ldpc_chest_kernel(const chest_plane* __restrict__ planes, uint32_t nplanes, const uint64_t* __restrict__ words,
                      const float* __restrict__ filters, const uint32_t* __restrict__ grid, void* __restrict__ est,
                      float2* __restrict__ pilots_out, chest_record* __restrict__ results, int ptr16)
{
  __shared__ __attribute__((aligned(16))) float2 s_lse[CH_PILOTS + 2U * CHEST_MAX_VPILOTS];
  __shared__ __attribute__((aligned(16))) float2 s_filt[CH_PILOTS];
  __shared__ __attribute__((aligned(16))) float2 s_interp[2U * CH_PILOTS];
  __shared__ uint16_t                            s_bits[CHEST_MAX_DMRS][CHEST_MAX_RB + 1U];
  __shared__ uint16_t                            s_rbs[CHEST_MAX_RB + 1U];
  __shared__ float                               s_vp[2][2][CHEST_MAX_VPILOTS];
  __shared__ float                               s_red[CHEST_BLOCK / 64];

  const chest_plane  pl  = planes[block_item(planes, nplanes)];
  const uint32_t     t   = threadIdx.x;
  const uint32_t     nrb = pl.n_rb, np = CHEST_DPR * nrb, nsym = pl.nsym, layer = pl.layer;

  /* the allocated RBs in ascending order: RB n is the (set bits below n)-th */
  for (uint32_t n = pl.rb_begin + t; n < pl.rb_end; n += CHEST_BLOCK) {
    const uint64_t w = words[pl.word0 + n / 64U];
    if (((w >> (n & 63U)) & 1ULL) != 0ULL) {
      uint32_t idx = static_cast<uint32_t>(__popcll(w & ((1ULL << (n & 63U)) - 1ULL)));
      for (uint32_t k = 0; k != n / 64U; ++k) {
        idx += static_cast<uint32_t>(__popcll(words[pl.word0 + k]));
      }
      if (idx < nrb) {
        s_rbs[idx] = static_cast<uint16_t>(n);
      }
    }
  }
  __syncthreads();

  /* an RB's 12 sequence bits once per DM-RS symbol; they end before bit 64 of the word they begin in */
  for (uint32_t r = t; r < nrb; r += CHEST_BLOCK) {
    const uint32_t b0 = 2U * CHEST_DPR * (s_rbs[r] - pl.rb_begin);
#pragma unroll
    for (uint32_t s = 0; s < CHEST_MAX_DMRS; ++s) {
      if (s < nsym) {
        uint32_t x1 = pl.x1[s], x2 = pl.x2[s];
        prs_jump_words(x1, x2, b0 >> 5);
        const uint64_t lo = prs_next_word(x1, x2);
        const uint64_t hi = prs_next_word(x1, x2);
        s_bits[s][r]      = static_cast<uint16_t>(((lo | (hi << 32)) >> (b0 & 31U)) & 0xfffU);
      }
    }
  }
  __syncthreads();

  /* LS sums, EPRE and CFO terms: a thread per pilot */
  float epre[CHEST_MAX_DMRS] = {0.0F, 0.0F, 0.0F, 0.0F};
  float dot_re = 0.0F, dot_im = 0.0F;
  for (uint32_t m = t; m < np; m += CHEST_BLOCK) {
    const uint32_t r = m / CHEST_DPR, j = m - CHEST_DPR * r;
    const uint64_t k    = pl.grid_base + 12ULL * s_rbs[r] + 2U * j + (layer >> 1);
    const uint32_t flip = ((layer & 1U) != 0U && (j & 1U) != 0U) ? 0x80000000U : 0U;
    ch_cf          lse{0.0F, 0.0F}, p0{0.0F, 0.0F};
#pragma unroll
    for (uint32_t s = 0; s < CHEST_MAX_DMRS; ++s) {
      if (s < nsym) {
        const ch_cf rx   = ch_rx(grid, k + pl.dmrs_sym[s] * pl.grid_sym_stride);
        const ch_cf prod = ch_mul(rx, ch_conj(ch_pilot(s_bits[s][r], j, flip)));
        epre[s] += ch_norm(rx);
        if (s == 0) {
          lse = prod;
          p0  = prod;
        } else {
          lse.re += prod.re;
          lse.im += prod.im;
        }
        if (s == 1) {
          const ch_cf d = ch_mul(prod, ch_conj(p0));
          dot_re += d.re;
          dot_im += d.im;
        }
      }
    }
    s_lse[CHEST_MAX_VPILOTS + m] = make_float2(lse.re * pl.total_scaling, lse.im * pl.total_scaling);
  }
  const float fnp      = static_cast<float>(np);
  float       epre_sum = 0.0F;
#pragma unroll
  for (uint32_t s = 0; s < CHEST_MAX_DMRS; ++s) {
    if (s < nsym) { /* block-uniform */
      const float e = ch_block_sum(epre[s], s_red) / fnp * fnp;
      epre_sum      = s == 0 ? e : epre_sum + e;
    }
  }
  dot_re = ch_block_sum(dot_re, s_red);
  dot_im = ch_block_sum(dot_im, s_red); /* its barriers also publish s_lse */

  /* frequency-domain smoothing */
  if (pl.filter == CHEST_NO_FILTER) {
    for (uint32_t m = t; m < np; m += CHEST_BLOCK) {
      s_filt[m] = s_lse[CHEST_MAX_VPILOTS + m];
    }
  } else {
    const uint32_t nv = pl.nvp, T = pl.ntaps;
    if (t == 0U) {
      ch_vpilots(s_lse + CHEST_MAX_VPILOTS - nv, s_lse + CHEST_MAX_VPILOTS, nv, true, s_vp[0][0], s_vp[0][1]);
    } else if (t == 64U) {
      ch_vpilots(s_lse + CHEST_MAX_VPILOTS + np, s_lse + CHEST_MAX_VPILOTS + np - nv, nv, false, s_vp[1][0],
                 s_vp[1][1]);
    }
    __syncthreads();
    const float* y = filters + pl.filter * CHEST_TAP_STRIDE;
    for (uint32_t m = t; m < np; m += CHEST_BLOCK) {
      const float2* x = s_lse + CHEST_MAX_VPILOTS + m - T / 2U;
      float         re = 0.0F, im = 0.0F;
      for (uint32_t i = 0; i != T; ++i) {
        const float c = y[T - 1U - i];
        re += x[i].x * c;
        im += x[i].y * c;
      }
      s_filt[m] = make_float2(re, im);
    }
  }
  __syncthreads();

  /* the filtered pilots out, RSRP and noise terms, the interpolation's jumps (over the LS sums, which are done) */
  float  power = 0.0F;
  float  noise[CHEST_MAX_DMRS] = {0.0F, 0.0F, 0.0F, 0.0F};
  float2* s_jump = s_lse;
  for (uint32_t m = t; m < np; m += CHEST_BLOCK) {
    const uint32_t r = m / CHEST_DPR, j = m - CHEST_DPR * r;
    const uint64_t k    = pl.grid_base + 12ULL * s_rbs[r] + 2U * j + (layer >> 1);
    const uint32_t flip = ((layer & 1U) != 0U && (j & 1U) != 0U) ? 0x80000000U : 0U;
    const float2   f    = s_filt[m];
    if (pilots_out != nullptr) {
      pilots_out[pl.pil_base + m] = f;
    }
    power += ch_norm(ch_cf{f.x, f.y});
    const ch_cf scaled = ch_mul(ch_cf{f.x, f.y}, ch_cf{-pl.beta, 0.0F});
#pragma unroll
    for (uint32_t s = 0; s < CHEST_MAX_DMRS; ++s) {
      if (s < nsym) {
        const ch_cf rx = ch_rx(grid, k + pl.dmrs_sym[s] * pl.grid_sym_stride);
        ch_cf       pr = ch_mul(scaled, ch_pilot(s_bits[s][r], j, flip));
        pr.re += rx.re;
        pr.im += rx.im;
        noise[s] += ch_norm(pr);
      }
    }
    if (m + 1U < np) {
      const float2 g = s_filt[m + 1U];
      s_jump[m]      = make_float2((g.x - f.x) / 2.0F, (g.y - f.y) / 2.0F);
    }
  }
  power           = ch_block_sum(power, s_red);
  float noise_sum = 0.0F;
#pragma unroll
  for (uint32_t s = 0; s < CHEST_MAX_DMRS; ++s) {
    if (s < nsym) {
      const float e = ch_block_sum(noise[s], s_red) / fnp * fnp;
      noise_sum     = s == 0 ? e : noise_sum + e;
    }
  }
  if (t == 0U) {
    chest_record rec{};
    rec.epre_sum   = epre_sum;
    rec.filt_power = power;
    rec.noise_sum  = noise_sum;
    rec.dot_re     = dot_re;
    rec.dot_im     = dot_im;
    rec.nof_pilots = np;
    results[pl.res_index] = rec;
  }

  /* the serial recurrence (interpolator_linear_impl.cpp:32-79 at stride 2): lane c runs component c */
  const uint32_t nre = 2U * np, off = layer >> 1;
  if (t < 2U) {
    const float* in  = reinterpret_cast<const float*>(s_filt) + t;
    const float* jp  = reinterpret_cast<const float*>(s_jump) + t;
    float*       out = reinterpret_cast<float*>(s_interp) + t;
    float        val = in[0];
    for (uint32_t i = 0; i <= off; ++i) {
      out[2U * i] = val;
    }
    uint32_t o = off;
#ifdef LDPC_HIP_EXP_CHEST_NO_RECURRENCE
    /* timing experiment only (make exp, tools/time_chest.py): what the serial chain costs; the estimates are wrong */
    o += 2U * (np - 1U);
#else
#pragma unroll 4
    for (uint32_t k = 0; k + 1U < np; ++k) {
      const float jump = jp[2U * k];
      val += jump;
      out[2U * (o + 1U)] = val;
      val += jump;
      out[2U * (o + 2U)] = val;
      o += 2U;
    }
#endif
    for (uint32_t i = o + 1U; i < nre; ++i) {
      out[2U * i] = in[2U * (np - 1U)];
    }
  }
  __syncthreads();

  /* put: every symbol of the range at the allocated RBs */
  const uint32_t nsymb = pl.nof_symbols;
  if constexpr (!CF32) {
    uint32_t* s_c16 = reinterpret_cast<uint32_t*>(s_filt); /* 12 n_rb words over the 6 n_rb filtered pilots */
    for (uint32_t e = t; e < nre; e += CHEST_BLOCK) {
      s_c16[e] = ch_bf16(s_interp[e].x) | (ch_bf16(s_interp[e].y) << 16);
    }
    __syncthreads();
    uint32_t* o32 = static_cast<uint32_t*>(est);
    if (pl.wide != 0 && ptr16 != 0) {
      const uint32_t per = 3U * nrb; /* quads of a symbol */
      for (uint32_t q = t; q < per * nsymb; q += CHEST_BLOCK) {
        const uint32_t l = q / per, c = q - l * per, r = c / 3U, e = 4U * (c - 3U * r);
        const uint64_t at = pl.est_base + (pl.first_symbol + l) * pl.est_sym_stride + 12ULL * s_rbs[r] + e;
        *reinterpret_cast<uint4*>(o32 + at) = *reinterpret_cast<const uint4*>(s_c16 + 12U * r + e);
      }
    } else {
      for (uint32_t q = t; q < nre * nsymb; q += CHEST_BLOCK) {
        const uint32_t l = q / nre, c = q - l * nre, r = c / 12U, e = c - 12U * r;
        o32[pl.est_base + (pl.first_symbol + l) * pl.est_sym_stride + 12ULL * s_rbs[r] + e] = s_c16[c];
      }
    }
  } else {
    float2* o64 = static_cast<float2*>(est);
    if (pl.wide != 0 && ptr16 != 0) {
      const uint32_t per = 6U * nrb; /* pairs of a symbol */
      for (uint32_t q = t; q < per * nsymb; q += CHEST_BLOCK) {
        const uint32_t l = q / per, c = q - l * per, r = c / 6U, e = 2U * (c - 6U * r);
        const uint64_t at = pl.est_base + (pl.first_symbol + l) * pl.est_sym_stride + 12ULL * s_rbs[r] + e;
        *reinterpret_cast<float4*>(o64 + at) = *reinterpret_cast<const float4*>(s_interp + 12U * r + e);
      }
    } else {
      for (uint32_t q = t; q < nre * nsymb; q += CHEST_BLOCK) {
        const uint32_t l = q / nre, c = q - l * nre, r = c / 12U, e = c - 12U * r;
        o64[pl.est_base + (pl.first_symbol + l) * pl.est_sym_stride + 12ULL * s_rbs[r] + e] = s_interp[c];
      }
    }
  }
}

hipError_t launch_chest(const chest_plane* d_planes, uint32_t nplanes, const uint64_t* d_words, const float* d_filters,
                        const void* d_grid, void* d_est, bool cf32, void* d_pilots, void* d_results,
                        hipStream_t stream)
{
  if (nplanes == 0) {
    return hipSuccess;
  }
  const int ptr16 = (reinterpret_cast<uintptr_t>(d_est) & 15U) == 0U ? 1 : 0;
  if (cf32) {
    hipLaunchKernelGGL((ldpc_chest_kernel<true>), dim3(nplanes), dim3(CHEST_BLOCK), 0, stream, d_planes, nplanes,
                       d_words, d_filters, static_cast<const uint32_t*>(d_grid), d_est, static_cast<float2*>(d_pilots),
                       static_cast<chest_record*>(d_results), ptr16);
  } else {
    hipLaunchKernelGGL((ldpc_chest_kernel<false>), dim3(nplanes), dim3(CHEST_BLOCK), 0, stream, d_planes, nplanes,
                       d_words, d_filters, static_cast<const uint32_t*>(d_grid), d_est, static_cast<float2*>(d_pilots),
                       static_cast<chest_record*>(d_results), ptr16);
  }
  return hipGetLastError();
}

} // namespace ldpc_hip
