/*
 * The channel equalizer's code object (uplink, in front of the soft demodulator; nothing of the decoder, the uplink
 * family or the mapper is compiled here): ldpc_equalize_kernel and its host launcher (ldpc_equalize.h).
 *
 * channel_equalizer_generic_impl.cpp:165-221 dispatches on (algorithm, rx ports, tx layers) to the scalar loops of
 * equalize_zf_1xn.h:136-178, equalize_mmse_1xn.h:56-96 and equalize_zf_2xn.h:58-63, 182-252, and so does the kernel,
 * operand by operand in float32:
 *   1 x N: ch_mod_sq, nvar_acc and re_out accumulate over the ports in ascending order from zero; a port whose squared
 *          norm is not normal, or whose noise variance is not normal or not positive, is skipped. MMSE scales the
 *          estimate by tx_scaling before its norm. ZF: d = tx_scaling ch_mod_sq, r = 1 / d, (re_out r, nvar_acc r r);
 *          MMSE: r = 1 / (ch_mod_sq ch_mod_sq + nvar_acc), (re_out ch_mod_sq r, nvar_acc r). Unless the denominator's
 *          term and nvar_acc are both normal the RE is (0, +inf).
 *   2 x N: the port norms per layer, xi = sum conj(h_p0) h_p1, the matched inputs sum conj(h_pl) y_p, d_pinv =
 *          tx_scaling (n0 n1 - |xi|^2), d_nvars = tx_scaling d_pinv; symbols ((n1 m0 - xi m1) / d_pinv, (n0 m1 -
 *          conj(xi) m0) / d_pinv) as a multiply by 1 / d_pinv, variances noise_var n1 (1 / d_nvars) and noise_var n0
 *          (1 / d_nvars) left to right. noise_var is std::max_element of the port variances (:182); when it is not
 *          normal or negative the whole segment is (0, +inf) (:59). A negative d_pinv is normal and gives negative
 *          variances, as in the reference.
 * A complex product is (ac - bd, ad + bc) in separate multiplies and adds (no contraction in this file), a division
 * the IEEE one, f32 denormals are kept. std::isnormal is the exponent test (neither 0 nor 255); cbf16 to float is
 * bits << 16.
 *
 * A thread owns EQ_RES = 4 consecutive REs: each plane's four elements in one 16-byte load where the plane's address
 * allows (two 8-byte loads at 8-byte alignment, element loads otherwise and in a segment's last, partial group), the
 * 4 L symbols and 4 L variances in 16-byte stores under the same rule. Nothing outside a segment's planes is read and
 * nothing outside its nof_re x layers outputs written. No LDS, no scratch.
 */
#include "ldpc_block_item.h"
#include "ldpc_equalize.h"

#pragma clang fp contract(off)

namespace ldpc_hip {
namespace {

struct eq_cf {
  float re, im;
};

__device__ __forceinline__ eq_cf eq_mul(eq_cf a, eq_cf b)
{
  return eq_cf{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ eq_cf eq_conj(eq_cf a) { return eq_cf{a.re, -a.im}; }
__device__ __forceinline__ float eq_norm(eq_cf a) { return a.re * a.re + a.im * a.im; }
__device__ __forceinline__ eq_cf eq_from_cbf16(uint32_t w)
{
  return eq_cf{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000U)};
}
__device__ __forceinline__ bool eq_isnormal(float x)
{
  const uint32_t e = (__float_as_uint(x) >> 23) & 0xffU;
  return e != 0U && e != 0xffU;
}

/* the n <= EQ_RES elements at p (a thread's group of a plane; its address is 16 bytes times the thread's index past
 * the plane's first element, so the alignment is the plane's) */
__device__ __forceinline__ void eq_load(const uint32_t* __restrict__ p, uint32_t n, uint32_t (&w)[EQ_RES])
{
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (n == EQ_RES && (a & 15U) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else if (n == EQ_RES && (a & 7U) == 0) {
    const uint2 lo = reinterpret_cast<const uint2*>(p)[0], hi = reinterpret_cast<const uint2*>(p)[1];
    w[0] = lo.x, w[1] = lo.y, w[2] = hi.x, w[3] = hi.y;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < EQ_RES; ++k) {
      w[k] = k < n ? p[k] : 0U;
    }
  }
}

/* the first n of v's N floats to o, N a multiple of 4 */
template <int N>
__device__ __forceinline__ void eq_store(float* __restrict__ o, const float (&v)[N], uint32_t n)
{
  static_assert(N % 4 == 0, "whole 16-byte stores");
  const uintptr_t a = reinterpret_cast<uintptr_t>(o);
  if (n == static_cast<uint32_t>(N) && (a & 15U) == 0) {
#pragma unroll
    for (int g = 0; g < N / 4; ++g) {
      reinterpret_cast<float4*>(o)[g] = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
    }
  } else if (n == static_cast<uint32_t>(N) && (a & 7U) == 0) {
#pragma unroll
    for (int g = 0; g < N / 2; ++g) {
      reinterpret_cast<float2*>(o)[g] = make_float2(v[2 * g], v[2 * g + 1]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (static_cast<uint32_t>(k) < n) {
        o[k] = v[k];
      }
    }
  }
}

/* equalize_zf_1xn.h:137-177 / equalize_mmse_1xn.h:57-95 for one RE; ok: bit p set when port p's noise variance is
 * normal and positive */
template <bool MMSE, int P>
__device__ __forceinline__ void eq_1xn(const eq_cf (&y)[P], const eq_cf (&h)[P], const eq_seg& sg, uint32_t ok,
                                       eq_cf& sym, float& nvar)
{
  float ch_mod_sq = 0.0F, nvar_acc = 0.0F;
  eq_cf re_out{0.0F, 0.0F};
#pragma unroll
  for (int p = 0; p < P; ++p) {
    eq_cf est = h[p];
    if constexpr (MMSE) {
      est = eq_cf{est.re * sg.tx_scaling, est.im * sg.tx_scaling};
    }
    const float norm = eq_norm(est);
    if (eq_isnormal(norm) && ((ok >> p) & 1U) != 0U) {
      ch_mod_sq += norm;
      nvar_acc += norm * sg.noise_var[p];
      const eq_cf m = eq_mul(y[p], eq_conj(est));
      re_out.re += m.re;
      re_out.im += m.im;
    }
  }
  sym  = eq_cf{0.0F, 0.0F};
  nvar = __uint_as_float(0x7f800000U);
  if constexpr (MMSE) {
    if (eq_isnormal(ch_mod_sq) && eq_isnormal(nvar_acc)) {
      const float rcp = 1.0F / (ch_mod_sq * ch_mod_sq + nvar_acc);
      sym             = eq_cf{re_out.re * ch_mod_sq * rcp, re_out.im * ch_mod_sq * rcp};
      nvar            = nvar_acc * rcp;
    }
  } else {
    const float d_pinv = sg.tx_scaling * ch_mod_sq;
    if (eq_isnormal(d_pinv) && eq_isnormal(nvar_acc)) {
      const float rcp = 1.0F / d_pinv;
      sym             = eq_cf{re_out.re * rcp, re_out.im * rcp};
      nvar            = nvar_acc * rcp * rcp;
    }
  }
}

/* equalize_zf_2xn.h:183-251 for one RE; h[l][p]; noise_var: the segment's largest port variance, normal and not
 * negative (the caller took the early return otherwise) */
template <int P>
__device__ __forceinline__ void eq_2xn(const eq_cf (&y)[P], const eq_cf (&h)[2][P], float tx_scaling, float noise_var,
                                       eq_cf (&sym)[2], float (&nvar)[2])
{
  float norm_sq[2];
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    float sum = 0.0F;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      sum += eq_norm(h[l][p]);
    }
    norm_sq[l] = sum;
  }
  eq_cf xi{0.0F, 0.0F};
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const eq_cf m = eq_mul(eq_conj(h[0][p]), h[1][p]);
    xi.re += m.re;
    xi.im += m.im;
  }
  const eq_cf xi_conj   = eq_conj(xi);
  const float xi_mod_sq = eq_norm(xi);
  eq_cf       matched[2];
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    matched[l] = eq_cf{0.0F, 0.0F};
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const eq_cf m = eq_mul(eq_conj(h[l][p]), y[p]);
      matched[l].re += m.re;
      matched[l].im += m.im;
    }
  }
  const float d_pinv  = tx_scaling * ((norm_sq[0] * norm_sq[1]) - xi_mod_sq);
  const float d_nvars = tx_scaling * d_pinv;
  sym[0] = sym[1] = eq_cf{0.0F, 0.0F};
  nvar[0] = nvar[1] = __uint_as_float(0x7f800000U);
  if (eq_isnormal(d_pinv)) {
    const float rcp = 1.0F / d_pinv, nrcp = 1.0F / d_nvars;
    const eq_cf a = eq_mul(xi, matched[1]), b = eq_mul(xi_conj, matched[0]);
    sym[0]  = eq_cf{(norm_sq[1] * matched[0].re - a.re) * rcp, (norm_sq[1] * matched[0].im - a.im) * rcp};
    sym[1]  = eq_cf{(norm_sq[0] * matched[1].re - b.re) * rcp, (norm_sq[0] * matched[1].im - b.im) * rcp};
    nvar[0] = noise_var * norm_sq[1] * nrcp;
    nvar[1] = noise_var * norm_sq[0] * nrcp;
  }
}

/* the thread's group of REs, the segment's RE g .. g + EQ_RES - 1 */
template <bool MMSE, int P, int L>
__device__ __forceinline__ void eq_segment(const eq_seg& sg, uint32_t g, const uint32_t* __restrict__ syms,
                                           const uint32_t* __restrict__ ests, float* __restrict__ eq_syms,
                                           float* __restrict__ eq_nvs)
{
  if (g >= sg.nof_re) {
    return;
  }
  const uint32_t n  = min(static_cast<uint32_t>(EQ_RES), sg.nof_re - g);
  float*         os = eq_syms + 2U * (sg.out_offset + static_cast<uint64_t>(L) * g);
  float*         on = eq_nvs + (sg.out_offset + static_cast<uint64_t>(L) * g);
  float          vs[2 * L * EQ_RES], vn[L * EQ_RES];

  /* segment-uniform: the ports that count (1 x N), the variance and the early return (2 x N) */
  uint32_t ok        = 0;
  float    noise_var = sg.noise_var[0];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    ok |= (eq_isnormal(sg.noise_var[p]) && sg.noise_var[p] > 0.0F) ? 1U << p : 0U;
    if (p != 0 && noise_var < sg.noise_var[p]) { /* std::max_element: the first largest, a NaN never replaces */
      noise_var = sg.noise_var[p];
    }
  }
  if (L == 2 && (!eq_isnormal(noise_var) || noise_var < 0.0F)) {
#pragma unroll
    for (int k = 0; k < L * EQ_RES; ++k) {
      vs[2 * k] = vs[2 * k + 1] = 0.0F;
      vn[k]                     = __uint_as_float(0x7f800000U);
    }
    eq_store(os, vs, 2U * L * n);
    eq_store(on, vn, L * n);
    return;
  }

  uint32_t wy[P][EQ_RES], wh[L][P][EQ_RES];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    eq_load(syms + sg.sym_offset + p * sg.sym_stride + g, n, wy[p]);
  }
#pragma unroll
  for (int l = 0; l < L; ++l) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      eq_load(ests + sg.est_offset + static_cast<uint64_t>(l * P + p) * sg.est_stride + g, n, wh[l][p]);
    }
  }
#pragma unroll
  for (int k = 0; k < EQ_RES; ++k) {
    eq_cf y[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      y[p] = eq_from_cbf16(wy[p][k]);
    }
    if constexpr (L == 1) {
      eq_cf h[P];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        h[p] = eq_from_cbf16(wh[0][p][k]);
      }
      eq_cf s;
      eq_1xn<MMSE, P>(y, h, sg, ok, s, vn[k]);
      vs[2 * k]     = s.re;
      vs[2 * k + 1] = s.im;
    } else {
      eq_cf h[2][P];
#pragma unroll
      for (int l = 0; l < 2; ++l) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
          h[l][p] = eq_from_cbf16(wh[l][p][k]);
        }
      }
      eq_cf s[2];
      float v[2];
      eq_2xn<P>(y, h, sg.tx_scaling, noise_var, s, v);
#pragma unroll
      for (int l = 0; l < 2; ++l) { /* the reverted layer mapping: eq[2 i + layer] */
        vs[2 * (2 * k + l)]     = s[l].re;
        vs[2 * (2 * k + l) + 1] = s[l].im;
        vn[2 * k + l]           = v[l];
      }
    }
  }
  eq_store(os, vs, 2U * L * n);
  eq_store(on, vn, L * n);
}

} // namespace

__global__ void __launch_bounds__(EQ_BLOCK)
    ldpc_equalize_kernel(const eq_seg* __restrict__ segs, uint32_t nseg, const uint32_t* __restrict__ syms,
                         const uint32_t* __restrict__ ests, float* __restrict__ eq_syms, float* __restrict__ eq_nvs)
{
  const eq_seg   sg = segs[block_item(segs, nseg)];
  const uint32_t g  = ((blockIdx.x - sg.block0) * EQ_BLOCK + threadIdx.x) * EQ_RES;
  /* block-uniform; the host admits these ten only */
  switch (sg.algorithm * 8U + (sg.nof_tx_layers - 1U) * 4U + (sg.nof_rx_ports - 1U)) {
    case 0: eq_segment<false, 1, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 1: eq_segment<false, 2, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 2: eq_segment<false, 3, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 3: eq_segment<false, 4, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 5: eq_segment<false, 2, 2>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 7: eq_segment<false, 4, 2>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 8: eq_segment<true, 1, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 9: eq_segment<true, 2, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 10: eq_segment<true, 3, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    case 11: eq_segment<true, 4, 1>(sg, g, syms, ests, eq_syms, eq_nvs); break;
    default: break;
  }
}

hipError_t launch_equalize(const eq_seg* d_segs, uint32_t nseg, uint32_t nblocks, const uint16_t* d_ch_symbols,
                           const uint16_t* d_ch_estimates, float* d_eq_symbols, float* d_eq_noise_vars,
                           hipStream_t stream)
{
  if (nblocks == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_equalize_kernel, dim3(nblocks), dim3(EQ_BLOCK), 0, stream, d_segs, nseg,
                     reinterpret_cast<const uint32_t*>(d_ch_symbols), reinterpret_cast<const uint32_t*>(d_ch_estimates),
                     d_eq_symbols, d_eq_noise_vars);
  return hipGetLastError();
}

} // namespace ldpc_hip
