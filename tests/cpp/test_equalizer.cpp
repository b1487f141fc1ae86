/*
 * The channel equalizer through the srsRAN-side classes: equalizers made by create_channel_equalizer_factory_hip
 * equalise random cbf16 REs of all ten topologies (zero, denormal-norm, infinite and NaN estimates and one bad port
 * variance among them), and the result is compared bit for bit with the scalar rule computed here in float32
 * (built with -ffp-contract=off): equalize_zf_1xn.h:136-178, equalize_mmse_1xn.h:56-96, equalize_zf_2xn.h:58-63,
 * 182-252, a complex product being (ac - bd, ad + bc).
 */
#include "ldpc_hip_adapters.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace srsran;

static int failures = 0;
#define CHECK(cond, ...)                                                                                             \
  do {                                                                                                               \
    if (!(cond)) {                                                                                                   \
      ++failures;                                                                                                    \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                               \
      std::printf(__VA_ARGS__);                                                                                      \
      std::printf("\n");                                                                                             \
    }                                                                                                                \
  } while (0)

struct cpx {
  float re, im;
};
static cpx   mul(cpx a, cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
static cpx   conj(cpx a) { return {a.re, -a.im}; }
static float norm(cpx a) { return a.re * a.re + a.im * a.im; }
static cpx   cf(cbf16_t v) { return {to_float(v.real), to_float(v.imag)}; }

static uint32_t bits(float f)
{
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint32_t draw()
{
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return static_cast<uint32_t>(rng_state >> 33);
}
static bf16_t pattern(unsigned e_lo, unsigned e_hi)
{
  const uint32_t d = draw();
  return bf16_t{static_cast<uint16_t>((d & 0x8000U) | ((e_lo + (d >> 16) % (e_hi - e_lo)) << 7) | (d & 0x7fU))};
}

static void expect(channel_equalizer_algorithm_type type, unsigned n, unsigned P, unsigned L,
                   const std::vector<cbf16_t>& y, const std::vector<cbf16_t>& h, const std::vector<float>& nv, float ts,
                   std::vector<cpx>& sym, std::vector<float>& var)
{
  const float inf = std::numeric_limits<float>::infinity();
  sym.assign(n * L, cpx{0.0F, 0.0F});
  var.assign(n * L, inf);
  if (L == 1) {
    for (unsigned i = 0; i != n; ++i) {
      float ch_mod_sq = 0.0F, nvar_acc = 0.0F;
      cpx   re_out{0.0F, 0.0F};
      for (unsigned p = 0; p != P; ++p) {
        cpx est = cf(h[p * n + i]);
        if (type == channel_equalizer_algorithm_type::mmse) {
          est = {est.re * ts, est.im * ts};
        }
        const float nrm = norm(est);
        if (std::isnormal(nrm) && std::isnormal(nv[p]) && nv[p] > 0) {
          ch_mod_sq += nrm;
          nvar_acc += nrm * nv[p];
          const cpx m = mul(cf(y[p * n + i]), conj(est));
          re_out      = {re_out.re + m.re, re_out.im + m.im};
        }
      }
      if (type == channel_equalizer_algorithm_type::mmse) {
        if (std::isnormal(ch_mod_sq) && std::isnormal(nvar_acc)) {
          const float rcp = 1.0F / (ch_mod_sq * ch_mod_sq + nvar_acc);
          sym[i]          = {re_out.re * ch_mod_sq * rcp, re_out.im * ch_mod_sq * rcp};
          var[i]          = nvar_acc * rcp;
        }
      } else {
        const float d_pinv = ts * ch_mod_sq;
        if (std::isnormal(d_pinv) && std::isnormal(nvar_acc)) {
          const float rcp = 1.0F / d_pinv;
          sym[i]          = {re_out.re * rcp, re_out.im * rcp};
          var[i]          = nvar_acc * rcp * rcp;
        }
      }
    }
    return;
  }
  float noise_var = nv[0];
  for (unsigned p = 1; p != P; ++p) {
    if (noise_var < nv[p]) {
      noise_var = nv[p];
    }
  }
  if (!std::isnormal(noise_var) || noise_var < 0.0F) {
    return;
  }
  for (unsigned i = 0; i != n; ++i) {
    float n_sq[2];
    cpx   matched[2], xi{0.0F, 0.0F};
    for (unsigned l = 0; l != 2; ++l) {
      float s = 0.0F;
      for (unsigned p = 0; p != P; ++p) {
        s += norm(cf(h[(l * P + p) * n + i]));
      }
      n_sq[l] = s;
    }
    for (unsigned p = 0; p != P; ++p) {
      const cpx m = mul(conj(cf(h[p * n + i])), cf(h[(P + p) * n + i]));
      xi          = {xi.re + m.re, xi.im + m.im};
    }
    for (unsigned l = 0; l != 2; ++l) {
      matched[l] = {0.0F, 0.0F};
      for (unsigned p = 0; p != P; ++p) {
        const cpx m = mul(conj(cf(h[(l * P + p) * n + i])), cf(y[p * n + i]));
        matched[l]  = {matched[l].re + m.re, matched[l].im + m.im};
      }
    }
    const float d_pinv  = ts * ((n_sq[0] * n_sq[1]) - norm(xi));
    const float d_nvars = ts * d_pinv;
    if (std::isnormal(d_pinv)) {
      const float rcp = 1.0F / d_pinv, nrcp = 1.0F / d_nvars;
      const cpx   a = mul(xi, matched[1]), b = mul(conj(xi), matched[0]);
      sym[2 * i]     = {(n_sq[1] * matched[0].re - a.re) * rcp, (n_sq[1] * matched[0].im - a.im) * rcp};
      sym[2 * i + 1] = {(n_sq[0] * matched[1].re - b.re) * rcp, (n_sq[0] * matched[1].im - b.im) * rcp};
      var[2 * i]     = noise_var * n_sq[1] * nrcp;
      var[2 * i + 1] = noise_var * n_sq[0] * nrcp;
    }
  }
}

static void run(channel_equalizer& eq, channel_equalizer_algorithm_type type, unsigned n, unsigned P, unsigned L,
                float ts, int bad_port)
{
  static const uint16_t specials[] = {0x0000, 0x8000, 0x1f80, 0x7f80, 0xff80, 0x7fc0};
  dynamic_tensor<2, cbf16_t, channel_equalizer::re_list::dims>     y({n, P});
  dynamic_tensor<3, cbf16_t, channel_equalizer::ch_est_list::dims> h({n, P, L});
  for (cbf16_t& v : y.get_data()) {
    v.real = pattern(120, 131);
    v.imag = pattern(120, 131);
  }
  for (cbf16_t& v : h.get_data()) {
    v.real = pattern(118, 131);
    v.imag = pattern(118, 131);
  }
  for (unsigned i = 0; i < n; i += 9) { /* a special estimate in one plane, or (every third time) in all of them */
    const bf16_t s{specials[draw() % 6]};
    const unsigned plane = draw() % (L * P);
    for (unsigned q = 0; q != L * P; ++q) {
      if (q == plane || i % 27 == 0) {
        h.get_data()[q * n + i].real = s;
        h.get_data()[q * n + i].imag = s;
      }
    }
  }
  std::vector<float> nv(P);
  for (unsigned p = 0; p != P; ++p) {
    nv[p] = static_cast<float>(1 + draw() % 64) / 1024.0F;
  }
  if (bad_port >= 0) {
    nv[bad_port % P] = (bad_port & 1) ? -1.0F : 0.0F;
  }
  std::vector<cbf16_t> yv(y.get_data().begin(), y.get_data().end()), hv(h.get_data().begin(), h.get_data().end());
  std::vector<cpx>     want;
  std::vector<float>   want_var, got_var(n * L, -3.0F);
  std::vector<cf_t>    got(n * L, cf_t(-3.0F, -3.0F));
  expect(type, n, P, L, yv, hv, nv, ts, want, want_var);
  eq.equalize(span<cf_t>(got), span<float>(got_var), y, h, span<const float>(nv), ts);
  unsigned bad = 0, finite = 0;
  for (unsigned k = 0; k != n * L; ++k) {
    bad += bits(got[k].real()) != bits(want[k].re) || bits(got[k].imag()) != bits(want[k].im) ||
           bits(got_var[k]) != bits(want_var[k]);
    finite += std::isfinite(want_var[k]) ? 1 : 0;
  }
  CHECK(bad == 0, "type %d, %u ports, %u layers, %u REs: %u outputs differ", static_cast<int>(type), P, L, n, bad);
  CHECK(bad_port >= 0 || n < 100 || (finite > n * L / 2 && finite < n * L), "%u of %u outputs finite", finite, n * L);
}

int main()
{
  /* the compat conversions the inputs rely on: ties to even, and the shift back */
  CHECK(to_bf16(1.00390625F).value() == 0x3f80 && to_bf16(1.01171875F).value() == 0x3f82, "to_bf16 ties to even");
  CHECK(to_float(bf16_t{0x3fc0}) == 1.5F && to_cbf16(cf_t(1.5F, -2.0F)) == cbf16_t(1.5F, -2.0F), "bf16 round trip");
  const channel_equalizer_algorithm_type zf = channel_equalizer_algorithm_type::zf,
                                         mmse = channel_equalizer_algorithm_type::mmse;
  std::unique_ptr<channel_equalizer> eq_zf   = create_channel_equalizer_factory_hip(zf)->create();
  std::unique_ptr<channel_equalizer> eq_mmse = create_channel_equalizer_factory_hip(mmse)->create();
  const float scalings[] = {1.0F, 0.7071F, 2.5F};
  unsigned    k = 0;
  for (unsigned n : {1U, 131U, 1031U}) {
    for (unsigned P = 1; P <= 4; ++P) {
      run(*eq_zf, zf, n, P, 1, scalings[k++ % 3], -1);
      run(*eq_mmse, mmse, n, P, 1, scalings[k++ % 3], -1);
    }
    run(*eq_zf, zf, n, 2, 2, scalings[k++ % 3], -1);
    run(*eq_zf, zf, n, 4, 2, scalings[k++ % 3], -1);
  }
  for (int bad_port = 0; bad_port != 4; ++bad_port) {
    run(*eq_zf, zf, 67, 3, 1, 1.0F, bad_port);
    run(*eq_mmse, mmse, 67, 2, 1, 2.5F, bad_port);
    run(*eq_zf, zf, 67, 4, 2, 0.7071F, bad_port);
  }
  std::printf(failures == 0 ? "PASS\n" : "FAILED (%d)\n", failures);
  return failures == 0 ? 0 : 1;
}
