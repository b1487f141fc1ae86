/*
 * The channel precoder through the srsRAN-side classes: precoders made by create_channel_precoder_factory_hip run
 * apply_layer_map_and_precoding and apply_precoding for all ten topologies (1 <= layers <= ports <= 4), through
 * buffers whose slices are not contiguous, and the result is compared bit for bit with the scalar rule computed here
 * in float32 (built with -ffp-contract=off): channel_precoder_generic.cpp:27-70, the first product assigned, the others
 * added in ascending layer order, a complex product being (ac - bd, ad + bc).
 */
#include "ldpc_hip_adapters.h"

#include <cstdio>
#include <cstring>
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
static cpx mul(cpx a, cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

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

/* slices `pitch` elements apart with a gap after each, so that no two are contiguous */
class gapped_buffer : public re_buffer_reader, public re_buffer_writer
{
public:
  gapped_buffer(unsigned slices, unsigned re) : nslices(slices), nre(re), data((re + 3U) * slices, cf_t(-3.0F, -3.0F)) {}
  unsigned         get_nof_slices() const override { return nslices; }
  unsigned         get_nof_re() const override { return nre; }
  span<cf_t>       get_slice(unsigned i) override { return span<cf_t>(data.data() + i * (nre + 3U), nre); }
  span<const cf_t> get_slice(unsigned i) const override { return span<const cf_t>(data.data() + i * (nre + 3U), nre); }
  bool gaps_intact() const
  {
    for (unsigned i = 0; i != nslices; ++i) {
      for (unsigned g = 0; g != 3; ++g) {
        if (data[i * (nre + 3U) + nre + g] != cf_t(-3.0F, -3.0F)) {
          return false;
        }
      }
    }
    return true;
  }

private:
  unsigned          nslices, nre;
  std::vector<cf_t> data;
};

static unsigned compare(const gapped_buffer& got, const std::vector<cpx>& want, unsigned n, unsigned P)
{
  unsigned bad = 0;
  for (unsigned p = 0; p != P; ++p) {
    for (unsigned r = 0; r != n; ++r) {
      const cf_t g = got.get_slice(p)[r];
      bad += bits(g.real()) != bits(want[p * n + r].re) || bits(g.imag()) != bits(want[p * n + r].im);
    }
  }
  return bad;
}

static void run(const channel_precoder& pc, unsigned n, unsigned L, unsigned P, float scaling, int max_level)
{
  precoding_weight_matrix w(L, P);
  for (unsigned p = 0; p != P; ++p) {
    for (unsigned l = 0; l != L; ++l) {
      const float re = static_cast<float>(static_cast<int>(draw() % 129U) - 64) / 37.0F;
      const float im = static_cast<float>(static_cast<int>(draw() % 129U) - 64) / 37.0F;
      w.set_coefficient(cf_t(re * scaling, im * scaling), l, p);
    }
  }
  /* apply_layer_map_and_precoding: odd levels, RE r's layer l at r L + l */
  std::vector<ci8_t> sym(static_cast<std::size_t>(n) * L);
  for (ci8_t& s : sym) {
    const int m = max_level + 1;
    s = ci8_t(static_cast<int8_t>(2 * static_cast<int>(draw() % m) - (m - 1)),
              static_cast<int8_t>(2 * static_cast<int>(draw() % m) - (m - 1)));
  }
  gapped_buffer in(L, n), out(P, n);
  for (unsigned l = 0; l != L; ++l) {
    for (unsigned r = 0; r != n; ++r) {
      in.get_slice(l)[r] = cf_t(static_cast<float>(static_cast<int>(draw() % 1025U) - 512) / 37.0F,
                                static_cast<float>(static_cast<int>(draw() % 1025U) - 512) / 37.0F);
    }
  }
  std::vector<cpx> want_ci8(static_cast<std::size_t>(n) * P), want_cf(static_cast<std::size_t>(n) * P);
  for (unsigned r = 0; r != n; ++r) {
    for (unsigned p = 0; p != P; ++p) {
      cpx a{}, b{};
      for (unsigned l = 0; l != L; ++l) {
        const cf_t c = w.get_coefficient(l, p);
        const cpx  wc{c.real(), c.imag()};
        const cpx  x{static_cast<float>(sym[r * L + l].real()), static_cast<float>(sym[r * L + l].imag())};
        const cf_t y = static_cast<const gapped_buffer&>(in).get_slice(l)[r];
        const cpx  ma = mul(x, wc), mb = mul(cpx{y.real(), y.imag()}, wc);
        a = l == 0 ? ma : cpx{a.re + ma.re, a.im + ma.im};
        b = l == 0 ? mb : cpx{b.re + mb.re, b.im + mb.im};
      }
      want_ci8[p * n + r] = a;
      want_cf[p * n + r]  = b;
    }
  }
  pc.apply_layer_map_and_precoding(out, span<const ci8_t>(sym), w);
  unsigned bad = compare(out, want_ci8, n, P);
  CHECK(bad == 0 && out.gaps_intact(), "ci8 in, %u layers, %u ports, %u REs: %u outputs differ", L, P, n, bad);
  pc.apply_precoding(out, in, w);
  bad = compare(out, want_cf, n, P);
  CHECK(bad == 0 && out.gaps_intact(), "cf32 in, %u layers, %u ports, %u REs: %u outputs differ", L, P, n, bad);
}

int main()
{
  std::unique_ptr<channel_precoder> pc = create_channel_precoder_factory_hip()->create();
  const float scalings[]   = {0.70710678F, 0.31622776F, 0.15430336F, 0.07669650F};
  const int   max_levels[] = {1, 3, 7, 15};
  unsigned    k            = 0;
  for (unsigned n : {1U, 131U, 1031U}) {
    for (unsigned L = 1; L <= 4; ++L) {
      for (unsigned P = L; P <= 4; ++P, ++k) {
        run(*pc, n, L, P, scalings[k % 4], max_levels[k % 4]);
      }
    }
  }
  /* one layer, zero weight, level -1: the first product is assigned, so the zero is negative */
  {
    precoding_weight_matrix w(1, 1);
    w.set_coefficient(cf_t(0.0F, 0.0F), 0, 0);
    std::vector<ci8_t> sym(1, ci8_t(-1, 1));
    gapped_buffer      out(1, 1);
    pc->apply_layer_map_and_precoding(out, span<const ci8_t>(sym), w);
    const cf_t g = static_cast<const gapped_buffer&>(out).get_slice(0)[0];
    /* (-1 0 - 1 0, -1 0 + 1 0) = (-0 - 0, -0 + 0) = (-0, +0) */
    CHECK(bits(g.real()) == 0x80000000U && bits(g.imag()) == 0U, "a negative zero: %08x %08x", bits(g.real()),
          bits(g.imag()));
  }
  std::printf(failures == 0 ? "PASS\n" : "FAILED (%d)\n", failures);
  return failures == 0 ? 0 : 1;
}
