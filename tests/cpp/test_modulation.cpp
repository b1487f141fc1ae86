/*
 * The modulation mapper through the srsRAN-side classes: a mapper made by create_channel_modulation_factory_hip maps
 * every symbol index of every scheme, span<cf_t> and span<ci8_t>, and the result is compared bit for bit with tables
 * computed here by the rule of modulation_mapper_lut_impl.cpp: s_k = 1 - 2 b_k, Re from the even-index bits and Im
 * from the odd ones in the nested form of TS 38.211 5.1, cf32 = float(level) * scaling in one float32 multiply.
 */
#include "ldpc_hip_adapters.h"

#include <cmath>
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

static int axis(const int* s, int n) /* s_0 (2^(n-1) - s_1 (2^(n-2) - .. s_(n-1))) */
{
  int t = s[n - 1];
  for (int j = n - 2; j >= 0; --j) {
    t = s[j] * ((1 << (n - 1 - j)) - t);
  }
  return t;
}

/* the integer levels of symbol i of the span, whose Qm bits are b[0 .. Qm) */
static void levels(modulation_scheme scheme, const int* b, unsigned i, int& re, int& im)
{
  int s[8];
  for (int k = 0; k < 8; ++k) {
    s[k] = 1 - 2 * b[k];
  }
  if (scheme == modulation_scheme::BPSK || scheme == modulation_scheme::PI_2_BPSK) {
    re = (scheme == modulation_scheme::PI_2_BPSK && (i & 1U) != 0) ? -s[0] : s[0];
    im = s[0];
    return;
  }
  const int n = static_cast<int>(get_bits_per_symbol(scheme)) / 2;
  int       e[4], o[4];
  for (int k = 0; k < n; ++k) {
    e[k] = s[2 * k];
    o[k] = s[2 * k + 1];
  }
  re = axis(e, n);
  im = axis(o, n);
}

static float scaling(modulation_scheme scheme)
{
  switch (scheme) {
    case modulation_scheme::QAM16: return std::sqrt(1.0F / 10.0F);
    case modulation_scheme::QAM64: return std::sqrt(1.0F / 42.0F);
    case modulation_scheme::QAM256: return std::sqrt(1.0F / 170.0F);
    default: return std::sqrt(1.0F / 2.0F);
  }
}

int main()
{
  auto factory = create_channel_modulation_factory_hip(0);
  auto mapper  = factory->create_modulation_mapper();
  CHECK(mapper != nullptr, "the factory makes a modulation mapper");
  const modulation_scheme schemes[] = {modulation_scheme::PI_2_BPSK, modulation_scheme::BPSK, modulation_scheme::QPSK,
                                       modulation_scheme::QAM16,     modulation_scheme::QAM64, modulation_scheme::QAM256};
  for (modulation_scheme scheme : schemes) {
    const unsigned qm = get_bits_per_symbol(scheme);
    /* every index in order; the two BPSKs as bits 0, 0, 1, 1 so that both parities see both bits */
    std::vector<unsigned> idx;
    if (qm == 1) {
      idx = {0, 0, 1, 1};
    } else {
      for (unsigned v = 0; v != (1U << qm); ++v) {
        idx.push_back(v);
      }
    }
    const unsigned       n = static_cast<unsigned>(idx.size());
    std::vector<uint8_t> packed((n * qm + 7) / 8, 0);
    for (unsigned i = 0; i != n; ++i) {
      for (unsigned k = 0; k != qm; ++k) {
        const unsigned bit = (idx[i] >> (qm - 1 - k)) & 1U, p = i * qm + k;
        packed[p / 8] |= static_cast<uint8_t>(bit << (7 - p % 8));
      }
    }
    bit_buffer          bits(span<uint8_t>(packed), n * qm);
    std::vector<cf_t>   sym(n);
    std::vector<ci8_t>  isym(n);
    mapper->modulate(span<cf_t>(sym), bits, scheme);
    const float sc  = mapper->modulate(span<ci8_t>(isym), bits, scheme);
    const float exp = scaling(scheme);
    CHECK(std::memcmp(&sc, &exp, 4) == 0, "scheme %d: returned scaling %a, expected %a", static_cast<int>(scheme), sc,
          exp);
    const float st = modulation_mapper::get_modulation_scaling(scheme);
    CHECK(std::memcmp(&st, &exp, 4) == 0, "scheme %d: get_modulation_scaling %a", static_cast<int>(scheme), st);
    for (unsigned i = 0; i != n; ++i) {
      int b[8] = {0};
      for (unsigned k = 0; k != qm; ++k) {
        b[k] = static_cast<int>((idx[i] >> (qm - 1 - k)) & 1U);
      }
      int re, im;
      levels(scheme, b, i, re, im);
      CHECK(isym[i].real() == re && isym[i].imag() == im, "scheme %d index %u: ci8 (%d, %d), expected (%d, %d)",
            static_cast<int>(scheme), idx[i], isym[i].real(), isym[i].imag(), re, im);
      const float er = static_cast<float>(re) * exp, ei = static_cast<float>(im) * exp;
      const float gr = sym[i].real(), gi = sym[i].imag();
      CHECK(std::memcmp(&gr, &er, 4) == 0 && std::memcmp(&gi, &ei, 4) == 0,
            "scheme %d index %u: cf32 (%a, %a), expected (%a, %a)", static_cast<int>(scheme), idx[i], gr, gi, er, ei);
    }
  }
  if (failures != 0) {
    std::printf("FAILED (%d)\n", failures);
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
