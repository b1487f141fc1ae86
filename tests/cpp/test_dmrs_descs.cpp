/* Host test of the DM-RS generator's translation (csrc/ldpc_hip_descs.h make_dmrs_table, dmrs_c_init): the rows of
 * good tables field by field, the blob's layout, and one rejection per reason. Links the host-only units alone (no HIP
 * runtime); built with AddressSanitizer and UBSan by tests/test_dmrs_host.py. */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ldpc_hip_descs.h"

using namespace ldpc_hip;

static int g_failed = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                      \
      ++g_failed;                                                                                                      \
    }                                                                                                                  \
  } while (0)

static void expect_reason(const char* got, const char* want, int line)
{
  if (got == nullptr || std::strcmp(got, want) != 0) {
    std::printf("FAIL line %d: reason \"%s\", expected \"%s\"\n", line, got != nullptr ? got : "(accepted)", want);
    ++g_failed;
  }
}
#define REASON(got, want) expect_reason(got, want, __LINE__)

static const char* const R_WEIGHT   = "dmrs_pdsch: a weight component is not finite or is 2^64 or more in magnitude";
static const char* const R_TYPE     = "dmrs_pdsch: the DM-RS type is 1 or 2";
static const char* const R_TOPOLOGY = "dmrs_pdsch: unsupported topology (1 <= layers <= ports <= 4)";
static const char* const R_AMP      = "dmrs_pdsch: the amplitude is not finite";
static const char* const R_ID       = "dmrs_pdsch: scrambling_id above 65535";
static const char* const R_NSCID    = "dmrs_pdsch: n_scid above 1";
static const char* const R_NOSYM    = "dmrs_pdsch: an empty symbol mask";
static const char* const R_SYM14    = "dmrs_pdsch: a symbol-mask bit at or above 14";
static const char* const R_WIDTH    = "dmrs_pdsch: 12 nof_rb above the row's width";
static const char* const R_SSTRIDE  = "dmrs_pdsch: a row is wider than its symbol stride";
static const char* const R_PSTRIDE  = "dmrs_pdsch: the DM-RS symbols are wider than the port stride";
static const char* const R_MASK     = "dmrs_pdsch: an RB mask lies outside the masks";
static const char* const R_TAIL     = "dmrs_pdsch: an RB-mask bit beyond nof_rb";
static const char* const R_WREACH   = "dmrs_pdsch: a weight matrix lies outside the weights";
static const char* const R_BELOW    = "dmrs_pdsch: an allocated RB below reference_point_k_rb";

/* a 70-RB grid: RBs 5 to 9 and 66 to 68, two layers on three ports, DM-RS on symbols 2 and 11 */
static ldpc_hip_dmrs_pdsch_desc good_desc()
{
  ldpc_hip_dmrs_pdsch_desc d{};
  d.grid_offset          = 7;
  d.symbol_stride        = 850;
  d.port_stride          = 14 * 850 + 3;
  d.mask_offset          = 1;
  d.weight_offset        = 2;
  d.nof_rb               = 70;
  d.width                = 840;
  d.slot_index           = 9;
  d.scrambling_id        = 513;
  d.reference_point_k_rb = 4;
  d.amplitude            = 1.4125375F;
  d.symbols_mask         = (1U << 2) | (1U << 11);
  d.type                 = 1;
  d.nof_layers           = 2;
  d.nof_ports            = 3;
  d.n_scid               = 1;
  return d;
}

static const std::vector<uint64_t> g_masks   = {~0ULL, 0x1fULL << 5, 0x7ULL << 2, 0};
static std::vector<float>          g_weights = {9, 9, 9, 9, 0.5F, -0.25F, 1, 0, 0, 1, -1, 0, 0.125F, 2, 3, -4, 9, 9};

static const char* make(const ldpc_hip_dmrs_pdsch_desc& d, dmrs_table& t, const std::vector<float>& w = g_weights,
                        const std::vector<uint64_t>& m = g_masks)
{
  return make_dmrs_table(1, &d, w.data(), static_cast<uint32_t>(w.size() / 2), m.data(),
                         static_cast<uint32_t>(m.size()), t);
}

static void test_c_init()
{
  /* the exact integer modulo 2^31, by 128-bit arithmetic here */
  const uint32_t slots[] = {0, 1, 19, 159}, ids[] = {0, 1, 513, 65535};
  for (uint32_t slot : slots) {
    for (uint32_t l = 0; l != 14; ++l) {
      for (uint32_t id : ids) {
        for (uint32_t n = 0; n != 2; ++n) {
          const unsigned __int128 v =
              static_cast<unsigned __int128>(14U * slot + l + 1U) * (2U * id + 1U) * 131072U + 2U * id + n;
          CHECK(dmrs_c_init(slot, l, id, n) == static_cast<uint32_t>(v % (static_cast<unsigned __int128>(1) << 31)));
        }
      }
    }
  }
  /* the wrap case: the 32-bit product wraps, and wrapping first gives the same */
  const uint32_t wrapped = ((14U * 159U + 13U + 1U) * (2U * 65535U + 1U) * 131072U + (2U * 65535U + 1U)) % 0x80000000U;
  CHECK(dmrs_c_init(159, 13, 65535, 1) == wrapped);
  CHECK(static_cast<uint64_t>(14U * 159U + 14U) * 131071U * 131072U > 0xffffffffULL);
}

static void test_good_tables()
{
  dmrs_table                     t;
  const ldpc_hip_dmrs_pdsch_desc d = good_desc();
  CHECK(make(d, t) == nullptr);
  CHECK(t.rows.size() == 2 && t.nblocks == 2);
  const uint32_t syms[2] = {2, 11};
  for (int i = 0; i != 2; ++i) {
    const dmrs_row&          r  = t.rows[i];
    const ldpc_hip_prs_state st = prs_state_at(dmrs_c_init(9, syms[i], 513, 1), 0);
    CHECK(r.out_offset == 7 + syms[i] * 850ULL && r.out_stride == 14 * 850 + 3);
    CHECK(r.x1 == st.x1 && r.x2 == st.x2);
    CHECK(r.a == static_cast<float>(M_SQRT1_2 * static_cast<double>(1.4125375F)));
    CHECK(r.word0 == 0 && r.weight0 == 2 && r.rb_begin == 5 && r.rb_end == 69 && r.ref_rb == 4);
    CHECK(r.block0 == static_cast<uint32_t>(i) && r.type == 1 && r.nof_layers == 2 && r.nof_ports == 3);
    CHECK(r.bypass == 0 && r.pad == 0);
  }
  /* the blob: rows, the mask's two words, every weight */
  CHECK(t.words_at == 2 * sizeof(dmrs_row) && t.weights_at == t.words_at + 16);
  CHECK(t.blob.size() == t.weights_at + 4 * g_weights.size());
  CHECK(std::memcmp(t.blob.data(), t.rows.data(), t.words_at) == 0);
  CHECK(std::memcmp(t.blob.data() + t.words_at, g_masks.data() + 1, 16) == 0);
  CHECK(std::memcmp(t.blob.data() + t.weights_at, g_weights.data(), 4 * g_weights.size()) == 0);

  /* two transmissions on one mask share its words; type 2; a 275-RB row of several blocks */
  ldpc_hip_dmrs_pdsch_desc two[3] = {d, d, d};
  two[1].type                     = 2;
  two[1].symbols_mask             = 1U << 13;
  two[1].reference_point_k_rb     = 5;
  std::vector<uint64_t> wide(5, 0);
  wide[0] = 1ULL << 3, wide[4] = 1ULL << 18; /* RBs 3 and 274 */
  std::vector<uint64_t> masks = g_masks;
  masks.insert(masks.end(), wide.begin(), wide.end());
  two[2].mask_offset = 4, two[2].nof_rb = 275, two[2].width = 3300, two[2].symbol_stride = 3300;
  two[2].port_stride = 14 * 3300, two[2].reference_point_k_rb = 0, two[2].symbols_mask = 1U << 3;
  CHECK(make_dmrs_table(3, two, g_weights.data(), 9, masks.data(), 9, t) == nullptr);
  CHECK(t.rows.size() == 4 && t.nblocks == 3 + (272 + DMRS_BLOCK * DMRS_RBS - 1) / (DMRS_BLOCK * DMRS_RBS));
  CHECK(t.rows[2].word0 == 0 && t.rows[2].type == 2 && t.rows[2].ref_rb == 5 && t.rows[2].block0 == 2);
  CHECK(t.rows[3].word0 == 2 && t.rows[3].rb_begin == 3 && t.rows[3].rb_end == 275 && t.rows[3].block0 == 3);
  CHECK(t.weights_at - t.words_at == 7 * 8);

  /* an empty RB mask is skipped: no rows, no blob; zero descriptors likewise */
  ldpc_hip_dmrs_pdsch_desc e = d;
  e.mask_offset              = 3;
  e.nof_rb                   = 11;
  CHECK(make(e, t) == nullptr && t.rows.empty() && t.blob.empty() && t.nblocks == 0);
  CHECK(make_dmrs_table(0, nullptr, nullptr, 0, nullptr, 0, t) == nullptr && t.rows.empty());

  /* the bypass: one layer on one port and a weight that compares equal to 1 */
  ldpc_hip_dmrs_pdsch_desc b = d;
  b.nof_layers = b.nof_ports = 1;
  b.weight_offset            = 3; /* (1, 0) */
  CHECK(make(b, t) == nullptr && t.rows[0].bypass == 1 && t.rows[1].bypass == 1);
  std::vector<float> w = g_weights;
  w[7]                 = -0.0F;
  CHECK(make(b, t, w) == nullptr && t.rows[0].bypass == 1);
  b.weight_offset = 4; /* (0, 1) */
  CHECK(make(b, t) == nullptr && t.rows[0].bypass == 0);
  b.weight_offset = 3, b.nof_ports = 2; /* (1, 0) on two ports */
  CHECK(make(b, t) == nullptr && t.rows[0].bypass == 0);
  /* amplitude -0: a = -0 */
  b.amplitude = -0.0F;
  CHECK(make(b, t) == nullptr && std::signbit(t.rows[0].a) && t.rows[0].a == 0.0F);
  /* the first RB on the reference point; the last symbol's row ending on the port stride */
  ldpc_hip_dmrs_pdsch_desc edge = d;
  edge.reference_point_k_rb     = 5;
  edge.port_stride              = 11 * 850 + 840;
  edge.symbol_stride            = 850;
  CHECK(make(edge, t) == nullptr);
  edge.scrambling_id = 65535, edge.symbols_mask = 0x3fff;
  CHECK(make(edge, t) != nullptr); /* symbol 13 now past the port stride */
  edge.port_stride = 13 * 850 + 840;
  CHECK(make(edge, t) == nullptr && t.rows.size() == 14);
}

static void test_rejections()
{
  dmrs_table                     t;
  const ldpc_hip_dmrs_pdsch_desc g = good_desc();
  ldpc_hip_dmrs_pdsch_desc       d = g;
  const float                    inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");

  for (uint8_t type : {0, 3, 255}) {
    d = g, d.type = type;
    REASON(make(d, t), R_TYPE);
  }
  const uint8_t bad[][2] = {{0, 1}, {1, 0}, {2, 1}, {3, 2}, {4, 3}, {1, 5}, {5, 5}, {0, 0}};
  for (const auto& lp : bad) {
    d = g, d.nof_layers = lp[0], d.nof_ports = lp[1];
    REASON(make(d, t), R_TOPOLOGY);
  }
  for (float v : {inf, -inf, nan, 18446744073709551616.0F, -18446744073709551616.0F}) {
    for (size_t at : {size_t(0), g_weights.size() - 1, size_t(9)}) { /* anywhere in the array, used or not */
      std::vector<float> w = g_weights;
      w[at]                = v;
      REASON(make(g, t, w), R_WEIGHT);
    }
  }
  std::vector<float> w = g_weights;
  w[9]                 = 18446742974197923840.0F; /* the float below 2^64 */
  CHECK(make(g, t, w) == nullptr);
  for (float v : {inf, -inf, nan}) {
    d = g, d.amplitude = v;
    REASON(make(d, t), R_AMP);
  }
  d = g, d.symbols_mask = 0;
  REASON(make(d, t), R_NOSYM);
  d = g, d.symbols_mask = 1U << 14;
  REASON(make(d, t), R_SYM14);
  d = g, d.symbols_mask = 0x8004;
  REASON(make(d, t), R_SYM14);
  d = g, d.reference_point_k_rb = 6; /* RB 5 is allocated */
  REASON(make(d, t), R_BELOW);
  d = g, d.reference_point_k_rb = 0xffffffffU;
  REASON(make(d, t), R_BELOW);
  d = g, d.width = 839;
  REASON(make(d, t), R_WIDTH);
  d = g, d.nof_rb = 0x20000000U; /* 12 nof_rb would wrap 32 bits */
  REASON(make(d, t), R_WIDTH);
  d = g, d.symbol_stride = 839;
  REASON(make(d, t), R_SSTRIDE);
  d = g, d.port_stride = 11 * 850 + 839; /* symbol 11's row ends one past it */
  REASON(make(d, t), R_PSTRIDE);
  d = g, d.symbol_stride = ~0ULL / 8, d.port_stride = ~0ULL;
  REASON(make(d, t), R_PSTRIDE);
  d = g, d.mask_offset = 3; /* two words from the last */
  REASON(make(d, t), R_MASK);
  d = g, d.mask_offset = 5;
  REASON(make(d, t), R_MASK);
  d = g, d.mask_offset = 0xffffffffU;
  REASON(make(d, t), R_MASK);
  d = g, d.nof_rb = 66, d.width = 840; /* RBs 66 to 68 are set */
  REASON(make(d, t), R_TAIL);
  d = g, d.weight_offset = 4; /* six weights from the fourth of nine */
  REASON(make(d, t), R_WREACH);
  d = g, d.weight_offset = 10;
  REASON(make(d, t), R_WREACH);
  d = g, d.nof_layers = 4, d.nof_ports = 4, d.weight_offset = 0;
  REASON(make(d, t), R_WREACH);
  d = g, d.scrambling_id = 65536;
  REASON(make(d, t), R_ID);
  d = g, d.n_scid = 2;
  REASON(make(d, t), R_NSCID);
  /* the second descriptor's violation is found too, and leaves no table behind */
  ldpc_hip_dmrs_pdsch_desc two[2] = {g, g};
  two[1].type                     = 0;
  REASON(make_dmrs_table(2, two, g_weights.data(), 9, g_masks.data(), 4, t), R_TYPE);
  CHECK(t.blob.empty() && t.nblocks == 0);
}

int main()
{
  CHECK(sizeof(ldpc_hip_dmrs_pdsch_desc) == 64 && sizeof(dmrs_row) == 64);
  for (uint32_t type = 0; type != 4; ++type) {
    for (uint32_t l = 0; l != 6; ++l) {
      for (uint32_t p = 0; p != 6; ++p) {
        CHECK(dmrs_supported(type, l, p) == ((type == 1 || type == 2) && l >= 1 && l <= p && p <= 4));
      }
    }
  }
  test_c_init();
  test_good_tables();
  test_rejections();
  std::printf(g_failed == 0 ? "test_dmrs_descs: all passed\n" : "test_dmrs_descs: %d checks failed\n", g_failed);
  return g_failed == 0 ? 0 : 1;
}
