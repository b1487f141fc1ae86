/* Host test of the PUSCH DM-RS channel estimator's translation (csrc/ldpc_hip_descs.h make_chest_table, chest_filter,
 * chest_finalize): the planes of a good table field by field, the blob's layout, the filter taps and virtual pilots for
 * 1, 2, 3 and 273 RBs against values computed here from the 31-tap table, the generator states at the first allocated
 * RB, and one rejection per reason. Links the host-only units alone (no HIP runtime); built with AddressSanitizer and
 * UBSan by tests/test_chest_host.py. */
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

static const char* const R_TYPE     = "dmrs_pusch: only DM-RS type 1";
static const char* const R_TOPOLOGY = "dmrs_pusch: unsupported topology (1 to 4 layers on 1 to 4 receive ports)";
static const char* const R_STRATEGY = "dmrs_pusch: the smoothing strategy is LDPC_HIP_CHEST_NONE or LDPC_HIP_CHEST_FILTER";
static const char* const R_CFO      = "dmrs_pusch: CFO compensation is not supported";
static const char* const R_SCALING  = "dmrs_pusch: the scaling is not positive or not finite";
static const char* const R_ID       = "dmrs_pusch: scrambling_id above 65535";
static const char* const R_NSCID    = "dmrs_pusch: n_scid above 1";
static const char* const R_RANGE    = "dmrs_pusch: the symbol range is empty or passes symbol 14";
static const char* const R_NOSYM    = "dmrs_pusch: an empty symbol mask";
static const char* const R_OUTSIDE  = "dmrs_pusch: a DM-RS symbol outside the symbol range";
static const char* const R_FIVE     = "dmrs_pusch: more than 4 DM-RS symbols";
static const char* const R_NRB      = "dmrs_pusch: nof_rb above 275";
static const char* const R_WIDTH    = "dmrs_pusch: 12 nof_rb above the row's width";
static const char* const R_SSTRIDE  = "dmrs_pusch: a row is wider than a symbol stride";
static const char* const R_GSTRIDE  = "dmrs_pusch: the DM-RS symbols are wider than the grid's port stride";
static const char* const R_PSTRIDE  = "dmrs_pusch: the symbol range is wider than the plane stride";
static const char* const R_RXPORT   = "dmrs_pusch: an rx port at or above the grid's ports";
static const char* const R_MASK     = "dmrs_pusch: an RB mask lies outside the masks";
static const char* const R_TAIL     = "dmrs_pusch: an RB-mask bit beyond nof_rb";
static const char* const R_HUGE     = "dmrs_pusch: an offset or stride of 2^48 elements or more";

/* a 70-RB grid of 4 ports: RBs 5 to 9 and 66 to 68, two layers on rx ports {3, 1}, DM-RS on symbols 3 and 11 of the
 * range 2 .. 13 */
static ldpc_hip_dmrs_pusch_desc good_desc()
{
  ldpc_hip_dmrs_pusch_desc d{};
  d.grid_offset        = 7;
  d.grid_symbol_stride = 850;
  d.grid_port_stride   = 14 * 850 + 3;
  d.est_offset         = 8;
  d.symbol_stride      = 844;
  d.plane_stride       = 14 * 844 + 4;
  d.pilots_offset      = 5;
  d.result_offset      = 2;
  d.mask_offset        = 1;
  d.nof_rb             = 70;
  d.width              = 840;
  d.grid_ports         = 4;
  d.slot_index         = 9;
  d.scrambling_id      = 513;
  d.scaling            = 1.4142135F;
  d.symbols_mask       = (1U << 3) | (1U << 11);
  d.type               = 1;
  d.nof_layers         = 2;
  d.nof_rx_ports       = 2;
  d.n_scid             = 1;
  d.first_symbol       = 2;
  d.nof_symbols        = 12;
  d.strategy           = LDPC_HIP_CHEST_FILTER;
  d.rx_ports[0]        = 3;
  d.rx_ports[1]        = 1;
  return d;
}

static const std::vector<uint64_t> g_masks = {~0ULL, 0x1fULL << 5, 0x7ULL << 2, 0};

static const char* make(const ldpc_hip_dmrs_pusch_desc& d, chest_table& t, const std::vector<uint64_t>& m = g_masks)
{
  return make_chest_table(1, &d, m.data(), static_cast<uint32_t>(m.size()), t);
}

/* RC_FILTER of the reference, retyped here: the test's own copy */
static const float RC[31] = {-0.0641253F, -0.0660711F, -0.0611526F, -0.0485918F, -0.0281126F, 0.0000000F,  0.0348830F,
                             0.0751249F,  0.1188406F,  0.1637874F,  0.2075139F,  0.2475302F,  0.2814857F,  0.3073415F,
                             0.3235207F,  0.3290274F,  0.3235207F,  0.3073415F,  0.2814857F,  0.2475302F,  0.2075139F,
                             0.1637874F,  0.1188406F,  0.0751249F,  0.0348830F,  0.0000000F,  -0.0281126F, -0.0485918F,
                             -0.0611526F, -0.0660711F, -0.0641253F};

static void test_filters()
{
  const uint32_t rbs[4] = {1, 2, 3, 273}, taps[4] = {5, 11, 15, 15}, vps[4] = {6, 5, 7, 7};
  for (int c = 0; c != 4; ++c) {
    float y[CHEST_MAX_TAPS];
    for (float& v : y) {
      v = 99.0F;
    }
    CHECK(chest_filter(rbs[c], y) == taps[c]);
    CHECK(chest_virtual_pilots(rbs[c]) == vps[c]);
    /* every second coefficient around the centre, divided by their sequential float32 sum */
    float          total = 0;
    const uint32_t first = 15U - (taps[c] - 1U);
    for (uint32_t i = 0; i != taps[c]; ++i) {
      total += RC[first + 2U * i];
    }
    float sum = 0;
    for (uint32_t i = 0; i != CHEST_MAX_TAPS; ++i) {
      const float want = i < taps[c] ? RC[first + 2U * i] * (1 / total) : 0.0F;
      CHECK(std::memcmp(&y[i], &want, sizeof(float)) == 0);
      sum += y[i];
    }
    CHECK(std::fabs(sum - 1.0F) < 1e-6F);
    CHECK(y[taps[c] / 2U] == RC[15] * (1 / total)); /* the centre tap in the middle: symmetric */
    for (uint32_t i = 0; i != taps[c]; ++i) {
      CHECK(y[i] == y[taps[c] - 1U - i]);
    }
  }
}

static void test_good_table()
{
  chest_table                    t;
  const ldpc_hip_dmrs_pusch_desc d = good_desc();
  CHECK(make(d, t) == nullptr);
  CHECK(t.planes.size() == 4);
  for (uint32_t i = 0; i != 4 && i < t.planes.size(); ++i) {
    const chest_plane& r     = t.planes[i];
    const uint32_t     layer = i / 2, p = i % 2;
    CHECK(r.grid_base == 7 + d.rx_ports[p] * d.grid_port_stride && r.grid_sym_stride == 850);
    CHECK(r.est_base == 8 + i * d.plane_stride && r.est_sym_stride == 844);
    CHECK(r.pil_base == 5 + i * 6ULL * 8 && r.res_index == 2 + i);
    CHECK(r.word0 == 0 && r.rb_begin == 5 && r.rb_end == 69 && r.n_rb == 8);
    CHECK(r.nsym == 2 && r.dmrs_sym[0] == 3 && r.dmrs_sym[1] == 11);
    CHECK(r.layer == layer && r.first_symbol == 2 && r.nof_symbols == 12);
    CHECK(r.filter == 2 && r.ntaps == 15 && r.nvp == 7);
    CHECK(r.beta == d.scaling && r.total_scaling == 1.0F / (2.0F * d.scaling));
    CHECK(r.wide == (r.est_base % 4 == 0 ? 1 : 0));
    CHECK(r.block0 == i);
    /* the generator's state at the first allocated RB's first bit */
    const uint32_t syms[2] = {3, 11};
    for (int s = 0; s != 2; ++s) {
      const ldpc_hip_prs_state st = prs_state_at(dmrs_c_init(9, syms[s], 513, 1), 12ULL * 5);
      CHECK(r.x1[s] == st.x1 && r.x2[s] == st.x2);
      const ldpc_hip_prs_state st0 = prs_state_at(dmrs_c_init(9, syms[s], 513, 1), 0);
      CHECK(r.x2[s] != st0.x2);
    }
  }
  CHECK(t.planes[0].wide == 1 && t.planes[1].wide == 1); /* offsets 8 and 8 + 11820: multiples of 4 */
  /* the blob: planes, the mask's two words, three filters of 16 floats */
  CHECK(t.words_at == 4 * sizeof(chest_plane) && t.filters_at == t.words_at + 2 * 8);
  CHECK(t.blob.size() == t.filters_at + 3 * 16 * 4);
  CHECK(std::memcmp(t.blob.data(), t.planes.data(), t.words_at) == 0);
  CHECK(std::memcmp(t.blob.data() + t.words_at, g_masks.data() + 1, 16) == 0);
  for (uint32_t f = 0; f != 3; ++f) {
    float y[CHEST_MAX_TAPS];
    chest_filter(f + 1, y);
    CHECK(std::memcmp(t.blob.data() + t.filters_at + 64 * f, y, sizeof(y)) == 0);
  }
  /* smoothing none; an odd estimate offset or stride takes the narrow stores; one DM-RS symbol */
  ldpc_hip_dmrs_pusch_desc e = good_desc();
  e.strategy                 = LDPC_HIP_CHEST_NONE;
  e.est_offset               = 9;
  e.symbols_mask             = 1U << 13;
  CHECK(make(e, t) == nullptr && t.planes.size() == 4);
  CHECK(t.planes[0].filter == CHEST_NO_FILTER && t.planes[0].wide == 0 && t.planes[0].nsym == 1);
  CHECK(t.planes[0].total_scaling == 1.0F / (1.0F * e.scaling));
  e            = good_desc();
  e.symbol_stride = 845;
  e.plane_stride  = 14 * 845;
  CHECK(make(e, t) == nullptr && t.planes[0].wide == 0);
  /* one and two allocated RBs pick the short filters */
  e             = good_desc();
  e.mask_offset = 2;
  e.nof_rb      = 64;
  e.width       = 840;
  CHECK(make(e, t) == nullptr && t.planes[0].n_rb == 3 && t.planes[0].filter == 2 && t.planes[0].rb_begin == 2);
  std::vector<uint64_t> m = {1ULL << 40, (1ULL << 3) | (1ULL << 9)};
  e.mask_offset           = 0;
  CHECK(make(e, t, m) == nullptr && t.planes[0].n_rb == 1 && t.planes[0].filter == 0 && t.planes[0].ntaps == 5 &&
        t.planes[0].nvp == 6);
  e.mask_offset = 1;
  CHECK(make(e, t, m) == nullptr && t.planes[0].n_rb == 2 && t.planes[0].filter == 1 && t.planes[0].ntaps == 11 &&
        t.planes[0].nvp == 5);
  /* an empty RB mask is skipped; two transmissions share equal mask words */
  e             = good_desc();
  e.mask_offset = 3;
  e.nof_rb      = 64;
  CHECK(make(e, t) == nullptr && t.planes.empty() && t.blob.empty());
  const ldpc_hip_dmrs_pusch_desc two[2] = {good_desc(), good_desc()};
  CHECK(make_chest_table(2, two, g_masks.data(), 4, t) == nullptr && t.planes.size() == 8);
  CHECK(t.planes[4].word0 == 0 && t.planes[4].block0 == 4 && t.filters_at == t.words_at + 16);
}

static void test_rejections()
{
  chest_table              t;
  ldpc_hip_dmrs_pusch_desc d;
#define BAD(stmt, reason)    \
  d = good_desc();           \
  stmt;                      \
  REASON(make(d, t), reason); \
  CHECK(t.planes.empty() || reason == nullptr)
  BAD(d.type = 2, R_TYPE);
  BAD(d.type = 0, R_TYPE);
  BAD(d.nof_layers = 0, R_TOPOLOGY);
  BAD(d.nof_layers = 5, R_TOPOLOGY);
  BAD(d.nof_rx_ports = 0, R_TOPOLOGY);
  BAD(d.nof_rx_ports = 5, R_TOPOLOGY);
  BAD(d.strategy = 2, R_STRATEGY); /* `mean` and anything else */
  BAD(d.compensate_cfo = 1, R_CFO);
  BAD(d.scaling = 0.0F, R_SCALING);
  BAD(d.scaling = -1.0F, R_SCALING);
  BAD(d.scaling = std::numeric_limits<float>::infinity(), R_SCALING);
  BAD(d.scaling = std::numeric_limits<float>::quiet_NaN(), R_SCALING);
  BAD(d.scrambling_id = 65536, R_ID);
  BAD(d.n_scid = 2, R_NSCID);
  BAD(d.nof_symbols = 0, R_RANGE);
  BAD(d.nof_symbols = 13, R_RANGE);
  BAD(d.symbols_mask = 0, R_NOSYM);
  BAD(d.symbols_mask = (1U << 1) | (1U << 3), R_OUTSIDE);
  BAD(d.symbols_mask = 1U << 14, R_OUTSIDE);
  BAD((d.first_symbol = 2, d.nof_symbols = 9, d.symbols_mask = 1U << 11), R_OUTSIDE);
  BAD(d.symbols_mask = 0x1fU << 3, R_FIVE);
  BAD((d.nof_rb = 276, d.width = 12 * 276, d.grid_symbol_stride = d.symbol_stride = 4000,
       d.grid_port_stride = d.plane_stride = 14 * 4000),
      R_NRB);
  BAD(d.width = 839, R_WIDTH);
  BAD(d.grid_symbol_stride = 839, R_SSTRIDE);
  BAD(d.symbol_stride = 839, R_SSTRIDE);
  BAD(d.grid_port_stride = 11 * 850 + 839, R_GSTRIDE);
  BAD(d.plane_stride = 13 * 844 + 839, R_PSTRIDE);
  BAD(d.rx_ports[1] = 4, R_RXPORT);
  BAD(d.grid_ports = 3, R_RXPORT);
  BAD(d.mask_offset = 3, R_MASK);
  BAD(d.mask_offset = 5, R_MASK);
  BAD((d.mask_offset = 1, d.nof_rb = 68, d.width = 840), R_TAIL);
  /* an offset or stride that could wrap a base: est_offset + plane plane_stride and the like */
  BAD(d.est_offset = 1ULL << 48, R_HUGE);
  BAD(d.grid_offset = ~0ULL - 5, R_HUGE);
  BAD(d.pilots_offset = 1ULL << 63, R_HUGE);
  BAD(d.plane_stride = (1ULL << 62) + 4, R_HUGE);
  BAD(d.grid_port_stride = 1ULL << 62, R_HUGE);
  BAD(d.symbol_stride = 1ULL << 60, R_HUGE);
  BAD(d.grid_symbol_stride = 1ULL << 60, R_HUGE);
#undef BAD
  /* exactly at the limits: accepted */
  d                  = good_desc();
  d.grid_port_stride = 11 * 850 + 840;
  d.plane_stride     = 13 * 844 + 840;
  CHECK(make(d, t) == nullptr && t.planes.size() == 4);
  d            = good_desc();
  d.est_offset = (1ULL << 48) - 4; /* the largest accepted: nothing wraps */
  CHECK(make(d, t) == nullptr && t.planes[3].est_base == d.est_offset + 3 * d.plane_stride);
  d             = good_desc();
  d.rx_ports[3] = 200; /* beyond nof_rx_ports: not looked at */
  CHECK(make(d, t) == nullptr);
}

static void test_finalize()
{
  ldpc_hip_chest_result  r{};
  ldpc_hip_chest_metrics m{};
  r.epre_sum   = 96.0F;
  r.filt_power = 24.0F;
  r.noise_sum  = 5.875F;
  r.dot_re     = 1.0F;
  r.dot_im     = 1.0F;
  r.nof_pilots = 24;
  CHECK(chest_finalize(r, 2.0F, 2, 2, 11, 1, m) == nullptr);
  CHECK(m.epre == 2.0F && m.rsrp == 4.0F && m.noise_var == 0.125F && m.snr == 8.0F && m.has_cfo == 1);
  /* pi / 4 over 2 pi over the nine symbols and their cyclic prefixes between symbols 2 and 11, at 30 kHz */
  const double gap = 9.0 + 9.0 * 72.0 * 64.0 * 30000.0 / (480000.0 * 4096.0);
  CHECK(std::fabs(m.cfo_Hz - 0.125 / gap * 30000.0) < 0.01);
  CHECK(chest_finalize(r, 2.0F, 1, 2, 0, 0, m) == nullptr && m.has_cfo == 0 && m.cfo_Hz == 0.0F);
  /* the floor at rsrp / 10^10, and snr 1000 at a zero noise variance */
  r.noise_sum = 0.0F;
  CHECK(chest_finalize(r, 2.0F, 2, 2, 11, 0, m) == nullptr && m.noise_var == 4.0F / 1e10F && m.snr == 1.0F / m.noise_var);
  r.filt_power = 0.0F;
  r.dot_re = r.dot_im = 0.0F;
  CHECK(chest_finalize(r, 2.0F, 2, 2, 11, 0, m) == nullptr && m.noise_var == 0.0F && m.snr == 1000.0F &&
        m.cfo_Hz == 0.0F && m.has_cfo == 1);
  CHECK(chest_finalize(r, 2.0F, 0, 2, 11, 0, m) != nullptr && chest_finalize(r, 2.0F, 5, 2, 11, 0, m) != nullptr);
  CHECK(chest_finalize(r, 2.0F, 2, 11, 2, 0, m) != nullptr && chest_finalize(r, 2.0F, 2, 2, 14, 0, m) != nullptr);
  CHECK(chest_finalize(r, 0.0F, 2, 2, 11, 0, m) != nullptr && chest_finalize(r, 2.0F, 2, 2, 11, 5, m) != nullptr);
  r.nof_pilots = 0;
  CHECK(chest_finalize(r, 2.0F, 2, 2, 11, 0, m) != nullptr);
}

int main()
{
  CHECK(chest_supported(1, 1, 1, 0, 0) && chest_supported(1, 4, 4, 1, 0) && chest_supported(1, 4, 1, 1, 0));
  CHECK(!chest_supported(2, 1, 1, 0, 0) && !chest_supported(1, 5, 1, 0, 0) && !chest_supported(1, 1, 0, 0, 0));
  CHECK(!chest_supported(1, 1, 1, 2, 0) && !chest_supported(1, 1, 1, 1, 1));
  test_filters();
  test_good_table();
  test_rejections();
  test_finalize();
  if (g_failed != 0) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all passed\n");
  return 0;
}
