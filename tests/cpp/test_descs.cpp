/* Host test of the descriptor translations (csrc/ldpc_hip_descs.h): every work item field by field for valid
 * descriptors, one rejection per reason, the order of the checks, and the one-CB / plan equivalence. Links the
 * host-only units alone (no HIP runtime); built with AddressSanitizer and UBSan by tests/test_descs_host.py.
 * The expected reasons are the texts of the entry points' errors before the translations were gathered in one unit. */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
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

static const char* const R_DEC_GRAPH  = "invalid base graph / lifting size";
static const char* const R_DEC_ITER   = "Max iterations must be different to 0";
static const char* const R_DEC_LEN    = "input length out of range [(K+2)Z, N_short Z]";
static const char* const R_DEC_FILL   = "invalid number of filler bits";
static const char* const R_DEC_MODE   = "invalid CRC mode";
static const char* const R_DEC_POLY   = "invalid CRC polynomial";
static const char* const R_DEC_SCALE  = "Scaling factor must be between 0 and 1 exclusively";
static const char* const R_DM_PARAMS  = "invalid rv / modulation / rm_length";
static const char* const R_DM_LARGE   = "N_ref / cb_length too large";
static const char* const R_DM_LEN     = "LDPC rate dematching: invalid input length.";
static const char* const R_DM_FILL    = "LDPC rate dematching: invalid number of filler bits.";
static const char* const R_DM_NCB     = "LDPC rate dematching: limited buffer shorter than the systematic bits.";
static const char* const R_DM_PAIRED  = "dematch_decode_launch: dematch descriptor does not match its codeblock "
                                        "(cb_length != llr_length or filler bits differ)";
/* the one wording of what were "demod_dematch_launch: symbols x bits per symbol must equal rm_length",
 * "demod_dematch_launch: rm_length above 32768 (use demodulate + dematch)" and the fused launch's text below */
static const char* const R_DM_DEMOD   = "demod_dematch_launch: symbols x bits per symbol must equal rm_length <= 32768";
static const char* const R_DM_DEMOD_F = "dematch_decode_launch: symbols x bits per symbol must equal rm_length <= 32768";
static const char* const R_DM_SCR     = "scrambled codeblock with rm_length above 32768 cannot be descrambled in the "
                                        "dematcher: descramble it with ldpc_hip_descramble_launch first";

static const char* const R_DEMOD_MOD   = "demodulate: invalid modulation scheme";
static const char* const R_DEMOD_MANY  = "demodulate: too many symbols for one launch";
static const char* const R_PRS_CINIT   = "pseudo-random sequence: c_init above 31 bits";
static const char* const R_PRS_MANY    = "pseudo-random sequence: too many LLRs or bits for one launch";
static const char* const R_MOD_MOD     = "modulate: invalid modulation scheme";
static const char* const R_MOD_CINIT   = "modulate: c_init above 31 bits";
static const char* const R_MOD_SEG     = "modulate: a segment holds fewer than 2^31 symbols";
static const char* const R_MOD_MANY    = "modulate: too many symbols for one launch";
static const char* const R_RMMOD_BPSK  = "rate_match_modulate_launch: pi/2-BPSK is not a PDSCH scheme (a span per "
                                         "codeblock would restart the symbol parity): rate-match, then "
                                         "ldpc_hip_modulate_launch over the codeword";
static const char* const R_RMMOD_PAIR  = "rate_match_modulate_launch: symbols x bits per symbol must equal rm_length, "
                                         "the scheme's bits per symbol modulation_order";
static const char* const R_RM_PARAMS   = "rate_match_launch: invalid parameters";
static const char* const R_EQ_TOPOLOGY = "equalize: unsupported (algorithm, rx ports, tx layers): ZF or MMSE with one "
                                         "layer on 1-4 ports, ZF with two layers on 2 or 4 ports";
static const char* const R_EQ_SCALING  = "equalize: tx_scaling must be positive";
static const char* const R_EQ_STRIDE   = "equalize: a plane stride below nof_re";
static const char* const R_EQ_SEG      = "equalize: a segment holds fewer than 2^31 outputs";
static const char* const R_EQ_MANY     = "equalize: too many REs for one launch";
/* the precoder's, as ldpc_hip_precode.cpp gave them before its translation moved into the descriptor unit */
static const char* const R_PC_WEIGHT   = "precode: a weight component is not finite or is 2^64 or more in magnitude";
static const char* const R_PC_TOPOLOGY = "precode: unsupported topology (1 <= layers <= ports <= 4)";
static const char* const R_PC_PRG      = "precode: prg_size must be at least 1";
static const char* const R_PC_STRIDE   = "precode: a row is wider than its port stride";
static const char* const R_PC_MASK     = "precode: a row's mask lies outside the masks";
static const char* const R_PC_TAIL     = "precode: a mask bit beyond the row's width";
static const char* const R_PC_REACH    = "precode: a masked subcarrier's PRG lies outside the weight block";

static ldpc_hip_dec_desc dec_desc(int bg, unsigned Z)
{
  ldpc_hip_dec_desc d{};
  d.base_graph      = static_cast<uint8_t>(bg);
  d.max_iterations  = 8;
  d.crc_mode        = LDPC_HIP_CRC_MODE_EARLY_STOP;
  d.crc_poly        = 1;
  d.lifting_size    = static_cast<uint16_t>(Z);
  d.nof_filler_bits = 0;
  d.llr_length      = (bg == 1 ? 66U : 50U) * Z;
  d.scaling_factor  = 0.0f;
  d.llr_offset      = 4096;
  d.out_offset      = 512;
  return d;
}

static ldpc_hip_dematch_desc dm_desc(int bg, unsigned Z, unsigned Qm, unsigned E)
{
  ldpc_hip_dematch_desc d{};
  d.modulation_order = static_cast<uint8_t>(Qm);
  d.rv               = 2;
  d.new_data         = 1;
  d.cb_length        = (bg == 1 ? 66U : 50U) * Z;
  d.rm_length        = E;
  d.Nref             = 0;
  d.nof_filler_bits  = 0;
  return d;
}

static const char* dematch(const ldpc_hip_dematch_desc& s, dematch_cb& out, const ldpc_hip_demod_desc* demod = nullptr,
                           const ldpc_hip_scramble_desc* scr = nullptr, const dec_cb* paired = nullptr)
{
  static int8_t llr[4], soft[4];
  static float  sym[64], nv[64];
  return make_dematch_cb(s, llr, soft, demod, sym, nv, scr, paired, out);
}

/* the generator's registers, bit by bit (TS 38.211 5.2.1): 31 bits from bit Nc + offset */
static ldpc_hip_prs_state prs_reference(uint32_t c_init, uint32_t offset)
{
  const uint32_t       n = 1600 + offset + 31;
  std::vector<uint8_t> x1(n + 31, 0), x2(n + 31, 0);
  x1[0] = 1;
  for (int i = 0; i != 31; ++i) {
    x2[i] = (c_init >> i) & 1U;
  }
  for (uint32_t i = 0; i != n; ++i) {
    x1[i + 31] = x1[i + 3] ^ x1[i];
    x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i];
  }
  ldpc_hip_prs_state st{0, 0};
  for (int i = 0; i != 31; ++i) {
    st.x1 |= static_cast<uint32_t>(x1[1600 + offset + i]) << i;
    st.x2 |= static_cast<uint32_t>(x2[1600 + offset + i]) << i;
  }
  return st;
}

static void test_decode_valid()
{
  const struct {
    int      bg;
    unsigned Z;
  } graphs[] = {{1, 384}, {2, 36}, {2, 2}};
  for (const auto& g : graphs) {
    ldpc_hip_dec_desc d = dec_desc(g.bg, g.Z);
    d.nof_filler_bits   = static_cast<uint16_t>(g.Z - 1);
    d.crc_mode          = LDPC_HIP_CRC_MODE_EARLY_STOP | LDPC_HIP_CRC_MODE_FLAG_KEEP_PASSED;
    dec_cb c;
    std::memset(&c, 0xa5, sizeof(c));
    CHECK(make_dec_cb(d, c) == nullptr);
    CHECK(c.llr_offset == 4096 && c.out_offset == 512 && c.llr_length == d.llr_length && c.result_index == 0);
    CHECK(c.nof_filler_bits == g.Z - 1 && c.max_iterations == 8);
    CHECK(c.crc_mode == LDPC_HIP_CRC_MODE_EARLY_STOP && c.keep_passed == 1 && c.crc_poly == 1);
    CHECK(c.pad[0] == 0 && c.pad[1] == 0);
    CHECK(c.scaling_factor == 0.8f); /* 0 selects the default */
    /* the shortest and the longest input */
    d.llr_length = ((g.bg == 1 ? 22U : 10U) + 2U) * g.Z;
    CHECK(make_dec_cb(d, c) == nullptr && c.llr_length == d.llr_length);
    /* no CRC: the polynomial is ignored and forced to 0 */
    d.crc_mode = LDPC_HIP_CRC_MODE_NONE;
    d.crc_poly = 7;
    CHECK(make_dec_cb(d, c) == nullptr && c.crc_mode == 0 && c.crc_poly == 0 && c.keep_passed == 0);
    d.crc_mode       = LDPC_HIP_CRC_MODE_CHECK_AFTER;
    d.crc_poly       = 2;
    d.scaling_factor = 0.75f;
    CHECK(make_dec_cb(d, c) == nullptr && c.crc_mode == 2 && c.crc_poly == 2 && c.scaling_factor == 0.75f);
    CHECK(graph_slot(g.bg, g.Z) == (g.bg - 1) * 51 + lifting_position(g.Z));
    CHECK(msg_bytes_of(g.bg, g.Z) == ((g.bg == 1 ? 22U : 10U) * g.Z + 7U) / 8U);
  }
}

static void test_decode_rejections()
{
  dec_cb                  c;
  const ldpc_hip_dec_desc ok = dec_desc(1, 384);
  ldpc_hip_dec_desc       d  = ok;
  d.base_graph = 3;
  REASON(make_dec_cb(d, c), R_DEC_GRAPH);
  d = ok, d.lifting_size = 37;
  REASON(make_dec_cb(d, c), R_DEC_GRAPH);
  d = ok, d.max_iterations = 0;
  REASON(make_dec_cb(d, c), R_DEC_ITER);
  d = ok, d.llr_length = 24U * 384U - 1U;
  REASON(make_dec_cb(d, c), R_DEC_LEN);
  d = ok, d.llr_length = 66U * 384U + 1U;
  REASON(make_dec_cb(d, c), R_DEC_LEN);
  d = dec_desc(2, 36), d.llr_length = 12U * 36U - 1U;
  REASON(make_dec_cb(d, c), R_DEC_LEN);
  d = dec_desc(2, 36), d.llr_length = 50U * 36U + 1U;
  REASON(make_dec_cb(d, c), R_DEC_LEN);
  d = ok, d.nof_filler_bits = 22U * 384U;
  REASON(make_dec_cb(d, c), R_DEC_FILL);
  d = ok, d.crc_mode = 3;
  REASON(make_dec_cb(d, c), R_DEC_MODE);
  d = ok, d.crc_mode = 3 | LDPC_HIP_CRC_MODE_FLAG_KEEP_PASSED;
  REASON(make_dec_cb(d, c), R_DEC_MODE);
  d = ok, d.crc_poly = 3;
  REASON(make_dec_cb(d, c), R_DEC_POLY);
  d = ok, d.crc_poly = -1;
  REASON(make_dec_cb(d, c), R_DEC_POLY);
  d = ok, d.scaling_factor = 1.0f;
  REASON(make_dec_cb(d, c), R_DEC_SCALE);
  d = ok, d.scaling_factor = -0.5f;
  REASON(make_dec_cb(d, c), R_DEC_SCALE);
  /* order: graph, iterations, length, filler bits, CRC mode, CRC polynomial, scaling factor */
  d = ok, d.scaling_factor = 2.0f, d.crc_poly = 5;
  REASON(make_dec_cb(d, c), R_DEC_POLY);
  d.crc_mode = 9;
  REASON(make_dec_cb(d, c), R_DEC_MODE);
  d.nof_filler_bits = 0xffff;
  REASON(make_dec_cb(d, c), R_DEC_FILL);
  d.llr_length = 1;
  REASON(make_dec_cb(d, c), R_DEC_LEN);
  d.max_iterations = 0;
  REASON(make_dec_cb(d, c), R_DEC_ITER);
  d.lifting_size = 1;
  REASON(make_dec_cb(d, c), R_DEC_GRAPH);
}

static void test_plan_order_and_equivalence()
{
  /* one CB: the plan's item is the one-CB item */
  for (const ldpc_hip_dec_desc& d : {dec_desc(1, 384), dec_desc(2, 36), dec_desc(2, 2)}) {
    dec_cb              one;
    std::vector<dec_cb> cbs;
    CHECK(make_dec_cb(d, one) == nullptr && make_dec_cbs(1, &d, cbs) == nullptr && cbs.size() == 1);
    one.result_index = cbs[0].result_index;
    CHECK(cbs[0].result_index == 0 && std::memcmp(&one, &cbs[0], sizeof(dec_cb)) == 0);
  }
  /* grouped by (BG, Z) in slot order, the default scaling before another, the caller's order inside a group */
  ldpc_hip_dec_desc d[5] = {dec_desc(2, 36), dec_desc(1, 384), dec_desc(2, 36), dec_desc(1, 384), dec_desc(1, 384)};
  d[3].scaling_factor    = 0.5f;
  std::vector<dec_cb> cbs;
  CHECK(make_dec_cbs(5, d, cbs) == nullptr && cbs.size() == 5);
  const uint32_t want[5] = {1, 4, 3, 0, 2};
  for (int i = 0; i != 5; ++i) {
    CHECK(cbs[i].result_index == want[i]);
  }
  CHECK(cbs[2].scaling_factor == 0.5f && cbs[1].scaling_factor == 0.8f);
  /* the first invalid descriptor in the caller's order decides the reason; nothing is produced */
  d[4].max_iterations = 0;
  d[2].crc_mode       = 3;
  cbs.clear();
  REASON(make_dec_cbs(5, d, cbs), R_DEC_MODE);
  CHECK(cbs.empty());
  CHECK(make_dec_cbs(0, nullptr, cbs) == nullptr && cbs.empty());
}

static void test_hw_config()
{
  ldpc_hip_hw_config cfg{};
  cfg.base_graph              = 2;
  cfg.lifting_size            = 36;
  cfg.nof_filler_bits         = 8;
  cfg.max_nof_ldpc_iterations = 6;
  cfg.use_early_stop          = 1;
  cfg.cb_crc_type             = 2;
  ldpc_hip_dec_desc x = make_dec_desc_from_hw(cfg, 1800, 1234, 96);
  CHECK(x.base_graph == 2 && x.lifting_size == 36 && x.nof_filler_bits == 8 && x.max_iterations == 6);
  CHECK(x.crc_mode == LDPC_HIP_CRC_MODE_EARLY_STOP && x.crc_poly == 2 && x.llr_length == 1800);
  CHECK(x.scaling_factor == 0.8f && x.llr_offset == 1234 && x.out_offset == 96);
  cfg.use_early_stop = 0;
  x                  = make_dec_desc_from_hw(cfg, 1800, 0, 0);
  CHECK(x.crc_mode == LDPC_HIP_CRC_MODE_CHECK_AFTER);
  dec_cb c;
  CHECK(make_dec_cb(x, c) == nullptr);
}

static void test_dematch_valid()
{
  static int8_t llr[4], soft[4];
  static float  sym[64], nv[64];
  const struct {
    int      bg;
    unsigned Z, Qm, E;
  } cases[] = {{1, 384, 8, 30000}, {2, 36, 2, 1248}, {2, 2, 1, 77}, {1, 384, 6, 32784 * 3}};
  for (const auto& k : cases) {
    ldpc_hip_dematch_desc s = dm_desc(k.bg, k.Z, k.Qm, k.E);
    s.Nref                  = s.cb_length - 1;
    s.nof_filler_bits       = k.Z - 1;
    dematch_cb c;
    std::memset(static_cast<void*>(&c), 0xa5, sizeof(c));
    CHECK(make_dematch_cb(s, llr + 1, soft + 2, nullptr, nullptr, nullptr, nullptr, nullptr, c) == nullptr);
    CHECK(c.llr == llr + 1 && c.soft == soft + 2 && c.sym == nullptr && c.nv == nullptr);
    CHECK(c.cb_length == s.cb_length && c.rm_length == k.E && c.Nref == s.cb_length - 1);
    CHECK(c.nof_filler_bits == k.Z - 1 && c.modulation_order == k.Qm && c.rv == 2 && c.new_data == 1);
    CHECK(c.demod == 0 && c.stage_bytes == 0 && c.scr_x1 == 0 && c.scr_x2 == 0);
    /* a disabled scrambling descriptor changes nothing, whatever the length */
    const ldpc_hip_scramble_desc off{12345, 0, {0, 0, 0}, 99};
    dematch_cb                   c2;
    CHECK(make_dematch_cb(s, llr + 1, soft + 2, nullptr, nullptr, nullptr, &off, nullptr, c2) == nullptr);
    CHECK(std::memcmp(&c, &c2, sizeof(c)) == 0);
  }
  /* demodulated: 64-QAM, 200 symbols */
  ldpc_hip_dematch_desc s = dm_desc(2, 36, 6, 1200);
  ldpc_hip_demod_desc   m{};
  m.symbol_offset = 5;
  m.noise_offset  = 7;
  m.nof_symbols   = 200;
  m.modulation    = 6;
  dematch_cb c;
  CHECK(make_dematch_cb(s, llr, soft, &m, sym, nv, nullptr, nullptr, c) == nullptr);
  CHECK(c.llr == nullptr && c.soft == soft && c.sym == sym + 10 && c.nv == nv + 7 && c.demod == 6);
  CHECK(c.rm_length == 1200 && c.modulation_order == 6 && c.scr_x1 == 0);
  /* BPSK and pi/2-BPSK (modulation 0 and 1) both carry one bit per symbol */
  s = dm_desc(2, 36, 1, 200), m.modulation = 0;
  CHECK(make_dematch_cb(s, llr, soft, &m, sym, nv, nullptr, nullptr, c) == nullptr && c.demod == 0 && c.sym == sym + 10);
  /* scrambled: the start state is ldpc_hip_prs_init's (prs_state_at), checked against the registers bit by bit */
  for (const uint32_t offset : {0U, 1U, 31U, 12345U}) {
    const ldpc_hip_scramble_desc scr{0x1234567U, 1, {0, 0, 0}, offset};
    s = dm_desc(1, 384, 4, 32768);
    CHECK(make_dematch_cb(s, llr, soft, nullptr, nullptr, nullptr, &scr, nullptr, c) == nullptr);
    const ldpc_hip_prs_state at = prs_state_at(0x1234567U, offset), ref = prs_reference(0x1234567U, offset);
    CHECK(at.x1 == ref.x1 && at.x2 == ref.x2 && at.x1 != 0);
    CHECK(c.scr_x1 == ref.x1 && c.scr_x2 == ref.x2 && c.llr == llr);
  }
  /* fused: the decode work item it feeds agrees */
  dec_cb                  cb;
  const ldpc_hip_dec_desc dd = dec_desc(2, 36);
  CHECK(make_dec_cb(dd, cb) == nullptr);
  s = dm_desc(2, 36, 2, 1248);
  CHECK(make_dematch_cb(s, llr, soft, nullptr, nullptr, nullptr, nullptr, &cb, c) == nullptr && c.cb_length == 1800);
}

static void test_dematch_rejections()
{
  dematch_cb                  c;
  const ldpc_hip_dematch_desc ok = dm_desc(2, 36, 2, 1248);
  ldpc_hip_dematch_desc       s  = ok;
  s.rv = 4;
  REASON(dematch(s, c), R_DM_PARAMS);
  s = ok, s.modulation_order = 3;
  REASON(dematch(s, c), R_DM_PARAMS);
  s = ok, s.modulation_order = 4, s.rm_length = 1250;
  REASON(dematch(s, c), R_DM_PARAMS);
  s = ok, s.cb_length = 1801;
  REASON(dematch(s, c), R_DM_LEN);
  s = ok, s.cb_length = 50 * 37; /* 37 is no lifting size */
  REASON(dematch(s, c), R_DM_LEN);
  s = ok, s.cb_length = 66 * 385;
  REASON(dematch(s, c), R_DM_LARGE);
  s = ok, s.Nref = 66 * 384 + 1;
  REASON(dematch(s, c), R_DM_LARGE);
  s = ok, s.nof_filler_bits = 8 * 36;
  REASON(dematch(s, c), R_DM_FILL);
  s = dm_desc(1, 384, 2, 1248), s.nof_filler_bits = 20 * 384;
  REASON(dematch(s, c), R_DM_FILL);
  /* demodulated */
  ldpc_hip_demod_desc m{};
  m.nof_symbols = 623; /* x 2 = 1246 */
  m.modulation  = 2;
  REASON(dematch(ok, c, &m), R_DM_DEMOD);
  m.nof_symbols = 624, m.modulation = 4; /* bits per symbol differ from Qm */
  REASON(dematch(ok, c, &m), R_DM_DEMOD);
  m.modulation = 3;
  REASON(dematch(ok, c, &m), R_DM_DEMOD);
  s = dm_desc(1, 384, 2, 32784), m.modulation = 2, m.nof_symbols = 16392;
  REASON(dematch(s, c, &m), R_DM_DEMOD);
  dec_cb                  cb;
  const ldpc_hip_dec_desc dd = dec_desc(1, 384);
  CHECK(make_dec_cb(dd, cb) == nullptr);
  REASON(dematch(s, c, &m, nullptr, &cb), R_DM_DEMOD_F);
  /* scrambled */
  const ldpc_hip_scramble_desc scr{1, 1, {0, 0, 0}, 0};
  REASON(dematch(s, c, nullptr, &scr), R_DM_SCR);
  s.rm_length = 32768;
  CHECK(dematch(s, c, nullptr, &scr) == nullptr);
  /* fused: length or filler bits differ from the decode item */
  cb.llr_length -= 384;
  REASON(dematch(s, c, nullptr, nullptr, &cb), R_DM_PAIRED);
  cb.llr_length += 384, cb.nof_filler_bits = 1;
  REASON(dematch(s, c, nullptr, nullptr, &cb), R_DM_PAIRED);
  cb.nof_filler_bits = 0;
  /* order: descriptor, then the fused pair, then the demodulator, then scrambling */
  s = dm_desc(1, 384, 2, 32784), m.nof_symbols = 1;
  REASON(dematch(s, c, &m, &scr, &cb), R_DM_DEMOD_F);
  cb.nof_filler_bits = 1;
  REASON(dematch(s, c, &m, &scr, &cb), R_DM_PAIRED);
  s.nof_filler_bits = 20 * 384;
  REASON(dematch(s, c, &m, &scr, &cb), R_DM_FILL);
  s.Nref = 1U << 20;
  REASON(dematch(s, c, &m, &scr, &cb), R_DM_LARGE);
  s.rv = 7;
  REASON(dematch(s, c, &m, &scr, &cb), R_DM_PARAMS);
  m.nof_symbols = 16392;
  REASON(dematch(dm_desc(1, 384, 2, 32784), c, &m, &scr), R_DM_DEMOD); /* the demodulator before scrambling */
}

/* a limited buffer must cover the systematic bits: Ncb = (K - 2) Z - 1 would wrap the allot loop's parity range
 * (Ncb - tmp_idx with tmp_idx raised to (K - 2) Z) and write past the soft buffer; Ncb = (K - 2) Z is the legal edge */
static void test_dematch_buffer_boundary()
{
  const struct {
    int      bg;
    unsigned Z, K;
  } graphs[] = {{1, 2, 22}, {1, 384, 22}, {2, 2, 10}, {2, 36, 10}, {2, 384, 10}};
  for (const auto& g : graphs) {
    const unsigned        nsys = (g.K - 2) * g.Z;
    ldpc_hip_dematch_desc s    = dm_desc(g.bg, g.Z, 2, 2 * g.Z + 6);
    s.nof_filler_bits          = g.Z / 2;
    dematch_cb c;
    s.Nref = nsys - 1;
    REASON(dematch(s, c), R_DM_NCB);
    s.Nref = 1;
    REASON(dematch(s, c), R_DM_NCB);
    for (const unsigned nref : {nsys, nsys + 1, s.cb_length, std::min(s.cb_length + 7U, 66U * 384U)}) {
      s.Nref = nref;
      std::memset(static_cast<void*>(&c), 0xa5, sizeof(c));
      CHECK(dematch(s, c) == nullptr);
      CHECK(c.Nref == nref && c.cb_length == s.cb_length && c.rm_length == 2 * g.Z + 6 && c.modulation_order == 2);
      CHECK(c.nof_filler_bits == g.Z / 2 && c.rv == 2 && c.new_data == 1 && c.sym == nullptr && c.scr_x1 == 0);
    }
    /* the refusal comes after the filler check and before the fused pair's */
    s.Nref = nsys - 1, s.nof_filler_bits = nsys;
    REASON(dematch(s, c), R_DM_FILL);
    s.nof_filler_bits = g.Z / 2;
    dec_cb                  cb;
    const ldpc_hip_dec_desc dd = dec_desc(g.bg, g.Z);
    CHECK(make_dec_cb(dd, cb) == nullptr);
    cb.nof_filler_bits = static_cast<uint16_t>(g.Z / 2 + 1);
    REASON(dematch(s, c, nullptr, nullptr, &cb), R_DM_NCB);
  }
}

static void test_encoder()
{
  enc_cb            e;
  ldpc_hip_enc_desc d{64, 128, 66 * 384, 384, 1, 0};
  CHECK(make_enc_cb(d, nullptr, e) == nullptr);
  CHECK(e.msg_offset == 64 && e.cw_offset == 128 && e.cw_length == 66 * 384 && e.graph_slot == graph_slot(1, 384));
  CHECK(e.msg_bit_off == 0 && e.data_bits == 22 * 384 && e.crc_at == 0 && e.pad == 0);
  const uint32_t ext[3] = {5, 8000, 8424};
  CHECK(make_enc_cb(d, ext, e) == nullptr && e.msg_bit_off == 5 && e.data_bits == 8000 && e.crc_at == 8424);
  ldpc_hip_enc_desc d2{0, 0, 100, 2, 2, 0};
  CHECK(make_enc_cb(d2, nullptr, e) == nullptr && e.graph_slot == 51 && e.data_bits == 20);
  d2.lifting_size = 1;
  REASON(make_enc_cb(d2, nullptr, e), "encode_launch: invalid base graph / lifting size");
  d2 = d, d2.base_graph = 0;
  REASON(make_enc_cb(d2, nullptr, e), "encode_launch: invalid base graph / lifting size");
  d2 = d, d2.cw_length = 0;
  REASON(make_enc_cb(d2, nullptr, e), "encode_launch: codeword length out of range");
  d2.cw_length = 66 * 384 + 1;
  REASON(make_enc_cb(d2, nullptr, e), "encode_launch: codeword length out of range");
  const uint32_t bad_off[3] = {8, 8000, 0}, bad_data[3] = {0, 8449, 0}, bad_crc[3] = {0, 8000, 8425},
                 bad_crc2[3] = {0, 8300, 8200};
  REASON(make_enc_cb(d, bad_off, e), "encode_launch: message bit range out of range");
  REASON(make_enc_cb(d, bad_data, e), "encode_launch: message bit range out of range");
  REASON(make_enc_cb(d, bad_crc, e), "encode_launch: message bit range out of range");
  REASON(make_enc_cb(d, bad_crc2, e), "encode_launch: message bit range out of range");
  REASON(make_enc_cb(d2, bad_off, e), "encode_launch: codeword length out of range"); /* order */
}

static void test_rate_matcher()
{
  ratematch_cb     r;
  ldpc_hip_rm_desc d{32, 96, 66 * 384, 30000, 0, 100, 8, 2};
  CHECK(make_rm_cb(d, r) == nullptr);
  CHECK(r.cw_offset == 32 && r.out_offset == 96 && r.cb_length == 25344 && r.rm_length == 30000 && r.Ncb == 25344);
  CHECK(r.k0 == 33 * 384 && r.fill_lo == 20 * 384 - 100 && r.fill_hi == 20 * 384 && r.Qm == 8 && r.pad == 0);
  d.Nref = 20000; /* limited buffer: k0 = floor(33 Ncb / N) Z */
  CHECK(make_rm_cb(d, r) == nullptr && r.Ncb == 20000 && r.k0 == (33U * 20000U / 25344U) * 384U);
  ldpc_hip_rm_desc d2{0, 0, 50 * 36, 1248, 0, 0, 2, 3};
  CHECK(make_rm_cb(d2, r) == nullptr && r.k0 == 43 * 36 && r.fill_lo == 8 * 36 && r.fill_hi == 8 * 36);
  d2.cb_length = 100; /* BG2 Z = 2 */
  CHECK(make_rm_cb(d2, r) == nullptr && r.k0 == 43 * 2);
  d2.cb_length = 1801;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid codeblock length");
  d2.cb_length = 50 * 37;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.cb_length = 1800, d2.rv = 4;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.rv = 0, d2.modulation_order = 0;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.modulation_order = 9;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.modulation_order = 2, d2.rm_length = 0;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.rm_length = 1249;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters");
  d2.rm_length = 1248, d2.nof_filler_bits = 8 * 36;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid number of filler bits");
  d2.rv = 4;
  REASON(make_rm_cb(d2, r), "rate_match_launch: invalid parameters"); /* order */
}

static void test_pdsch()
{
  pdsch_enc_cb      c;
  ldpc_hip_enc_desc ed{64, 0, 50 * 36, 36, 2, 0};
  ldpc_hip_rm_desc  rd{0, 96, 50 * 36, 1248, 0, 0, 2, 0};
  const uint32_t    ext[3] = {0, 300, 0};
  CHECK(make_pdsch_cb(ed, ext, rd, c) == nullptr);
  CHECK(c.enc.graph_slot == graph_slot(2, 36) && c.enc.data_bits == 300 && c.rm.rm_length == 1248 && c.rm.out_offset == 96);
  ed.cw_length = 40 * 36;
  REASON(make_pdsch_cb(ed, ext, rd, c), "pdsch_encode: encoder and rate matcher descriptors disagree");
  ed.cw_length = 0;
  REASON(make_pdsch_cb(ed, ext, rd, c), "encode_launch: codeword length out of range");
  ed.cw_length = 50 * 36, rd.rv = 4;
  REASON(make_pdsch_cb(ed, ext, rd, c), "rate_match_launch: invalid parameters");
  /* the lengths agree, the base graphs do not: 1800 bits are a whole BG2 codeword and a BG1 codeword's start */
  rd.rv = 0, ed.base_graph = 1;
  REASON(make_pdsch_cb(ed, ext, rd, c), "pdsch_encode: encoder and rate matcher descriptors disagree");
}

static void test_tb_join()
{
  /* msg_offset, tb_offset, msg_stride, tbs, result_index, nof_cbs, cb_msg_bits, nof_filler_bits, cb_crc_bits, pad */
  const ldpc_hip_tb_desc one{0, 0, 45, 256, 0, 1, 360, 80, 24, 0};
  CHECK(tb_desc_reason(one) == nullptr);
  const ldpc_hip_tb_desc two{0, 0, 1056, 16000, 0, 2, 8448, 412, 24, 0}; /* kd = 8012: 16000 - 8012 + 24 = 8012 */
  CHECK(tb_desc_reason(two) == nullptr);
  ldpc_hip_tb_desc d = one;
  d.nof_cbs = 0;
  REASON(tb_desc_reason(d), "tb_join: invalid sizes");
  d = one, d.tbs = 0;
  REASON(tb_desc_reason(d), "tb_join: invalid sizes");
  d = one, d.tbs = 250;
  REASON(tb_desc_reason(d), "tb_join: invalid sizes");
  d = one, d.msg_stride = 44;
  REASON(tb_desc_reason(d), "tb_join: invalid sizes");
  d = one, d.cb_crc_bits = 8;
  REASON(tb_desc_reason(d), "tb_join: CRC length must be 16 or 24");
  d = two, d.tbs = 8U * 4096U * 64U + 8U;
  REASON(tb_desc_reason(d), "tb_join: transport block too large");
  d = one, d.tbs = 264;
  REASON(tb_desc_reason(d), "tb_join: TB larger than its codeblock");
  d = two, d.cb_crc_bits = 16;
  REASON(tb_desc_reason(d), "tb_join: segmentation inconsistent with the TB size");
  d = two, d.tbs = 8008; /* fits one codeblock */
  REASON(tb_desc_reason(d), "tb_join: segmentation inconsistent with the TB size");
  d = two, d.tbs = 16008;
  REASON(tb_desc_reason(d), "tb_join: segmentation inconsistent with the TB size");
  d = two, d.nof_filler_bits = 8448 - 24;
  REASON(tb_desc_reason(d), "tb_join: segmentation inconsistent with the TB size");
  d = two, d.cb_crc_bits = 8, d.tbs = 4; /* order: sizes before the CRC length */
  REASON(tb_desc_reason(d), "tb_join: invalid sizes");
}

/* the segment launches' array forms, as their entry points call them */
static const char* make_demod_segs(uint32_t n, const ldpc_hip_demod_desc* d, std::vector<demod_seg>& g, uint32_t& nb)
{
  return make_segs(n, d, g, nb, make_demod_seg);
}
static const char* make_prs_segs(uint32_t n, const ldpc_hip_prs_seg* d, bool has_input, std::vector<prs_seg>& g,
                                 uint32_t& nb)
{
  return make_segs(n, d, g, nb, make_prs_seg, has_input);
}
static const char* make_mod_segs(uint32_t n, const ldpc_hip_mod_desc* d, std::vector<mod_seg>& g, uint32_t& nb)
{
  return make_segs(n, d, g, nb, make_mod_seg);
}
static const char* make_eq_segs(uint32_t n, const ldpc_hip_eq_desc* d, std::vector<eq_seg>& g, uint32_t& nb)
{
  return make_segs(n, d, g, nb, make_eq_seg);
}

/* `count` copies of d hold at most MAX_LAUNCH_BLOCKS blocks, each per_seg of them, and one more does not */
template <typename D, typename G, typename Make>
static void check_block_cap(const D& d, uint32_t count, uint32_t per_seg, const char* reason, Make make)
{
  CHECK(static_cast<uint64_t>(count) * per_seg <= MAX_LAUNCH_BLOCKS);
  CHECK(static_cast<uint64_t>(count + 1) * per_seg > MAX_LAUNCH_BLOCKS);
  std::vector<D> descs(count + 1, d);
  std::vector<G> segs;
  uint32_t       nblocks = 0;
  CHECK(make(count, descs.data(), segs, nblocks) == nullptr && segs.size() == count && nblocks == count * per_seg);
  CHECK(segs[count - 1].block0 == (count - 1) * per_seg);
  REASON(make(count + 1, descs.data(), segs, nblocks), reason);
}

static void test_demodulator()
{
  ldpc_hip_demod_desc d[3]{};
  d[0].symbol_offset = 5, d[0].noise_offset = 7, d[0].llr_offset = 128, d[0].nof_symbols = 64, d[0].modulation = 2;
  d[1].modulation    = 4; /* empty: validated, then dropped */
  d[2].symbol_offset = 69, d[2].noise_offset = 71, d[2].llr_offset = 256, d[2].nof_symbols = 300, d[2].modulation = 6;
  std::vector<demod_seg> sg;
  uint32_t               nblocks = 0;
  CHECK(make_demod_segs(3, d, sg, nblocks) == nullptr && sg.size() == 2 && nblocks == 3);
  CHECK(sg[0].sym_offset == 5 && sg[0].noise_offset == 7 && sg[0].llr_offset == 128 && sg[0].nof_symbols == 64);
  CHECK(sg[0].block0 == 0 && sg[0].modulation == 2 && sg[0].qm == 2);
  CHECK(sg[1].sym_offset == 69 && sg[1].noise_offset == 71 && sg[1].llr_offset == 256 && sg[1].nof_symbols == 300);
  CHECK(sg[1].block0 == 1 && sg[1].modulation == 6 && sg[1].qm == 6);
  for (const demod_seg& g : sg) {
    for (const uint8_t p : g.pad) {
      CHECK(p == 0);
    }
  }
  /* pi/2-BPSK: one bit per symbol; a whole block and one symbol more */
  d[0].modulation = 0, d[0].nof_symbols = 257;
  CHECK(make_demod_segs(1, d, sg, nblocks) == nullptr && sg.size() == 1 && sg[0].qm == 1 && nblocks == 2);
  CHECK(make_demod_segs(0, nullptr, sg, nblocks) == nullptr && sg.empty() && nblocks == 0);
  d[1].modulation = 3; /* the empty segment's scheme counts */
  REASON(make_demod_segs(3, d, sg, nblocks), R_DEMOD_MOD);
  ldpc_hip_demod_desc big{};
  big.nof_symbols = 0xffffffffU; /* 2^24 blocks */
  big.modulation  = 2;
  check_block_cap<ldpc_hip_demod_desc, demod_seg>(big, 127, 1U << 24, R_DEMOD_MANY, make_demod_segs);
}

static void test_sequences()
{
  ldpc_hip_prs_seg s[3]{};
  s[0].in_offset = 5, s[0].out_offset = 7, s[0].seq_offset = 12345, s[0].length = 1, s[0].c_init = 0x1234567U;
  s[1].in_offset = 9, s[1].c_init = 3; /* empty */
  s[2].in_offset = 64, s[2].out_offset = 96, s[2].seq_offset = 31, s[2].length = 32769, s[2].c_init = 0x7fffffffU;
  for (const bool has_input : {true, false}) {
    std::vector<prs_seg> sg;
    uint32_t             nblocks = 0;
    CHECK(make_prs_segs(3, s, has_input, sg, nblocks) == nullptr && sg.size() == 2);
    /* 1 bit is one word, one block; 32769 bits are 1025 words, one more than a block's PRS_BLOCK x PRS_WORDS */
    CHECK(nblocks == 3 && sg[0].block0 == 0 && sg[1].block0 == 1);
    CHECK(sg[0].in_offset == (has_input ? 5U : PRS_NO_INPUT) && sg[1].in_offset == (has_input ? 64U : PRS_NO_INPUT));
    CHECK(sg[0].out_offset == 7 && sg[0].length == 1 && sg[1].out_offset == 96 && sg[1].length == 32769);
    const ldpc_hip_prs_state r0 = prs_reference(0x1234567U, 12345), r1 = prs_reference(0x7fffffffU, 31);
    CHECK(sg[0].x1 == r0.x1 && sg[0].x2 == r0.x2 && sg[1].x1 == r1.x1 && sg[1].x2 == r1.x2);
  }
  std::vector<prs_seg> sg;
  uint32_t             nblocks = 0;
  s[1].c_init = 0x80000000U; /* the empty segment's c_init counts */
  REASON(make_prs_segs(3, s, true, sg, nblocks), R_PRS_CINIT);
  ldpc_hip_prs_seg big{};
  big.length = 0xffffffffU; /* 2^27 words, 2^17 blocks */
  check_block_cap<ldpc_hip_prs_seg, prs_seg>(
      big, 16383, 1U << 17, R_PRS_MANY,
      [](uint32_t n, const ldpc_hip_prs_seg* d, std::vector<prs_seg>& g, uint32_t& b) {
        return make_prs_segs(n, d, false, g, b);
      });
}

static ldpc_hip_mod_desc mod_desc(unsigned modulation, uint32_t nof_symbols, bool scramble)
{
  ldpc_hip_mod_desc d{};
  d.bit_offset    = 11;
  d.symbol_offset = 13;
  d.seq_offset    = 777;
  d.nof_symbols   = nof_symbols;
  d.c_init        = scramble ? 0x2345678U : 0xffffffffU; /* ignored when the bits are mapped as they are */
  d.modulation    = static_cast<uint8_t>(modulation);
  d.scramble      = scramble ? 1 : 0;
  return d;
}

static void test_mapper()
{
  /* a thread maps one chunk of 32 bits (96 for 64-QAM), a block MOD_BLOCK chunks: 100 QPSK symbols are 7 chunks, 4097
   * symbols of 64-QAM 257 chunks, 1025 symbols of 256-QAM 257 chunks */
  const ldpc_hip_mod_desc d[4] = {mod_desc(2, 100, true), mod_desc(4, 0, true), mod_desc(6, 4097, false),
                                  mod_desc(8, 1025, true)};
  std::vector<mod_seg>    sg;
  uint32_t                nblocks = 0;
  CHECK(make_mod_segs(4, d, sg, nblocks) == nullptr && sg.size() == 3 && nblocks == 5);
  const uint32_t           block0[3] = {0, 1, 3}, syms[3] = {100, 4097, 1025}, mods[3] = {2, 6, 8};
  const ldpc_hip_prs_state ref       = prs_reference(0x2345678U, 777);
  for (int i = 0; i != 3; ++i) {
    CHECK(sg[i].bit_offset == 11 && sg[i].sym_offset == 13 && sg[i].nof_symbols == syms[i]);
    CHECK(sg[i].block0 == block0[i] && sg[i].modulation == mods[i]);
    CHECK(sg[i].x1 == (i == 1 ? 0U : ref.x1) && sg[i].x2 == (i == 1 ? 0U : ref.x2));
    for (const uint8_t p : sg[i].pad) {
      CHECK(p == 0);
    }
  }
  /* one descriptor: the item starts at the launch's count so far and advances it */
  uint64_t blocks = 40;
  mod_seg  g;
  CHECK(make_mod_seg(d[2], blocks, g) == nullptr && g.block0 == 40 && blocks == 42);
  CHECK(make_mod_seg(d[1], blocks, g) == nullptr && blocks == 42);
  ldpc_hip_mod_desc x = mod_desc(3, 100, true);
  REASON(make_mod_seg(x, blocks, g), R_MOD_MOD);
  x = mod_desc(2, 100, true), x.c_init = 0x80000000U;
  REASON(make_mod_seg(x, blocks, g), R_MOD_CINIT);
  x = mod_desc(2, 0x80000000U, true);
  REASON(make_mod_seg(x, blocks, g), R_MOD_SEG);
  /* order: scheme, c_init, the segment's size */
  x.c_init = 0x80000000U;
  REASON(make_mod_seg(x, blocks, g), R_MOD_CINIT);
  x.modulation = 5;
  REASON(make_mod_seg(x, blocks, g), R_MOD_MOD);
  REASON(make_mod_segs(1, &x, sg, nblocks), R_MOD_MOD);
  /* 2^31 - 1 symbols of 256-QAM: 2^29 chunks, 2^21 blocks */
  check_block_cap<ldpc_hip_mod_desc, mod_seg>(mod_desc(8, 0x7fffffffU, false), 1023, 1U << 21, R_MOD_MANY,
                                              make_mod_segs);
}

static void test_rate_match_mapper()
{
  const ldpc_hip_rm_desc  rd{32, 96, 66 * 384, 30000, 0, 100, 8, 2};
  const ldpc_hip_mod_desc md = mod_desc(8, 3750, true);
  /* the pair is the rate matcher's item and the mapper's, each as translated alone */
  rm_mod_cb    cb;
  ratematch_cb r;
  mod_seg      g;
  uint64_t     blocks = 7, blocks_alone = 7;
  std::memset(&cb, 0xa5, sizeof(cb));
  CHECK(make_rm_mod_cb(rd, md, blocks, cb) == nullptr);
  CHECK(make_rm_cb(rd, r) == nullptr && make_mod_seg(md, blocks_alone, g) == nullptr);
  CHECK(std::memcmp(&cb.rm, &r, sizeof(r)) == 0 && std::memcmp(&cb.mod, &g, sizeof(g)) == 0);
  CHECK(blocks == blocks_alone && blocks == 7 + 4 && cb.mod.block0 == 7); /* 938 chunks of 4 symbols */
  /* the pair's own reasons */
  ldpc_hip_rm_desc  r1{0, 0, 50 * 36, 1248, 0, 0, 1, 0};
  ldpc_hip_mod_desc m1 = mod_desc(LDPC_HIP_MOD_PI_2_BPSK, 1248, false);
  REASON(make_rm_mod_cb(r1, m1, blocks, cb), R_RMMOD_BPSK);
  m1.modulation = LDPC_HIP_MOD_BPSK;
  CHECK(make_rm_mod_cb(r1, m1, blocks, cb) == nullptr);
  ldpc_hip_mod_desc m = md;
  m.nof_symbols       = 3749;
  REASON(make_rm_mod_cb(rd, m, blocks, cb), R_RMMOD_PAIR);
  m = mod_desc(6, 5000, true); /* 30000 bits, but not the rate matcher's interleaving */
  REASON(make_rm_mod_cb(rd, m, blocks, cb), R_RMMOD_PAIR);
  ldpc_hip_rm_desc r2 = rd;
  r2.modulation_order = 2, r2.rm_length = 0x80000000U;
  REASON(make_rm_mod_cb(r2, mod_desc(2, 0x40000000U, true), blocks, cb), R_RMMOD_PAIR);
  /* order: the rate matcher, the mapper, pi/2-BPSK, the pair's lengths */
  m1.modulation = LDPC_HIP_MOD_PI_2_BPSK, m1.nof_symbols = 1247;
  REASON(make_rm_mod_cb(r1, m1, blocks, cb), R_RMMOD_BPSK);
  m1.scramble = 1;
  REASON(make_rm_mod_cb(r1, m1, blocks, cb), R_MOD_CINIT);
  r1.rv = 4;
  REASON(make_rm_mod_cb(r1, m1, blocks, cb), R_RM_PARAMS);
}

static ldpc_hip_eq_desc eq_desc(int algorithm, unsigned ports, unsigned layers, uint32_t nof_re, uint64_t stride)
{
  ldpc_hip_eq_desc d{};
  d.sym_offset    = 3;
  d.sym_stride    = stride;
  d.est_offset    = 17;
  d.est_stride    = stride + 1;
  d.out_offset    = 29;
  d.nof_re        = nof_re;
  d.tx_scaling    = 0.5f;
  d.algorithm     = static_cast<uint8_t>(algorithm);
  d.nof_rx_ports  = static_cast<uint8_t>(ports);
  d.nof_tx_layers = static_cast<uint8_t>(layers);
  for (int p = 0; p != 4; ++p) {
    d.noise_var[p] = 0.25f * static_cast<float>(p + 1);
  }
  return d;
}

static void test_equalizer()
{
  /* a block equalises EQ_BLOCK x EQ_RES = 256 REs: 1025 REs are 5 blocks */
  const ldpc_hip_eq_desc d[3] = {eq_desc(LDPC_HIP_EQ_MMSE, 1, 1, 5, 8), eq_desc(LDPC_HIP_EQ_ZF, 4, 1, 0, 0),
                                 eq_desc(LDPC_HIP_EQ_ZF, 4, 2, 1025, 2000)};
  std::vector<eq_seg>    sg;
  uint32_t               nblocks = 0;
  CHECK(make_eq_segs(3, d, sg, nblocks) == nullptr && sg.size() == 2 && nblocks == 6);
  CHECK(sg[0].nof_re == 5 && sg[0].block0 == 0 && sg[0].sym_stride == 8 && sg[0].est_stride == 9);
  CHECK(sg[0].algorithm == LDPC_HIP_EQ_MMSE && sg[0].nof_rx_ports == 1 && sg[0].nof_tx_layers == 1);
  CHECK(sg[1].nof_re == 1025 && sg[1].block0 == 1 && sg[1].sym_stride == 2000 && sg[1].est_stride == 2001);
  CHECK(sg[1].algorithm == LDPC_HIP_EQ_ZF && sg[1].nof_rx_ports == 4 && sg[1].nof_tx_layers == 2);
  for (const eq_seg& g : sg) {
    CHECK(g.sym_offset == 3 && g.est_offset == 17 && g.out_offset == 29 && g.tx_scaling == 0.5f && g.pad == 0);
    CHECK(g.noise_var[0] == 0.25f && g.noise_var[1] == 0.5f && g.noise_var[2] == 0.75f && g.noise_var[3] == 1.0f);
  }
  uint64_t blocks = 9;
  eq_seg   g;
  CHECK(make_eq_seg(d[2], blocks, g) == nullptr && g.block0 == 9 && blocks == 14);
  REASON(make_eq_seg(eq_desc(LDPC_HIP_EQ_MMSE, 2, 2, 5, 8), blocks, g), R_EQ_TOPOLOGY);
  REASON(make_eq_seg(eq_desc(LDPC_HIP_EQ_ZF, 3, 2, 5, 8), blocks, g), R_EQ_TOPOLOGY);
  REASON(make_eq_seg(eq_desc(2, 1, 1, 5, 8), blocks, g), R_EQ_TOPOLOGY);
  ldpc_hip_eq_desc x = d[0];
  for (const float bad : {0.0f, -1.0f, std::nanf("")}) {
    x.tx_scaling = bad;
    REASON(make_eq_seg(x, blocks, g), R_EQ_SCALING);
  }
  x = d[0], x.sym_stride = 4;
  REASON(make_eq_seg(x, blocks, g), R_EQ_STRIDE);
  x = d[0], x.est_stride = 4;
  REASON(make_eq_seg(x, blocks, g), R_EQ_STRIDE);
  x = eq_desc(LDPC_HIP_EQ_ZF, 2, 2, 0x40000000U, 0x40000000U);
  REASON(make_eq_seg(x, blocks, g), R_EQ_SEG);
  /* order: topology, scaling, strides, the segment's size; the empty segment is validated too */
  x.sym_stride = 1;
  REASON(make_eq_seg(x, blocks, g), R_EQ_STRIDE);
  x.tx_scaling = std::nanf("");
  REASON(make_eq_seg(x, blocks, g), R_EQ_SCALING);
  x.algorithm = LDPC_HIP_EQ_MMSE;
  REASON(make_eq_seg(x, blocks, g), R_EQ_TOPOLOGY);
  CHECK(blocks == 14);
  x = d[1], x.tx_scaling = 0.0f;
  REASON(make_eq_segs(1, &x, sg, nblocks), R_EQ_SCALING);
  /* 2^31 - 1 REs of one layer: 2^23 blocks */
  check_block_cap<ldpc_hip_eq_desc, eq_seg>(eq_desc(LDPC_HIP_EQ_ZF, 1, 1, 0x7fffffffU, 0x7fffffffU), 255, 1U << 23,
                                            R_EQ_MANY, make_eq_segs);
}

static ldpc_hip_precode_desc pc_desc(uint32_t width, uint32_t mask_offset, unsigned layers, unsigned ports,
                                     uint32_t nof_prg, unsigned prg_size)
{
  ldpc_hip_precode_desc d{};
  d.sym_offset    = 5;
  d.grid_offset   = 9;
  d.port_stride   = width + 3U;
  d.mask_offset   = mask_offset;
  d.weight_offset = 0;
  d.nof_prg       = nof_prg;
  d.width         = width;
  d.prg_size      = static_cast<uint16_t>(prg_size);
  d.nof_layers    = static_cast<uint8_t>(layers);
  d.nof_ports     = static_cast<uint8_t>(ports);
  return d;
}

/* ceil(width / 64) mask words with bits [lo, hi) set */
static std::vector<uint64_t> pc_mask(uint32_t width, uint32_t lo, uint32_t hi)
{
  std::vector<uint64_t> m((width + 63U) / 64U, 0);
  for (uint32_t k = lo; k < hi; ++k) {
    m[k / 64U] |= 1ULL << (k % 64U);
  }
  return m;
}

static std::vector<float> pc_weights(uint32_t nof_weights)
{
  std::vector<float> w(2U * nof_weights);
  for (size_t i = 0; i != w.size(); ++i) {
    w[i] = 0.25f * static_cast<float>(i % 7U) - 0.5f;
  }
  return w;
}

static float float_of(uint32_t bits)
{
  float f;
  std::memcpy(&f, &bits, sizeof(f));
  return f;
}

struct pc_launch {
  std::vector<ldpc_hip_precode_desc> descs;
  std::vector<float>                 weights;
  std::vector<uint64_t>              masks;
  bool                               compact   = false;
  uint64_t                           in_stride = 0;
  const char* make(precode_table& t) const
  {
    return make_precode_table(static_cast<uint32_t>(descs.size()), descs.data(), weights.data(),
                              static_cast<uint32_t>(weights.size() / 2U), masks.data(),
                              static_cast<uint32_t>(masks.size()), compact, in_stride, t);
  }
};

/* An accepted launch's table against the plain rule: per row the first and last non-zero mask word give k_begin and
 * k_end, ceil((k_end - k_begin) / (PC_BLOCK PC_RES)) its blocks; a mask's words once per (mask_offset, words), each
 * with the popcount of the row's earlier words; the blob the three arrays back to back. */
static void check_pc_table(const pc_launch& l, int line)
{
  precode_table t;
  t.blob.assign(3, 0xa5); /* a used table is reset */
  t.nblocks = 77;
  const char* why = l.make(t);
  if (why != nullptr) {
    std::printf("FAIL line %d: refused: %s\n", line, why);
    ++g_failed;
    return;
  }
  std::vector<precode_row>  rows;
  std::vector<precode_word> words;
  struct shared {
    uint32_t mask_offset, nw, word0;
  };
  std::vector<shared> seen;
  uint32_t            blocks = 0;
  for (const ldpc_hip_precode_desc& d : l.descs) {
    const uint32_t  nw = (d.width + 63U) / 64U;
    const uint64_t* m  = l.masks.data() + d.mask_offset;
    int             first = -1, last = -1;
    for (uint32_t w = 0; w != nw; ++w) {
      if (m[w] != 0) {
        first = first < 0 ? static_cast<int>(w) : first;
        last  = static_cast<int>(w);
      }
    }
    if (first < 0) {
      continue;
    }
    uint32_t word0 = static_cast<uint32_t>(words.size());
    bool     found = false;
    for (const shared& s : seen) {
      if (s.mask_offset == d.mask_offset && s.nw == nw) {
        word0 = s.word0;
        found = true;
      }
    }
    if (!found) {
      seen.push_back({d.mask_offset, nw, word0});
      uint32_t prefix = 0;
      for (uint32_t w = 0; w != nw; ++w) {
        words.push_back(precode_word{m[w], prefix, 0});
        for (uint64_t b = m[w]; b != 0; b &= b - 1U) {
          ++prefix;
        }
      }
    }
    precode_row r{};
    r.in_offset  = d.sym_offset;
    r.in_stride  = l.in_stride;
    r.out_offset = d.grid_offset;
    r.out_stride = d.port_stride;
    r.word0      = word0;
    r.weight0    = d.weight_offset;
    r.k_begin    = static_cast<uint32_t>(first) * 64U;
    r.k_end      = std::min(d.width, (static_cast<uint32_t>(last) + 1U) * 64U);
    r.prg_subc   = l.compact ? 0xffffffffU : 12U * d.prg_size;
    r.block0     = blocks;
    r.nof_layers = d.nof_layers;
    r.nof_ports  = d.nof_ports;
    blocks += (r.k_end - r.k_begin + PC_BLOCK * PC_RES - 1U) / (PC_BLOCK * PC_RES);
    rows.push_back(r);
  }
  bool ok = t.rows.size() == rows.size() && t.words.size() == words.size() && t.nblocks == blocks;
  for (size_t i = 0; ok && i != rows.size(); ++i) {
    const precode_row &a = t.rows[i], &b = rows[i];
    ok = a.in_offset == b.in_offset && a.in_stride == b.in_stride && a.out_offset == b.out_offset &&
         a.out_stride == b.out_stride && a.word0 == b.word0 && a.weight0 == b.weight0 && a.k_begin == b.k_begin &&
         a.k_end == b.k_end && a.prg_subc == b.prg_subc && a.block0 == b.block0 && a.nof_layers == b.nof_layers &&
         a.nof_ports == b.nof_ports && std::all_of(a.pad, a.pad + 6, [](uint8_t p) { return p == 0; });
  }
  for (size_t i = 0; ok && i != words.size(); ++i) {
    ok = t.words[i].bits == words[i].bits && t.words[i].prefix == words[i].prefix && t.words[i].pad == 0;
  }
  if (ok && rows.empty()) {
    ok = t.blob.empty();
  } else if (ok) {
    const size_t nwb = 4U * l.weights.size();
    ok = t.words_at == 64U * rows.size() && t.weights_at == t.words_at + 16U * words.size() &&
         t.blob.size() == t.weights_at + nwb && std::memcmp(t.blob.data(), t.rows.data(), t.words_at) == 0 &&
         std::memcmp(t.blob.data() + t.words_at, t.words.data(), 16U * words.size()) == 0 &&
         std::memcmp(t.blob.data() + t.weights_at, l.weights.data(), nwb) == 0;
  }
  if (!ok) {
    std::printf("FAIL line %d: the precoder's table differs from the plain rule\n", line);
    ++g_failed;
  }
}
#define CHECK_PC_TABLE(l) check_pc_table(l, __LINE__)

/* "precode: too many blocks in one launch" is not tested: 2^31 blocks of 256 subcarriers need gigabytes of masks. */
static void test_precoder()
{
  precode_table t;
  /* a: PRBs 1 to 4 of an 11-PRB row, PRGs 0 and 1 of size 4, 2 layers on 4 ports */
  pc_launch a;
  a.descs   = {pc_desc(132, 0, 2, 4, 2, 4)};
  a.weights = pc_weights(16);
  a.masks   = pc_mask(132, 12, 60);
  CHECK_PC_TABLE(a);
  CHECK(a.make(t) == nullptr && t.rows.size() == 1 && t.words.size() == 3 && t.nblocks == 1);
  CHECK(t.words[0].prefix == 0 && t.words[1].prefix == 48 && t.words[2].prefix == 48);
  CHECK(t.rows[0].k_begin == 0 && t.rows[0].k_end == 64 && t.rows[0].block0 == 0 && t.rows[0].prg_subc == 48);
  CHECK(t.rows[0].in_offset == 5 && t.rows[0].in_stride == 0 && t.rows[0].out_offset == 9);
  CHECK(t.rows[0].out_stride == 135 && t.rows[0].weight0 == 0 && t.rows[0].nof_layers == 2 && t.rows[0].nof_ports == 4);
  CHECK(t.words_at == 64 && t.weights_at == 64 + 48 && t.blob.size() == 64 + 48 + 128);
  /* b: the last PRB of a 273-PRB row is one block high in the grid */
  pc_launch b;
  b.descs   = {pc_desc(3276, 0, 1, 1, 69, 4)};
  b.weights = pc_weights(69);
  b.masks   = pc_mask(3276, 3264, 3276);
  CHECK_PC_TABLE(b);
  CHECK(b.make(t) == nullptr && t.words.size() == 52 && t.nblocks == 1 && t.words[51].prefix == 0);
  CHECK(t.rows[0].k_begin == 3264 && t.rows[0].k_end == 3276);
  /* c: the whole row */
  pc_launch c = b;
  c.masks     = pc_mask(3276, 0, 3276);
  CHECK_PC_TABLE(c);
  CHECK(c.make(t) == nullptr && t.nblocks == 13 && t.rows[0].k_begin == 0 && t.rows[0].k_end == 3276);
  CHECK(t.words[51].prefix == 51 * 64);
  /* d: two rows of one mask share its words; another mask's come behind them */
  pc_launch d = a;
  d.descs     = {pc_desc(132, 0, 2, 4, 2, 4), pc_desc(132, 0, 1, 2, 3, 4), pc_desc(132, 3, 2, 4, 2, 4)};
  d.descs[1].sym_offset = 1000, d.descs[1].weight_offset = 4;
  const std::vector<uint64_t> other = pc_mask(132, 70, 96);
  d.masks.insert(d.masks.end(), other.begin(), other.end());
  CHECK_PC_TABLE(d);
  CHECK(d.make(t) == nullptr && t.rows.size() == 3 && t.words.size() == 6 && t.nblocks == 3);
  CHECK(t.rows[0].word0 == 0 && t.rows[1].word0 == 0 && t.rows[2].word0 == 3 && t.rows[1].weight0 == 4);
  CHECK(t.rows[2].k_begin == 64 && t.rows[2].k_end == 128 && t.rows[2].block0 == 2);
  /* e: a row without a masked RE is dropped, and the next row's block0 continues the count */
  pc_launch e = c;
  e.descs     = {c.descs[0], pc_desc(3276, 52, 1, 1, 69, 4), c.descs[0]};
  e.masks.resize(2U * 52U, 0);
  e.descs[2].grid_offset = 1U << 20;
  CHECK_PC_TABLE(e);
  CHECK(e.make(t) == nullptr && t.rows.size() == 2 && t.nblocks == 26 && t.rows[1].block0 == 13);
  CHECK(t.rows[1].out_offset == (1U << 20) && t.rows[1].word0 == 0 && t.words.size() == 52);
  /* f: no masked RE at all: nothing to launch, whatever the weights' reach */
  pc_launch f = d;
  std::fill(f.masks.begin(), f.masks.end(), 0);
  f.descs[0].nof_prg = 1000, f.descs[1].weight_offset = 999999, f.descs[2].nof_prg = 0;
  CHECK_PC_TABLE(f);
  CHECK(f.make(t) == nullptr && t.rows.empty() && t.words.empty() && t.nblocks == 0 && t.blob.empty());
  /* g: a width of whole words has no tail to check; the last bit is the last subcarrier */
  pc_launch g;
  g.descs   = {pc_desc(64, 0, 1, 1, 2, 4)};
  g.weights = pc_weights(2);
  g.masks   = pc_mask(64, 63, 64);
  CHECK_PC_TABLE(g);
  CHECK(g.make(t) == nullptr && t.rows[0].k_begin == 0 && t.rows[0].k_end == 64 && t.nblocks == 1);
  g.descs[0].nof_prg = 1; /* subcarrier 63 is PRG 1 */
  REASON(g.make(t), R_PC_REACH);
  /* h: the compact form is one PRG whatever its length, and carries the in_stride it was given */
  pc_launch h;
  h.descs     = {pc_desc(300, 0, 2, 2, 1, 1)};
  h.weights   = pc_weights(4);
  h.masks     = pc_mask(300, 0, 300);
  h.compact   = true;
  h.in_stride = 777;
  CHECK_PC_TABLE(h);
  CHECK(h.make(t) == nullptr && t.rows[0].prg_subc == 0xffffffffU && t.rows[0].in_stride == 777 && t.nblocks == 2);
  h.descs[0].port_stride = 299; /* no port-stride check in the compact form */
  CHECK_PC_TABLE(h);
  h.compact = false;
  REASON(h.make(t), R_PC_STRIDE);

  /* weights: the largest float below 2^64 passes; 2^64, the infinities and NaN do not, as either component */
  for (const size_t at : {size_t{14}, size_t{15}}) {
    pc_launch w   = a;
    w.weights[at] = float_of(0x5F7FFFFFU);
    CHECK_PC_TABLE(w);
    w.weights[at] = -float_of(0x5F7FFFFFU);
    CHECK_PC_TABLE(w);
    for (const uint32_t bits : {0x5F800000U, 0xDF800000U, 0x7F800000U, 0xFF800000U, 0x7FC00000U}) {
      w.weights[at] = float_of(bits);
      REASON(w.make(t), R_PC_WEIGHT);
    }
  }

  /* one rejection per reason */
  const unsigned outside[][2] = {{0, 1}, {1, 0}, {2, 1}, {3, 2}, {4, 3}, {1, 5}, {5, 5}, {0, 0}};
  for (const auto& lp : outside) {
    pc_launch x           = a;
    x.descs[0].nof_layers = static_cast<uint8_t>(lp[0]);
    x.descs[0].nof_ports  = static_cast<uint8_t>(lp[1]);
    REASON(x.make(t), R_PC_TOPOLOGY);
  }
  pc_launch x = a;
  x.descs[0].prg_size = 0;
  REASON(x.make(t), R_PC_PRG);
  x = a, x.descs[0].port_stride = 131;
  REASON(x.make(t), R_PC_STRIDE);
  x = a, x.descs[0].mask_offset = 4; /* past the three words; nothing of the masks is read */
  REASON(x.make(t), R_PC_MASK);
  x = a, x.descs[0].mask_offset = 0xffffffffU;
  REASON(x.make(t), R_PC_MASK);
  x = a, x.descs[0].mask_offset = 1; /* three words from word 1 of three */
  REASON(x.make(t), R_PC_MASK);
  x = a, x.masks.pop_back();
  REASON(x.make(t), R_PC_MASK);
  x = a, x.descs[0].width = 59, x.descs[0].nof_prg = 2; /* bit 59 is the first past a width of 59 */
  REASON(x.make(t), R_PC_TAIL);
  x.descs[0].width = 60;
  CHECK_PC_TABLE(x);
  x = a, x.descs[0].nof_prg = 1; /* subcarrier 48 is PRG 1 */
  REASON(x.make(t), R_PC_REACH);
  x = a, x.descs[0].weight_offset = 17; /* past the 16 weights */
  REASON(x.make(t), R_PC_REACH);
  x = a, x.descs[0].weight_offset = 1; /* the block's end past them */
  REASON(x.make(t), R_PC_REACH);
  x = a, x.weights.resize(30);
  REASON(x.make(t), R_PC_REACH);
  /* nof_prg x layers x ports is a 64-bit product: 2^29 x 8 and (2^32 - 1) x 8 do not wrap into the array */
  x = a, x.descs[0].nof_prg = 0xffffffffU;
  REASON(x.make(t), R_PC_REACH);
  x.descs[0].nof_prg = 0x20000000U;
  REASON(x.make(t), R_PC_REACH);

  /* order: the weights; then row by row topology, prg_size, width against the stride, the mask's range, its tail,
   * and the PRG / weight reach */
  x = a;
  x.descs[0].nof_prg = 1, x.descs[0].width = 50;
  REASON(x.make(t), R_PC_TAIL);
  x.masks.pop_back(), x.masks.pop_back(), x.masks.pop_back(); /* width 50 is one word: none left */
  REASON(x.make(t), R_PC_MASK);
  x.descs[0].port_stride = 49;
  REASON(x.make(t), R_PC_STRIDE);
  x.descs[0].prg_size = 0;
  REASON(x.make(t), R_PC_PRG);
  x.descs[0].nof_ports = 1;
  REASON(x.make(t), R_PC_TOPOLOGY);
  x.weights[3] = float_of(0x7FC00000U);
  REASON(x.make(t), R_PC_WEIGHT);
  /* the first invalid row in the caller's order decides; a refused weight comes before every row, used or not */
  x = d, x.descs[1].nof_prg = 0, x.descs[2].nof_layers = 5;
  REASON(x.make(t), R_PC_REACH);
  x.descs[0].prg_size = 0;
  REASON(x.make(t), R_PC_PRG);
  x = f, x.weights.back() = float_of(0x7F800000U);
  REASON(x.make(t), R_PC_WEIGHT);
  /* no row and no weight: accepted, nothing produced */
  CHECK(make_precode_table(0, nullptr, nullptr, 0, nullptr, 0, false, 0, t) == nullptr && t.rows.empty() &&
        t.blob.empty() && t.nblocks == 0);
}

int main()
{
  CHECK(align16(0) == 0 && align16(1) == 16 && align16(16) == 16 && align16(17) == 32);
  CHECK(align16((1ULL << 32) + 1) == (1ULL << 32) + 16);
  CHECK(valid_modulation(0) && valid_modulation(8) && !valid_modulation(3) && !valid_modulation(10));
  CHECK(bits_per_symbol(0) == 1 && bits_per_symbol(1) == 1 && bits_per_symbol(6) == 6);
  CHECK(graph_slot(1, 2) == 0 && graph_slot(2, 384) == 101 && graph_slot(0, 2) == -1 && graph_slot(1, 1) == -1);
  test_decode_valid();
  test_decode_rejections();
  test_plan_order_and_equivalence();
  test_hw_config();
  test_dematch_valid();
  test_dematch_rejections();
  test_dematch_buffer_boundary();
  test_encoder();
  test_rate_matcher();
  test_pdsch();
  test_tb_join();
  test_demodulator();
  test_sequences();
  test_mapper();
  test_rate_match_mapper();
  test_equalizer();
  test_precoder();
  std::printf(g_failed == 0 ? "test_descs: all passed\n" : "test_descs: %d checks failed\n", g_failed);
  return g_failed == 0 ? 0 : 1;
}
