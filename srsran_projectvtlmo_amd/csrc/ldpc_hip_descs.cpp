/* C-ABI descriptors into kernel work items (ldpc_hip_descs.h). */
#include "ldpc_hip_descs.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

namespace ldpc_hip {

/* the C ABI's struct layouts are part of the contract (tests/test_abi.py checks the same sizes from Python) */
static_assert(sizeof(ldpc_hip_dec_desc) == 32, "ldpc_hip_dec_desc layout");
static_assert(sizeof(ldpc_hip_dematch_desc) == 20, "ldpc_hip_dematch_desc layout");
static_assert(sizeof(ldpc_hip_hw_config) == 44, "ldpc_hip_hw_config layout");
static_assert(sizeof(ldpc_hip_cb_result) == 4, "ldpc_hip_cb_result layout");
static_assert(sizeof(ldpc_hip_tb_desc) == 40, "ldpc_hip_tb_desc layout");
static_assert(sizeof(ldpc_hip_tb_result) == 4, "ldpc_hip_tb_result layout");
static_assert(sizeof(ldpc_hip_enc_desc) == 24, "ldpc_hip_enc_desc layout");
static_assert(sizeof(ldpc_hip_rm_desc) == 32, "ldpc_hip_rm_desc layout");
static_assert(sizeof(ldpc_hip_demod_desc) == 32, "ldpc_hip_demod_desc layout");
static_assert(sizeof(ldpc_hip_dmrs_pdsch_desc) == 64, "ldpc_hip_dmrs_pdsch_desc layout");
static_assert(sizeof(ldpc_hip_dmrs_pusch_desc) == 104, "ldpc_hip_dmrs_pusch_desc layout");
static_assert(sizeof(ldpc_hip_chest_result) == sizeof(chest_record), "ldpc_hip_chest_result layout");
static_assert(sizeof(ldpc_hip_chest_metrics) == 24, "ldpc_hip_chest_metrics layout");

namespace {

/* ---- pseudo-random sequence generator, host side (ldpc_hip_device.h) ----
 * x^(2^k) mod g for both registers, built at load by repeated squaring from x (the recurrences enter through the
 * reduction x^31 = x^3 + 1 / x^3 + x^2 + x + 1). A jump by n bits is one polynomial jump per set bit of n. */
struct prs_host_tables {
  uint32_t pow2[2][64];
  prs_host_tables()
  {
    for (int x = 0; x != 2; ++x) {
      uint32_t p = 2;
      for (int k = 0; k != 64; ++k) {
        pow2[x][k] = p;
        p          = prs_mulmod(p, p, x == 0 ? PRS_G1 : PRS_G2);
      }
    }
  }
};
const prs_host_tables g_prs_host;

template <bool X2>
uint32_t prs_advance(uint32_t s, uint64_t n)
{
  for (int k = 0; n != 0; ++k, n >>= 1) {
    if ((n & 1U) != 0U) {
      s = prs_jump_poly<X2>(s, g_prs_host.pow2[X2 ? 1 : 0][k]);
    }
  }
  return s;
}

/* K and the full codeword's columns of a base graph (build_graph's g.K, g.N_full) */
unsigned bg_K(int bg) { return bg == 1 ? 22U : 10U; }
unsigned bg_N_full(int bg) { return bg == 1 ? 68U : 52U; }

/* a segment's blocks onto its launch's count; more than one launch holds: `too_many` */
const char* add_blocks(uint64_t& blocks, uint64_t units, uint64_t per_block, const char* too_many)
{
  blocks += (units + per_block - 1U) / per_block;
  return blocks <= MAX_LAUNCH_BLOCKS ? nullptr : too_many;
}

/* A weight component the reference's complex multiply handles without its NaN fall-back (__mulsc3, taken only when
 * both result components are NaN): finite and below 2^64, so that no intermediate overflows (127 2^64 2 4 < FLT_MAX). */
bool weight_ok(float v) { return std::isfinite(v) && std::fabs(v) < 18446744073709551616.0F; }

} // namespace

/* Nc = 1600 bits on from the initial registers, then offset (two jumps: 1600 + offset may not fit 64 bits) */
ldpc_hip_prs_state prs_state_at(uint32_t c_init, uint64_t offset)
{
  ldpc_hip_prs_state st;
  st.x1 = prs_advance<false>(prs_advance<false>(1U, PRS_NC), offset);
  st.x2 = prs_advance<true>(prs_advance<true>(c_init & PRS_MASK, PRS_NC), offset);
  return st;
}

int graph_slot(int bg, unsigned Z)
{
  int pos = lifting_position(Z);
  if (pos < 0 || (bg != 1 && bg != 2)) {
    return -1;
  }
  return (bg - 1) * 51 + pos;
}

const char* make_dec_cb(const ldpc_hip_dec_desc& s, dec_cb& out)
{
  if (graph_slot(s.base_graph, s.lifting_size) < 0) {
    return "invalid base graph / lifting size";
  }
  const unsigned Z  = s.lifting_size;
  const unsigned KZ = bg_K(s.base_graph) * Z;
  if (s.max_iterations == 0) {
    return "Max iterations must be different to 0";
  }
  if (s.llr_length > (bg_N_full(s.base_graph) - 2U) * Z || s.llr_length < KZ + 2U * Z) {
    return "input length out of range [(K+2)Z, N_short Z]";
  }
  if (s.nof_filler_bits >= KZ) {
    return "invalid number of filler bits";
  }
  const unsigned crc_mode = s.crc_mode & ~LDPC_HIP_CRC_MODE_FLAG_KEEP_PASSED;
  if (crc_mode > LDPC_HIP_CRC_MODE_CHECK_AFTER) {
    return "invalid CRC mode";
  }
  if (crc_mode != LDPC_HIP_CRC_MODE_NONE && (s.crc_poly < 0 || s.crc_poly > 2)) {
    return "invalid CRC polynomial";
  }
  const float sf = dec_scaling(s);
  if (!(sf > 0.0f && sf < 1.0f)) {
    return "Scaling factor must be between 0 and 1 exclusively";
  }
  out                 = dec_cb{};
  out.llr_offset      = s.llr_offset;
  out.out_offset      = s.out_offset;
  out.llr_length      = s.llr_length;
  out.nof_filler_bits = s.nof_filler_bits;
  out.max_iterations  = s.max_iterations;
  out.crc_mode        = static_cast<uint8_t>(crc_mode);
  out.keep_passed     = (s.crc_mode & LDPC_HIP_CRC_MODE_FLAG_KEEP_PASSED) != 0 ? 1 : 0;
  out.crc_poly        = (crc_mode == LDPC_HIP_CRC_MODE_NONE) ? 0 : s.crc_poly;
  out.scaling_factor  = sf;
  return nullptr;
}

const char* make_dec_cbs(uint32_t n, const ldpc_hip_dec_desc* descs, std::vector<dec_cb>& cbs)
{
  std::vector<dec_cb> by_caller(n);
  for (uint32_t i = 0; i != n; ++i) {
    if (const char* why = make_dec_cb(descs[i], by_caller[i])) {
      return why;
    }
    by_caller[i].result_index = i;
  }
  /* launch groups: one kernel launch per (BG, Z, default-scaling) class */
  auto key_of = [&](const dec_cb& c) {
    const ldpc_hip_dec_desc& s = descs[c.result_index];
    return 2 * graph_slot(s.base_graph, s.lifting_size) + (c.scaling_factor == 0.8f ? 0 : 1);
  };
  std::stable_sort(by_caller.begin(), by_caller.end(),
                   [&](const dec_cb& a, const dec_cb& b) { return key_of(a) < key_of(b); });
  cbs.swap(by_caller);
  return nullptr;
}

ldpc_hip_dec_desc make_dec_desc_from_hw(const ldpc_hip_hw_config& cfg, uint32_t N, uint64_t soft_off, uint64_t out_off)
{
  ldpc_hip_dec_desc x{};
  x.base_graph      = cfg.base_graph;
  x.max_iterations  = static_cast<uint8_t>(cfg.max_nof_ldpc_iterations);
  x.crc_mode        = cfg.use_early_stop ? LDPC_HIP_CRC_MODE_EARLY_STOP : LDPC_HIP_CRC_MODE_CHECK_AFTER;
  x.crc_poly        = static_cast<int8_t>(cfg.cb_crc_type);
  x.lifting_size    = static_cast<uint16_t>(cfg.lifting_size);
  x.nof_filler_bits = static_cast<uint16_t>(cfg.nof_filler_bits);
  x.llr_length      = N;
  x.scaling_factor  = 0.8f; /* pusch_decoder default (ldpc_decoder.h:50) */
  x.llr_offset      = soft_off;
  x.out_offset      = out_off;
  return x;
}

const char* make_dematch_cb(const ldpc_hip_dematch_desc& s, const int8_t* llr, int8_t* soft,
                            const ldpc_hip_demod_desc* demod, const float* sym_base, const float* nv_base,
                            const ldpc_hip_scramble_desc* scr, const dec_cb* paired, dematch_cb& out)
{
  const unsigned Qm = s.modulation_order;
  if (s.rv > 3 || !(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8) || s.rm_length % Qm != 0) {
    return "invalid rv / modulation / rm_length";
  }
  if (s.Nref > MAX_CB_LEN || s.cb_length > MAX_CB_LEN) {
    return "N_ref / cb_length too large";
  }
  unsigned Z = 0, K = 0;
  if (s.cb_length % 66 == 0) {
    Z = s.cb_length / 66;
    K = 22;
  } else if (s.cb_length % 50 == 0) {
    Z = s.cb_length / 50;
    K = 10;
  } else {
    return "LDPC rate dematching: invalid input length.";
  }
  if (lifting_index(Z) < 0) {
    return "LDPC rate dematching: invalid input length.";
  }
  if (s.nof_filler_bits >= (K - 2) * Z) {
    return "LDPC rate dematching: invalid number of filler bits.";
  }
  /* a limited buffer covers the systematic bits in every TS 38.212 configuration; a shorter one would make the allot
   * loop's parity range (Ncb - tmp_idx after tmp_idx was raised to (K - 2) Z) wrap and write past the soft buffer.
   * Ncb == (K - 2) Z is legal: that range is empty and the loop still ends */
  if (s.Nref != 0 && std::min<unsigned>(s.Nref, s.cb_length) < (K - 2) * Z) {
    return "LDPC rate dematching: limited buffer shorter than the systematic bits.";
  }
  /* the fused dematcher writes cb_length soft bits at the decode descriptor's offset, inside the workgroup that then
   * decodes them: a length or filler mismatch would write into a neighbour's buffer while it is being decoded */
  if (paired != nullptr && (s.cb_length != paired->llr_length || s.nof_filler_bits != paired->nof_filler_bits)) {
    return "dematch_decode_launch: dematch descriptor does not match its codeblock "
           "(cb_length != llr_length or filler bits differ)";
  }
  out = dematch_cb{};
  if (demod != nullptr) {
    /* the symbols are demodulated into the dematcher's LDS staging, which holds DM_STAGE LLRs */
    if (!valid_modulation(demod->modulation) || bits_per_symbol(demod->modulation) != Qm ||
        static_cast<uint64_t>(demod->nof_symbols) * Qm != s.rm_length || s.rm_length > DM_STAGE) {
      return paired != nullptr ? "dematch_decode_launch: symbols x bits per symbol must equal rm_length <= 32768"
                               : "demod_dematch_launch: symbols x bits per symbol must equal rm_length <= 32768";
    }
    out.sym   = sym_base + 2 * demod->symbol_offset;
    out.nv    = nv_base + demod->noise_offset;
    out.demod = demod->modulation;
  } else {
    out.llr = llr;
  }
  out.soft             = soft;
  out.cb_length        = s.cb_length;
  out.rm_length        = s.rm_length;
  out.Nref             = s.Nref;
  out.nof_filler_bits  = s.nof_filler_bits;
  out.modulation_order = s.modulation_order;
  out.rv               = s.rv;
  out.new_data         = s.new_data;
  if (scr != nullptr && scr->enable != 0) {
    if (s.rm_length > DM_STAGE) {
      return "scrambled codeblock with rm_length above 32768 cannot be descrambled in the dematcher: descramble it "
             "with ldpc_hip_descramble_launch first";
    }
    const ldpc_hip_prs_state st = prs_state_at(scr->c_init, scr->seq_offset);
    out.scr_x1                  = st.x1;
    out.scr_x2                  = st.x2;
  }
  return nullptr;
}

const char* tb_desc_reason(const ldpc_hip_tb_desc& d)
{
  const unsigned C = d.nof_cbs;
  if (C == 0 || d.tbs == 0 || d.tbs % 8 != 0 || d.msg_stride < (d.cb_msg_bits + 7U) / 8U) {
    return "tb_join: invalid sizes";
  }
  if (d.cb_crc_bits != 16 && d.cb_crc_bits != 24) {
    return "tb_join: CRC length must be 16 or 24";
  }
  if (d.tbs / 8U > static_cast<uint32_t>(TBJ_CHUNK * TBJ_MAX_CHUNKS)) {
    return "tb_join: transport block too large";
  }
  if (C == 1) {
    if (d.tbs + d.cb_crc_bits + d.nof_filler_bits > d.cb_msg_bits) {
      return "tb_join: TB larger than its codeblock";
    }
  } else {
    const unsigned kd = d.cb_msg_bits - d.cb_crc_bits - d.nof_filler_bits;
    if (d.cb_crc_bits != 24 || d.cb_crc_bits + d.nof_filler_bits >= d.cb_msg_bits || d.tbs <= (C - 1U) * kd ||
        d.tbs - (C - 1U) * kd + 24U > kd) {
      return "tb_join: segmentation inconsistent with the TB size";
    }
  }
  return nullptr;
}

const char* make_enc_cb(const ldpc_hip_enc_desc& d, const uint32_t* ext, enc_cb& out)
{
  const int slot = graph_slot(d.base_graph, d.lifting_size);
  if (slot < 0) {
    return "encode_launch: invalid base graph / lifting size";
  }
  const uint32_t Z  = d.lifting_size;
  const uint32_t KZ = bg_K(d.base_graph) * Z;
  if (d.cw_length == 0 || d.cw_length > (bg_N_full(d.base_graph) - 2U) * Z) {
    return "encode_launch: codeword length out of range";
  }
  const uint32_t bit_off = ext != nullptr ? ext[0] : 0U;
  const uint32_t data    = ext != nullptr ? ext[1] : KZ;
  const uint32_t crc_at  = ext != nullptr ? ext[2] : 0U;
  if (bit_off > 7 || data > KZ || (crc_at != 0 && (crc_at + 24 > KZ || data > crc_at))) {
    return "encode_launch: message bit range out of range";
  }
  out = enc_cb{d.msg_offset, d.cw_offset, d.cw_length, slot, bit_off, data, crc_at, 0};
  return nullptr;
}

/* ldpc_rate_matcher_impl.cpp:36-160 */
const char* make_rm_cb(const ldpc_hip_rm_desc& d, ratematch_cb& out)
{
  static const uint32_t sf_bg1[4] = {0, 17, 33, 56}, sf_bg2[4] = {0, 13, 25, 43}; /* ldpc_rate_matcher_impl.cpp:33-34 */
  const unsigned        N         = d.cb_length;
  const bool            bg1       = (N % 66U) == 0;
  if (!bg1 && (N % 50U) != 0) {
    return "rate_match_launch: invalid codeblock length";
  }
  const unsigned Z = bg1 ? N / 66U : N / 50U;
  if (graph_slot(bg1 ? 1 : 2, Z) < 0 || d.rv > 3 || d.modulation_order == 0 || d.modulation_order > 8 ||
      d.rm_length == 0 || d.rm_length % d.modulation_order != 0) {
    return "rate_match_launch: invalid parameters";
  }
  const unsigned nsys = ((bg1 ? 22U : 10U) - 2U) * Z;
  if (d.nof_filler_bits >= nsys) {
    return "rate_match_launch: invalid number of filler bits";
  }
  const unsigned Ncb = (d.Nref > 0) ? std::min<unsigned>(d.Nref, N) : N;
  const uint64_t sf  = bg1 ? sf_bg1[d.rv] : sf_bg2[d.rv];
  out                = ratematch_cb{};
  out.cw_offset      = d.cw_offset;
  out.out_offset     = d.out_offset;
  out.cb_length      = N;
  out.rm_length      = d.rm_length;
  out.Ncb            = Ncb;
  out.k0             = static_cast<uint32_t>((sf * Ncb) / N) * Z; /* :88-89, floor of an exact ratio */
  out.fill_lo        = nsys - d.nof_filler_bits;
  out.fill_hi        = nsys;
  out.Qm             = d.modulation_order;
  return nullptr;
}

const char* make_pdsch_cb(const ldpc_hip_enc_desc& ed, const uint32_t* ext, const ldpc_hip_rm_desc& rd,
                          pdsch_enc_cb& out)
{
  const char* why = make_enc_cb(ed, ext, out.enc);
  if (why == nullptr) {
    why = make_rm_cb(rd, out.rm);
  }
  if (why == nullptr && (out.enc.cw_length != out.rm.cb_length ||
                         out.enc.graph_slot != graph_slot(rd.cb_length % 66U == 0 ? 1 : 2, ed.lifting_size))) {
    why = "pdsch_encode: encoder and rate matcher descriptors disagree";
  }
  return why;
}

/* ---- segment launches ---- */
const char* make_demod_seg(const ldpc_hip_demod_desc& d, uint64_t& blocks, demod_seg& out)
{
  if (!valid_modulation(d.modulation)) {
    return "demodulate: invalid modulation scheme";
  }
  out              = demod_seg{};
  out.sym_offset   = d.symbol_offset;
  out.noise_offset = d.noise_offset;
  out.llr_offset   = d.llr_offset;
  out.nof_symbols  = d.nof_symbols;
  out.block0       = static_cast<uint32_t>(blocks);
  out.modulation   = d.modulation;
  out.qm           = static_cast<uint8_t>(bits_per_symbol(d.modulation));
  return add_blocks(blocks, d.nof_symbols, DEMOD_BLOCK, "demodulate: too many symbols for one launch");
}

const char* make_prs_seg(const ldpc_hip_prs_seg& d, uint64_t& blocks, prs_seg& out, bool has_input)
{
  if ((d.c_init & ~PRS_MASK) != 0U) {
    return "pseudo-random sequence: c_init above 31 bits";
  }
  const ldpc_hip_prs_state st = prs_state_at(d.c_init, d.seq_offset);
  out                         = prs_seg{};
  out.in_offset               = has_input ? d.in_offset : PRS_NO_INPUT;
  out.out_offset              = d.out_offset;
  out.length                  = d.length;
  out.block0                  = static_cast<uint32_t>(blocks);
  out.x1                      = st.x1;
  out.x2                      = st.x2;
  return add_blocks(blocks, (static_cast<uint64_t>(d.length) + 31U) / 32U, PRS_BLOCK * PRS_WORDS,
                    "pseudo-random sequence: too many LLRs or bits for one launch");
}

const char* make_mod_seg(const ldpc_hip_mod_desc& d, uint64_t& blocks, mod_seg& out)
{
  if (!valid_modulation(d.modulation)) {
    return "modulate: invalid modulation scheme";
  }
  if (d.scramble != 0 && (d.c_init & ~PRS_MASK) != 0U) {
    return "modulate: c_init above 31 bits";
  }
  if (d.nof_symbols >= 0x80000000U) {
    /* a thread's first symbol (chunk x symbols per chunk) is 32-bit in the kernels, the last block's surplus threads
     * included */
    return "modulate: a segment holds fewer than 2^31 symbols";
  }
  const uint32_t qm = bits_per_symbol(d.modulation);
  out               = mod_seg{};
  out.bit_offset    = d.bit_offset;
  out.sym_offset    = d.symbol_offset;
  out.nof_symbols   = d.nof_symbols;
  out.block0        = static_cast<uint32_t>(blocks);
  out.modulation    = d.modulation;
  if (d.scramble != 0) {
    const ldpc_hip_prs_state st = prs_state_at(d.c_init, d.seq_offset);
    out.x1                      = st.x1;
    out.x2                      = st.x2;
  }
  const uint64_t per_chunk = mod_chunk_bits(qm) / qm;
  return add_blocks(blocks, (d.nof_symbols + per_chunk - 1U) / per_chunk, MOD_BLOCK,
                    "modulate: too many symbols for one launch");
}

const char* make_rm_mod_cb(const ldpc_hip_rm_desc& rd, const ldpc_hip_mod_desc& md, uint64_t& blocks, rm_mod_cb& out)
{
  const char* why = make_rm_cb(rd, out.rm);
  if (why == nullptr) {
    why = make_mod_seg(md, blocks, out.mod);
  }
  if (why == nullptr && md.modulation == LDPC_HIP_MOD_PI_2_BPSK) {
    why = "rate_match_modulate_launch: pi/2-BPSK is not a PDSCH scheme (a span per codeblock would restart the "
          "symbol parity): rate-match, then ldpc_hip_modulate_launch over the codeword";
  }
  if (why == nullptr && (bits_per_symbol(md.modulation) != rd.modulation_order ||
                         static_cast<uint64_t>(md.nof_symbols) * rd.modulation_order != rd.rm_length ||
                         rd.rm_length >= 0x80000000U)) {
    why = "rate_match_modulate_launch: symbols x bits per symbol must equal rm_length, the scheme's bits per symbol "
          "modulation_order";
  }
  return why;
}

const char* make_eq_seg(const ldpc_hip_eq_desc& d, uint64_t& blocks, eq_seg& out)
{
  if (!eq_supported(d.algorithm, d.nof_rx_ports, d.nof_tx_layers)) {
    return "equalize: unsupported (algorithm, rx ports, tx layers): ZF or MMSE with one layer on 1-4 ports, ZF with "
           "two layers on 2 or 4 ports";
  }
  if (!(d.tx_scaling > 0.0F)) {
    return "equalize: tx_scaling must be positive";
  }
  if (d.sym_stride < d.nof_re || d.est_stride < d.nof_re) {
    return "equalize: a plane stride below nof_re";
  }
  if (static_cast<uint64_t>(d.nof_re) * d.nof_tx_layers >= 0x80000000ULL) {
    /* a thread's first RE and its output index are 32-bit in the kernel, the last block's surplus threads included */
    return "equalize: a segment holds fewer than 2^31 outputs";
  }
  out            = eq_seg{};
  out.sym_offset = d.sym_offset;
  out.sym_stride = d.sym_stride;
  out.est_offset = d.est_offset;
  out.est_stride = d.est_stride;
  out.out_offset = d.out_offset;
  out.nof_re     = d.nof_re;
  out.block0     = static_cast<uint32_t>(blocks);
  out.tx_scaling = d.tx_scaling;
  std::copy(d.noise_var, d.noise_var + EQ_MAX_PORTS, out.noise_var);
  out.algorithm     = d.algorithm;
  out.nof_rx_ports  = d.nof_rx_ports;
  out.nof_tx_layers = d.nof_tx_layers;
  return add_blocks(blocks, d.nof_re, static_cast<uint64_t>(EQ_BLOCK) * EQ_RES,
                    "equalize: too many REs for one launch");
}

/* ---- precoder ---- */
const char* make_precode_table(uint32_t n, const ldpc_hip_precode_desc* descs, const float* weights,
                               uint32_t nof_weights, const uint64_t* masks, uint32_t nof_mask_words, bool compact,
                               uint64_t in_stride, precode_table& t)
{
  t = precode_table{};
  for (uint64_t i = 0; i != 2ULL * nof_weights; ++i) {
    if (!weight_ok(weights[i])) {
      return "precode: a weight component is not finite or is 2^64 or more in magnitude";
    }
  }
  /* a mask's words with their prefix counts, once per (first word, words) */
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
  uint64_t                                          blocks = 0;
  for (uint32_t i = 0; i != n; ++i) {
    const ldpc_hip_precode_desc& d = descs[i];
    if (!precode_supported(d.nof_layers, d.nof_ports)) {
      return "precode: unsupported topology (1 <= layers <= ports <= 4)";
    }
    if (d.prg_size == 0) {
      return "precode: prg_size must be at least 1";
    }
    if (!compact && d.width > d.port_stride) {
      return "precode: a row is wider than its port stride";
    }
    const uint32_t nw = (d.width + 63U) / 64U;
    if (d.mask_offset > nof_mask_words || nw > nof_mask_words - d.mask_offset) {
      return "precode: a row's mask lies outside the masks";
    }
    const uint64_t* m = masks + d.mask_offset;
    if (d.width % 64U != 0 && (m[nw - 1] >> (d.width % 64U)) != 0) {
      return "precode: a mask bit beyond the row's width";
    }
    uint32_t lo = nw, hi = 0;
    for (uint32_t w = 0; w != nw; ++w) {
      if (m[w] != 0) {
        lo = lo == nw ? w : lo;
        hi = w;
      }
    }
    if (lo == nw) {
      continue; /* no masked RE */
    }
    const uint32_t prg_subc = compact ? 0xffffffffU : 12U * d.prg_size;
    const uint32_t k_last   = hi * 64U + 63U - static_cast<uint32_t>(__builtin_clzll(m[hi]));
    const uint64_t wl       = static_cast<uint64_t>(d.nof_layers) * d.nof_ports;
    if (k_last / prg_subc >= d.nof_prg || d.weight_offset > nof_weights ||
        d.nof_prg * wl > nof_weights - d.weight_offset) {
      return "precode: a masked subcarrier's PRG lies outside the weight block";
    }
    auto it = seen.find({d.mask_offset, nw});
    if (it == seen.end()) {
      it = seen.emplace(std::make_pair(d.mask_offset, nw), static_cast<uint32_t>(t.words.size())).first;
      uint64_t prefix = 0;
      for (uint32_t w = 0; w != nw; ++w) {
        t.words.push_back(precode_word{m[w], static_cast<uint32_t>(prefix), 0});
        prefix += static_cast<uint64_t>(__builtin_popcountll(m[w]));
      }
    }
    precode_row r{};
    r.in_offset  = d.sym_offset;
    r.in_stride  = in_stride;
    r.out_offset = d.grid_offset;
    r.out_stride = d.port_stride;
    r.word0      = it->second;
    r.weight0    = d.weight_offset;
    r.k_begin    = lo * 64U;
    r.k_end      = std::min(d.width, (hi + 1U) * 64U);
    r.prg_subc   = prg_subc;
    r.block0     = static_cast<uint32_t>(blocks);
    r.nof_layers = d.nof_layers;
    r.nof_ports  = d.nof_ports;
    if (const char* why = add_blocks(blocks, r.k_end - r.k_begin, static_cast<uint64_t>(PC_BLOCK) * PC_RES,
                                     "precode: too many blocks in one launch")) {
      return why;
    }
    t.rows.push_back(r);
  }
  if (t.rows.empty()) {
    return nullptr; /* nothing to launch: no blocks, an empty blob */
  }
  t.nblocks    = static_cast<uint32_t>(blocks);
  t.words_at   = t.rows.size() * sizeof(precode_row);
  t.weights_at = t.words_at + t.words.size() * sizeof(precode_word);
  t.blob.resize(t.weights_at + 8U * static_cast<size_t>(nof_weights));
  std::memcpy(t.blob.data(), t.rows.data(), t.words_at);
  std::memcpy(t.blob.data() + t.words_at, t.words.data(), t.weights_at - t.words_at);
  std::memcpy(t.blob.data() + t.weights_at, weights, 8U * static_cast<size_t>(nof_weights));
  return nullptr;
}

/* ---- PDSCH DM-RS ---- */
uint32_t dmrs_c_init(uint32_t slot_index, uint32_t symbol, uint32_t scrambling_id, uint32_t n_scid)
{
  /* 2^17 times the low 14 bits of the first product is that term modulo 2^31; nothing here can wrap 64 bits for a
   * scrambling_id of 16 bits */
  const uint64_t first = (14ULL * slot_index + symbol + 1ULL) * (2ULL * scrambling_id + 1ULL);
  return static_cast<uint32_t>((((first & 0x3fffULL) << 17) + 2ULL * scrambling_id + n_scid) & PRS_MASK);
}

const char* make_dmrs_table(uint32_t n, const ldpc_hip_dmrs_pdsch_desc* descs, const float* weights,
                            uint32_t nof_weights, const uint64_t* rb_masks, uint32_t nof_mask_words, dmrs_table& t)
{
  t = dmrs_table{};
  for (uint64_t i = 0; i != 2ULL * nof_weights; ++i) {
    if (!weight_ok(weights[i])) {
      return "dmrs_pdsch: a weight component is not finite or is 2^64 or more in magnitude";
    }
  }
  /* a mask's words once per (first word, words) */
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
  std::vector<uint64_t>                             words;
  uint64_t                                          blocks = 0;
  for (uint32_t i = 0; i != n; ++i) {
    const ldpc_hip_dmrs_pdsch_desc& d = descs[i];
    if (d.type != 1 && d.type != 2) {
      return "dmrs_pdsch: the DM-RS type is 1 or 2";
    }
    if (!dmrs_supported(d.type, d.nof_layers, d.nof_ports)) {
      return "dmrs_pdsch: unsupported topology (1 <= layers <= ports <= 4)";
    }
    if (!std::isfinite(d.amplitude)) {
      return "dmrs_pdsch: the amplitude is not finite";
    }
    if (d.scrambling_id > 65535U) {
      return "dmrs_pdsch: scrambling_id above 65535";
    }
    if (d.n_scid > 1U) {
      return "dmrs_pdsch: n_scid above 1";
    }
    if (d.symbols_mask == 0) {
      return "dmrs_pdsch: an empty symbol mask";
    }
    if ((d.symbols_mask >> DMRS_NSYMB) != 0) {
      return "dmrs_pdsch: a symbol-mask bit at or above 14";
    }
    if (12ULL * d.nof_rb > d.width) {
      return "dmrs_pdsch: 12 nof_rb above the row's width";
    }
    if (d.width > d.symbol_stride) {
      return "dmrs_pdsch: a row is wider than its symbol stride";
    }
    const uint32_t l_last = 31U - static_cast<uint32_t>(__builtin_clz(d.symbols_mask));
    /* (a symbol stride whose 14 symbols would wrap 64 bits is above every port stride) */
    if (d.symbol_stride > (~0ULL - d.width) / DMRS_NSYMB || l_last * d.symbol_stride + d.width > d.port_stride) {
      return "dmrs_pdsch: the DM-RS symbols are wider than the port stride";
    }
    const uint32_t nw = (d.nof_rb + 63U) / 64U;
    if (d.mask_offset > nof_mask_words || nw > nof_mask_words - d.mask_offset) {
      return "dmrs_pdsch: an RB mask lies outside the masks";
    }
    const uint64_t* m = rb_masks + d.mask_offset;
    if (d.nof_rb % 64U != 0 && (m[nw - 1] >> (d.nof_rb % 64U)) != 0) {
      return "dmrs_pdsch: an RB-mask bit beyond nof_rb";
    }
    if (d.weight_offset > nof_weights ||
        static_cast<uint32_t>(d.nof_layers) * d.nof_ports > nof_weights - d.weight_offset) {
      return "dmrs_pdsch: a weight matrix lies outside the weights";
    }
    uint32_t lo = nw, hi = 0;
    for (uint32_t w = 0; w != nw; ++w) {
      if (m[w] != 0) {
        lo = lo == nw ? w : lo;
        hi = w;
      }
    }
    if (lo == nw) {
      continue; /* no allocated RB */
    }
    const uint32_t rb_begin = lo * 64U + static_cast<uint32_t>(__builtin_ctzll(m[lo]));
    const uint32_t rb_end   = hi * 64U + 64U - static_cast<uint32_t>(__builtin_clzll(m[hi]));
    if (rb_begin < d.reference_point_k_rb) {
      return "dmrs_pdsch: an allocated RB below reference_point_k_rb";
    }
    auto it = seen.find({d.mask_offset, nw});
    if (it == seen.end()) {
      it = seen.emplace(std::make_pair(d.mask_offset, nw), static_cast<uint32_t>(words.size())).first;
      words.insert(words.end(), m, m + nw);
    }
    const float* w00 = weights + 2ULL * d.weight_offset;
    dmrs_row     r{};
    r.out_stride = d.port_stride;
    /* dmrs_pdsch_processor_impl.cpp:89: M_SQRT1_2 times the amplitude in double, rounded once */
    r.a          = static_cast<float>(0.70710678118654752440 * static_cast<double>(d.amplitude));
    r.word0      = it->second;
    r.weight0    = d.weight_offset;
    r.rb_begin   = rb_begin;
    r.rb_end     = rb_end;
    r.ref_rb     = d.reference_point_k_rb;
    r.type       = d.type;
    r.nof_layers = d.nof_layers;
    r.nof_ports  = d.nof_ports;
    /* resource_grid_mapper_impl.cpp:94-95, 230-231: cf_t == 1.0F, so an imaginary part of -0 passes too */
    r.bypass = d.nof_layers == 1 && d.nof_ports == 1 && w00[0] == 1.0F && w00[1] == 0.0F ? 1 : 0;
    for (uint32_t l = 0; l != DMRS_NSYMB; ++l) {
      if (((d.symbols_mask >> l) & 1U) == 0) {
        continue;
      }
      const ldpc_hip_prs_state st = prs_state_at(dmrs_c_init(d.slot_index, l, d.scrambling_id, d.n_scid), 0);
      r.out_offset                = d.grid_offset + l * d.symbol_stride;
      r.x1                        = st.x1;
      r.x2                        = st.x2;
      r.block0                    = static_cast<uint32_t>(blocks);
      if (const char* why = add_blocks(blocks, rb_end - rb_begin, static_cast<uint64_t>(DMRS_BLOCK) * DMRS_RBS,
                                       "dmrs_pdsch: too many blocks in one launch")) {
        return why;
      }
      t.rows.push_back(r);
    }
  }
  if (t.rows.empty()) {
    return nullptr; /* nothing to launch: no blocks, an empty blob */
  }
  t.nblocks    = static_cast<uint32_t>(blocks);
  t.words_at   = t.rows.size() * sizeof(dmrs_row);
  t.weights_at = t.words_at + words.size() * sizeof(uint64_t);
  t.blob.resize(t.weights_at + 8U * static_cast<size_t>(nof_weights));
  std::memcpy(t.blob.data(), t.rows.data(), t.words_at);
  std::memcpy(t.blob.data() + t.words_at, words.data(), t.weights_at - t.words_at);
  std::memcpy(t.blob.data() + t.weights_at, weights, 8U * static_cast<size_t>(nof_weights));
  return nullptr;
}

/* ---- PUSCH DM-RS channel estimator ---- */
namespace {
/* RC_FILTER (port_channel_estimator_average_impl.cpp:42-47): raised cosine, roll-off 0.2, 3 symbols, 10 samples each */
constexpr float CHEST_RC[31] = {-0.0641253F, -0.0660711F, -0.0611526F, -0.0485918F, -0.0281126F, 0.0000000F,  0.0348830F,
                                0.0751249F,  0.1188406F,  0.1637874F,  0.2075139F,  0.2475302F,  0.2814857F,  0.3073415F,
                                0.3235207F,  0.3290274F,  0.3235207F,  0.3073415F,  0.2814857F,  0.2475302F,  0.2075139F,
                                0.1637874F,  0.1188406F,  0.0751249F,  0.0348830F,  0.0000000F,  -0.0281126F, -0.0485918F,
                                -0.0611526F, -0.0660711F, -0.0641253F};
} // namespace

uint32_t chest_filter(uint32_t nof_rb, float* taps)
{
  const uint32_t stride = 2;
  nof_rb                = std::min(nof_rb, 3U);
  const uint32_t half   = (nof_rb * 10U + 1U) / 2U / stride;
  const uint32_t ntaps  = 2U * half + 1U;
  uint32_t       n      = 31U / 2U - half * stride;
  float          total  = 0;
  for (uint32_t i = 0; i != ntaps; ++i, n += stride) {
    taps[i] = CHEST_RC[n];
    total += taps[i];
  }
  const float h = 1 / total;
  for (uint32_t i = 0; i != CHEST_MAX_TAPS; ++i) {
    taps[i] = i < ntaps ? taps[i] * h : 0.0F;
  }
  return ntaps;
}

uint32_t chest_virtual_pilots(uint32_t nof_rb)
{
  float taps[CHEST_MAX_TAPS];
  return nof_rb == 1 ? CHEST_DPR : std::min(CHEST_MAX_VPILOTS, chest_filter(nof_rb, taps) / 2U);
}

const char* make_chest_table(uint32_t n, const ldpc_hip_dmrs_pusch_desc* descs, const uint64_t* rb_masks,
                             uint32_t nof_mask_words, chest_table& t)
{
  t = chest_table{};
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
  std::vector<uint64_t>                             words;
  for (uint32_t i = 0; i != n; ++i) {
    const ldpc_hip_dmrs_pusch_desc& d = descs[i];
    if (d.type != 1) {
      return "dmrs_pusch: only DM-RS type 1";
    }
    if (d.nof_layers < 1 || d.nof_layers > CHEST_MAX_LAYERS || d.nof_rx_ports < 1 ||
        d.nof_rx_ports > CHEST_MAX_PORTS) {
      return "dmrs_pusch: unsupported topology (1 to 4 layers on 1 to 4 receive ports)";
    }
    if (d.strategy != LDPC_HIP_CHEST_NONE && d.strategy != LDPC_HIP_CHEST_FILTER) {
      return "dmrs_pusch: the smoothing strategy is LDPC_HIP_CHEST_NONE or LDPC_HIP_CHEST_FILTER";
    }
    if (d.compensate_cfo != 0) {
      return "dmrs_pusch: CFO compensation is not supported";
    }
    if (!(d.scaling > 0.0F) || !std::isfinite(d.scaling)) {
      return "dmrs_pusch: the scaling is not positive or not finite";
    }
    if (d.scrambling_id > 65535U) {
      return "dmrs_pusch: scrambling_id above 65535";
    }
    if (d.n_scid > 1U) {
      return "dmrs_pusch: n_scid above 1";
    }
    if (d.nof_symbols == 0 || static_cast<uint32_t>(d.first_symbol) + d.nof_symbols > CHEST_NSYMB) {
      return "dmrs_pusch: the symbol range is empty or passes symbol 14";
    }
    if (d.symbols_mask == 0) {
      return "dmrs_pusch: an empty symbol mask";
    }
    const uint32_t range = ((1U << d.nof_symbols) - 1U) << d.first_symbol;
    if ((d.symbols_mask & ~range) != 0) {
      return "dmrs_pusch: a DM-RS symbol outside the symbol range";
    }
    const uint32_t nsym = static_cast<uint32_t>(__builtin_popcount(d.symbols_mask));
    if (nsym > CHEST_MAX_DMRS) {
      return "dmrs_pusch: more than 4 DM-RS symbols";
    }
    if (d.nof_rb > CHEST_MAX_RB) {
      return "dmrs_pusch: nof_rb above 275";
    }
    if (12ULL * d.nof_rb > d.width) {
      return "dmrs_pusch: 12 nof_rb above the row's width";
    }
    if (d.width > d.grid_symbol_stride || d.width > d.symbol_stride) {
      return "dmrs_pusch: a row is wider than a symbol stride";
    }
    /* no base, plane or row can then wrap 64 bits: at most 16 planes, 4 ports, 14 symbols and 6 x 275 pilots a plane */
    for (uint64_t v : {d.grid_offset, d.grid_symbol_stride, d.grid_port_stride, d.est_offset, d.symbol_stride,
                       d.plane_stride, d.pilots_offset}) {
      if (v >= (1ULL << 48)) {
        return "dmrs_pusch: an offset or stride of 2^48 elements or more";
      }
    }
    const uint32_t l_dmrs = 31U - static_cast<uint32_t>(__builtin_clz(d.symbols_mask));
    if (d.grid_symbol_stride > (~0ULL - d.width) / CHEST_NSYMB ||
        l_dmrs * d.grid_symbol_stride + d.width > d.grid_port_stride) {
      return "dmrs_pusch: the DM-RS symbols are wider than the grid's port stride";
    }
    const uint32_t l_last = static_cast<uint32_t>(d.first_symbol) + d.nof_symbols - 1U;
    if (d.symbol_stride > (~0ULL - d.width) / CHEST_NSYMB || l_last * d.symbol_stride + d.width > d.plane_stride) {
      return "dmrs_pusch: the symbol range is wider than the plane stride";
    }
    for (uint32_t p = 0; p != d.nof_rx_ports; ++p) {
      if (d.rx_ports[p] >= d.grid_ports) {
        return "dmrs_pusch: an rx port at or above the grid's ports";
      }
    }
    const uint32_t nw = (d.nof_rb + 63U) / 64U;
    if (d.mask_offset > nof_mask_words || nw > nof_mask_words - d.mask_offset) {
      return "dmrs_pusch: an RB mask lies outside the masks";
    }
    const uint64_t* m = rb_masks + d.mask_offset;
    if (d.nof_rb % 64U != 0 && (m[nw - 1] >> (d.nof_rb % 64U)) != 0) {
      return "dmrs_pusch: an RB-mask bit beyond nof_rb";
    }
    uint32_t lo = nw, hi = 0, count = 0;
    for (uint32_t w = 0; w != nw; ++w) {
      if (m[w] != 0) {
        lo = lo == nw ? w : lo;
        hi = w;
        count += static_cast<uint32_t>(__builtin_popcountll(m[w]));
      }
    }
    if (lo == nw) {
      continue; /* no allocated RB */
    }
    auto it = seen.find({d.mask_offset, nw});
    if (it == seen.end()) {
      it = seen.emplace(std::make_pair(d.mask_offset, nw), static_cast<uint32_t>(words.size())).first;
      words.insert(words.end(), m, m + nw);
    }
    chest_plane r{};
    r.grid_sym_stride = d.grid_symbol_stride;
    r.est_sym_stride  = d.symbol_stride;
    r.word0           = it->second;
    r.rb_begin        = lo * 64U + static_cast<uint32_t>(__builtin_ctzll(m[lo]));
    r.rb_end          = hi * 64U + 64U - static_cast<uint32_t>(__builtin_clzll(m[hi]));
    r.n_rb            = count;
    r.nsym            = static_cast<uint8_t>(nsym);
    for (uint32_t l = 0, s = 0; l != CHEST_NSYMB; ++l) {
      if (((d.symbols_mask >> l) & 1U) != 0) {
        /* the sequence of the symbol from its first used bit: RB rb_begin's pilot 0 */
        const ldpc_hip_prs_state st =
            prs_state_at(dmrs_c_init(d.slot_index, l, d.scrambling_id, d.n_scid), 2ULL * CHEST_DPR * r.rb_begin);
        r.x1[s]       = st.x1;
        r.x2[s]       = st.x2;
        r.dmrs_sym[s] = static_cast<uint8_t>(l);
        ++s;
      }
    }
    /* port_channel_estimator_average_impl.cpp:334-335 */
    r.total_scaling = 1.0F / (static_cast<float>(nsym) * d.scaling);
    r.beta          = d.scaling;
    r.first_symbol  = d.first_symbol;
    r.nof_symbols   = d.nof_symbols;
    r.filter        = CHEST_NO_FILTER;
    if (d.strategy == LDPC_HIP_CHEST_FILTER) {
      float taps[CHEST_MAX_TAPS];
      r.filter = static_cast<uint8_t>(std::min(count, CHEST_NOF_FILTERS) - 1U);
      r.ntaps  = static_cast<uint8_t>(chest_filter(count, taps));
      r.nvp    = static_cast<uint8_t>(chest_virtual_pilots(count));
    }
    r.wide = d.symbol_stride % 4U == 0 ? 1 : 0;
    for (uint32_t layer = 0; layer != d.nof_layers; ++layer) {
      for (uint32_t p = 0; p != d.nof_rx_ports; ++p) {
        const uint64_t plane = static_cast<uint64_t>(layer) * d.nof_rx_ports + p;
        chest_plane    q     = r;
        q.grid_base          = d.grid_offset + d.rx_ports[p] * d.grid_port_stride;
        q.est_base           = d.est_offset + plane * d.plane_stride;
        q.pil_base           = d.pilots_offset + plane * CHEST_DPR * count;
        q.res_index          = d.result_offset + static_cast<uint32_t>(plane);
        q.layer              = static_cast<uint8_t>(layer);
        q.wide               = r.wide != 0 && q.est_base % 4U == 0 ? 1 : 0;
        q.block0             = static_cast<uint32_t>(t.planes.size());
        if (t.planes.size() >= MAX_LAUNCH_BLOCKS) {
          return "dmrs_pusch: too many planes in one launch";
        }
        t.planes.push_back(q);
      }
    }
  }
  if (t.planes.empty()) {
    return nullptr; /* nothing to launch: an empty blob */
  }
  t.words_at   = t.planes.size() * sizeof(chest_plane);
  t.filters_at = t.words_at + words.size() * sizeof(uint64_t);
  float filters[CHEST_NOF_FILTERS][CHEST_TAP_STRIDE] = {};
  for (uint32_t f = 0; f != CHEST_NOF_FILTERS; ++f) {
    chest_filter(f + 1U, filters[f]);
  }
  t.blob.resize(t.filters_at + sizeof(filters));
  std::memcpy(t.blob.data(), t.planes.data(), t.words_at);
  std::memcpy(t.blob.data() + t.words_at, words.data(), t.filters_at - t.words_at);
  std::memcpy(t.blob.data() + t.filters_at, filters, sizeof(filters));
  return nullptr;
}

const char* chest_finalize(const ldpc_hip_chest_result& r, float scaling, uint32_t nsym, uint32_t l0, uint32_t l1,
                           uint32_t scs, ldpc_hip_chest_metrics& out)
{
  if (nsym < 1 || nsym > CHEST_MAX_DMRS || l0 >= CHEST_NSYMB || scs > 4 || !(scaling > 0.0F) || r.nof_pilots == 0) {
    return "dmrs_pusch_finalize: an argument outside its range";
  }
  if (nsym > 1 && (l1 >= CHEST_NSYMB || l1 <= l0)) {
    return "dmrs_pusch_finalize: the second DM-RS symbol is not after the first inside the slot";
  }
  out = ldpc_hip_chest_metrics{};
  const float    n      = static_cast<float>(r.nof_pilots);
  const unsigned pilots = r.nof_pilots * nsym;
  const unsigned khz    = 15U << scs;
  /* :357, then :257-281 */
  float rsrp = 0;
  rsrp += r.filt_power / n * n * scaling * scaling * static_cast<float>(nsym);
  float epre = 0;
  epre += r.epre_sum;
  float noise_var = 0;
  noise_var += r.noise_sum;
  rsrp /= static_cast<float>(pilots);
  epre /= static_cast<float>(pilots);
  noise_var /= static_cast<float>(pilots - 1U);
  const float min_noise_variance = rsrp / std::pow(10.0F, 100.0F / 10.0F);
  noise_var                      = std::max(min_noise_variance, noise_var);
  const float datarp             = rsrp / scaling / scaling;
  out.epre                       = epre;
  out.rsrp                       = rsrp;
  out.noise_var                  = noise_var;
  out.snr                        = (noise_var != 0) ? datarp / noise_var : 1000;
  if (nsym > 1) {
    /* :454-465: the symbols' start epochs in units of the symbol time, accumulated in float32 */
    const double t_c = 1.0 / static_cast<double>(480000LL * 4096LL);
    float        epochs[CHEST_NSYMB];
    for (uint32_t i = 0; i != CHEST_NSYMB; ++i) {
      const unsigned cp_len = (144U >> scs) + ((i == 0 || i == 7U * (1U << scs)) ? 16U : 0U);
      const double   sec    = static_cast<double>(static_cast<int64_t>(cp_len) * 64) * t_c;
      epochs[i] =
          i == 0 ? static_cast<float>(sec * khz * 1000) : static_cast<float>(epochs[i - 1] + sec * khz * 1000 + 1.0F);
    }
    const float twopi       = 2.0F * static_cast<float>(M_PI);
    const float noisy_phase = std::atan2(r.dot_im, r.dot_re);
    const float cfo         = noisy_phase / twopi / (epochs[l1] - epochs[l0]);
    out.cfo_Hz              = cfo * khz * 1000;
    out.has_cfo             = 1;
  }
  return nullptr;
}

} // namespace ldpc_hip
