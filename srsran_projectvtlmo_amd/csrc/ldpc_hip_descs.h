/*
 * The one translation of each C-ABI descriptor (include/srsran_ldpc_hip.h) into the work item the kernels read
 * (ldpc_hip_device.h, ldpc_equalize.h, ldpc_precode.h, ldpc_dmrs.h, ldpc_chest.h), with its validation, the segment
 * launches' and the precoder's, the DM-RS generator's and the channel estimator's tables included. Host only: no HIP
 * runtime call, no context. Each make_* returns the reason its descriptor is invalid, or nullptr after filling the work
 * item; the entry points report the reason through ldpc_hip_last_error with LDPC_HIP_EINVAL.
 */
#pragma once

#include <cstdint>
#include <vector>

#include "ldpc_chest.h"
#include "ldpc_dmrs.h"
#include "ldpc_equalize.h"
#include "ldpc_graph.h"
#include "ldpc_precode.h"

namespace ldpc_hip {

constexpr uint32_t MAX_CB_LEN = 66U * 384U; /* MAX_CODEBLOCK_SIZE (ldpc.h:113) */

constexpr uint64_t align16(uint64_t x) { return (x + 15U) & ~static_cast<uint64_t>(15U); }

inline bool     valid_modulation(int m) { return m == 0 || m == 1 || m == 2 || m == 4 || m == 6 || m == 8; }
inline unsigned bits_per_symbol(int m) { return (m == 0 || m == 1) ? 1U : static_cast<unsigned>(m); }
inline unsigned msg_bytes_of(int bg, unsigned Z) { return ((bg == 1 ? 22U : 10U) * Z + 7U) / 8U; }

/* the wide schedule's graph slot of (bg, Z): BG1 then BG2, by lifting position; -1 for an invalid pair */
int graph_slot(int bg, unsigned Z);

/* the generator's state `offset` bits into the sequence of c_init (ldpc_hip_prs_init) */
ldpc_hip_prs_state prs_state_at(uint32_t c_init, uint64_t offset);

/* the scaling factor a decode descriptor asks for: 0 is the default, 0.8 (ldpc_decoder.h:50) */
inline float dec_scaling(const ldpc_hip_dec_desc& d) { return d.scaling_factor == 0.0f ? 0.8f : d.scaling_factor; }

/* ---- decoder ---- */
/* one decode work item (result_index 0) */
const char* make_dec_cb(const ldpc_hip_dec_desc& s, dec_cb& out);
/* A plan's work items in launch order: every descriptor validated, then grouped by (BG, Z, default scaling or not)
 * with the caller's order kept inside a group; cbs[i].result_index is the caller's index of block i. */
const char* make_dec_cbs(uint32_t n, const ldpc_hip_dec_desc* descs, std::vector<dec_cb>& cbs);
/* the decode a HAL operation configures (hw_accelerator_pusch_dec::configure_operation): N soft bits at soft_off, the
 * message at out_off, early stop or a CRC check after the last iteration, the default scaling factor */
ldpc_hip_dec_desc make_dec_desc_from_hw(const ldpc_hip_hw_config& cfg, uint32_t N, uint64_t soft_off, uint64_t out_off);

/* ---- rate dematcher ---- */
/* One dematch work item reading llr (or, with demod, soft-demodulating its symbols from sym_base / nv_base) and
 * combining into soft; scr (may be null, or disabled) descrambles in the dematcher. paired: the decode work item whose
 * workgroup runs this dematcher first (the fused launch), which must agree in length and filler bits; it also names
 * the entry point in the demodulator's rejection. Pointers may be null and set later. */
const char* make_dematch_cb(const ldpc_hip_dematch_desc& s, const int8_t* llr, int8_t* soft,
                            const ldpc_hip_demod_desc* demod, const float* sym_base, const float* nv_base,
                            const ldpc_hip_scramble_desc* scr, const dec_cb* paired, dematch_cb& out);

/* ---- transport-block join ---- */
const char* tb_desc_reason(const ldpc_hip_tb_desc& d);

/* ---- encoder, rate matcher, the PDSCH queue's fused pair ---- */
/* ext: message bit offset (< 8), data bits (<= K Z) and CRC24B position (0: none); nullptr: K Z bits from bit 0 */
const char* make_enc_cb(const ldpc_hip_enc_desc& d, const uint32_t* ext, enc_cb& out);
const char* make_rm_cb(const ldpc_hip_rm_desc& d, ratematch_cb& out);
const char* make_pdsch_cb(const ldpc_hip_enc_desc& ed, const uint32_t* ext, const ldpc_hip_rm_desc& rd,
                          pdsch_enc_cb& out);

/* ---- segment launches: demodulator, pseudo-random sequences (has_input false, the scrambler generating: in_offset
 * is PRS_NO_INPUT), modulation mapper, equalizer ---- An item's block0 is `blocks`, its launch's count so far, which
 * the translation advances by the segment's blocks and refuses above MAX_LAUNCH_BLOCKS (a grid's 32-bit x). */
constexpr uint64_t MAX_LAUNCH_BLOCKS = 0x7fffffffULL;
const char* make_demod_seg(const ldpc_hip_demod_desc& d, uint64_t& blocks, demod_seg& out);
const char* make_prs_seg(const ldpc_hip_prs_seg& d, uint64_t& blocks, prs_seg& out, bool has_input);
const char* make_mod_seg(const ldpc_hip_mod_desc& d, uint64_t& blocks, mod_seg& out);
const char* make_eq_seg(const ldpc_hip_eq_desc& d, uint64_t& blocks, eq_seg& out);
/* the fused launch's codeblock: make_rm_cb, make_mod_seg, then that the pair agrees */
const char* make_rm_mod_cb(const ldpc_hip_rm_desc& rd, const ldpc_hip_mod_desc& md, uint64_t& blocks, rm_mod_cb& out);
/* A launch's segments through make(descriptor, blocks, item, more...): every descriptor validated in the caller's
 * order, a segment that takes no block (zero length) then dropped; nblocks is the launch's grid. */
template <typename D, typename G, typename Make, typename... More>
const char* make_segs(uint32_t n, const D* descs, std::vector<G>& segs, uint32_t& nblocks, Make make, More... more)
{
  segs.clear();
  segs.reserve(n);
  uint64_t blocks = 0;
  for (uint32_t i = 0; i != n; ++i) {
    G              g;
    const uint64_t before = blocks;
    if (const char* why = make(descs[i], blocks, g, more...)) {
      return why;
    }
    if (blocks != before) {
      segs.push_back(g);
    }
  }
  nblocks = static_cast<uint32_t>(blocks);
  return nullptr;
}

/* ---- precoder ---- */
/* a launch's table: rows, then mask words, then weights (16-byte aligned each), and the three as the launch uploads
 * them: blob[0, words_at) the rows, [words_at, weights_at) the words, then 8 bytes per weight */
struct precode_table {
  std::vector<precode_row>  rows;
  std::vector<precode_word> words;
  uint32_t                  nblocks = 0;
  std::vector<uint8_t>      blob;
  size_t                    words_at = 0, weights_at = 0;
};
/* A launch's rows: the weights validated first, then every row in the caller's order (topology, prg_size, width against
 * the port stride, the mask's words inside `masks`, no bit at or past the width, and, for a row with a masked RE, its
 * last masked subcarrier's PRG and its weight block inside `weights`). A mask's words are stored once per (mask_offset,
 * words) with the set bits before each; a row without a masked RE is dropped, one with works on [k_begin, k_end), its
 * non-zero words, from block0. No row left: no blocks and an empty blob, whatever the weights.
 * compact: the rows are a channel_precoder call's, one PRG whatever its length and no port-stride check; in_stride is
 * every row's (the compact cf32 input's layer planes; the ci8 forms do not read it). */
const char* make_precode_table(uint32_t n, const ldpc_hip_precode_desc* descs, const float* weights,
                               uint32_t nof_weights, const uint64_t* masks, uint32_t nof_mask_words, bool compact,
                               uint64_t in_stride, precode_table& t);

/* ---- PDSCH DM-RS ---- */
/* c_init of a DM-RS symbol (dmrs_pdsch_processor_impl.cpp:98), on the exact integer */
uint32_t dmrs_c_init(uint32_t slot_index, uint32_t symbol, uint32_t scrambling_id, uint32_t n_scid);
/* a launch's table: rows, then RB-mask words, then weights, and the three as the launch uploads them: blob[0, words_at)
 * the rows, [words_at, weights_at) the words (8 bytes each), then 8 bytes per weight */
struct dmrs_table {
  std::vector<dmrs_row> rows;
  uint32_t              nblocks = 0;
  std::vector<uint8_t>  blob;
  size_t                words_at = 0, weights_at = 0;
};
/* A launch's rows: the weights validated first, then every transmission in the caller's order (type and topology,
 * amplitude, scrambling_id and n_scid, the symbol mask, 12 nof_rb against the width, the width against the symbol
 * stride and the last DM-RS symbol's row against the port stride, the RB mask's words inside `rb_masks` with no bit at
 * or past nof_rb, no allocated RB below the reference point, the weight matrix inside `weights`). A transmission with
 * an empty RB mask is dropped; one with a set RB becomes one row per DM-RS symbol, on its lowest to its highest set
 * RB, from block0. No row left: no blocks and an empty blob. */
const char* make_dmrs_table(uint32_t n, const ldpc_hip_dmrs_pdsch_desc* descs, const float* weights,
                            uint32_t nof_weights, const uint64_t* rb_masks, uint32_t nof_mask_words, dmrs_table& t);

/* ---- PUSCH DM-RS channel estimator ---- */
/* The raised-cosine filter of port_channel_estimator_average_impl.cpp:74-101 for nof_rb RBs at stride 2: its taps
 * (5, 11 or 15, normalised as the reference does, in float32) into taps[0 .. CHEST_MAX_TAPS); returns their number. */
uint32_t chest_filter(uint32_t nof_rb, float* taps);
/* the virtual pilots per side (port_channel_estimator_average_impl.cpp:629-632) */
uint32_t chest_virtual_pilots(uint32_t nof_rb);
/* a launch's table: planes, then RB-mask words, then the three filters, and the three as the launch uploads them:
 * blob[0, words_at) the planes, [words_at, filters_at) the words (8 bytes each), then CHEST_NOF_FILTERS rows of
 * CHEST_TAP_STRIDE floats */
struct chest_table {
  std::vector<chest_plane> planes;
  std::vector<uint8_t>     blob;
  size_t                   words_at = 0, filters_at = 0;
};
/* A launch's planes: every transmission in the caller's order (type, topology, strategy and compensate_cfo, scaling,
 * scrambling_id and n_scid, the symbol range, the symbols mask inside it with 1 to 4 bits, nof_rb, 12 nof_rb against
 * the width, the width against both symbol strides, the last DM-RS symbol's row against the grid's port stride and the
 * range's last row against the plane stride, the rx ports against grid_ports, the RB mask's words inside `rb_masks`
 * with no bit at or past nof_rb). A transmission with an empty RB mask is dropped; another becomes one plane per
 * (layer, rx port), layer-major, its generator states at the first allocated RB. No plane left: an empty blob. */
const char* make_chest_table(uint32_t n, const ldpc_hip_dmrs_pusch_desc* descs, const uint64_t* rb_masks,
                             uint32_t nof_mask_words, chest_table& t);
/* port_channel_estimator_average_impl.cpp:257-281, 454-465, 495-497 on a plane's raw sums; nullptr or the reason */
const char* chest_finalize(const ldpc_hip_chest_result& r, float scaling, uint32_t nsym, uint32_t l0, uint32_t l1,
                           uint32_t scs, ldpc_hip_chest_metrics& out);

} // namespace ldpc_hip
