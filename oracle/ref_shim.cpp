/*
 * C interface to the reference implementation itself -- TEST INFRASTRUCTURE ONLY.
 *
 * This file holds no reference text: it includes the reference tree's headers at build time (oracle/Makefile, target
 * `ref`) and forwards plain C arguments to the reference's own generic (non-SIMD) classes, one fresh object per call.
 * The call shapes mirror ldpc_oracle.h so that oracle/ref.py can stand in for the oracle's Python functions.
 *
 * The reference asserts its contracts (ASSERTS_ENABLED): a violation ends the process. Callers keep LLRs in
 * [-120, 120] or +-127, lengths legal and 0 < scaling factor < 1.
 */
#include "crc_calculator_generic_impl.h"
#include "demodulation_mapper_impl.h"
#include "ldpc/ldpc_decoder_generic.h"
#include "ldpc/ldpc_encoder_generic.h"
#include "ldpc/ldpc_rate_dematcher_impl.h"
#include "ldpc/ldpc_rate_matcher_impl.h"
#include "pseudo_random_generator_impl.h"
#include "srsran/phy/upper/log_likelihood_ratio.h"
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

using namespace srsran;

static_assert(sizeof(log_likelihood_ratio) == 1, "LLR spans are views of int8 arrays");

namespace {

span<const log_likelihood_ratio> llr_in(const int8_t* p, unsigned n)
{
  return {reinterpret_cast<const log_likelihood_ratio*>(p), n};
}

span<log_likelihood_ratio> llr_out(int8_t* p, unsigned n)
{
  return {reinterpret_cast<log_likelihood_ratio*>(p), n};
}

modulation_scheme mod_of_qm(unsigned Qm)
{
  return Qm == 1 ? modulation_scheme::BPSK : static_cast<modulation_scheme>(Qm);
}

codeblock_metadata
metadata(int bg, unsigned Z, unsigned rv, unsigned Qm, unsigned Nref, unsigned F, unsigned nof_crc_bits)
{
  codeblock_metadata m;
  m.tb_common.base_graph        = bg == 1 ? ldpc_base_graph_type::BG1 : ldpc_base_graph_type::BG2;
  m.tb_common.lifting_size      = static_cast<ldpc::lifting_size_t>(Z);
  m.tb_common.rv                = rv;
  m.tb_common.mod               = mod_of_qm(Qm);
  m.tb_common.Nref              = Nref;
  m.cb_specific.nof_filler_bits = F;
  m.cb_specific.nof_crc_bits    = nof_crc_bits;
  return m;
}

} // namespace

extern "C" {

/* ldpc_decoder_generic::decode. crc_poly < 0: no CRC calculator. Returns iterations, 0 for std::nullopt. */
int ref_ldpc_decode(int           bg,
                    unsigned      Z,
                    unsigned      F,
                    const int8_t* llr,
                    unsigned      llr_len,
                    unsigned      max_iterations,
                    float         scaling_factor,
                    int           crc_poly,
                    uint8_t*      out_packed)
{
  auto                        dec = std::make_unique<ldpc_decoder_generic>();
  ldpc_decoder::configuration cfg;
  cfg.block_conf = metadata(bg, Z, 0, 1, 0, F, crc_poly == static_cast<int>(crc_generator_poly::CRC16) ? 16 : 24);
  cfg.algorithm_conf.max_iterations = max_iterations;
  cfg.algorithm_conf.scaling_factor = scaling_factor;
  unsigned                                     nbits = (bg == 1 ? 22 : 10) * Z;
  bit_buffer                                   out   = bit_buffer::from_bytes({out_packed, (nbits + 7) / 8}).first(nbits);
  std::unique_ptr<crc_calculator_generic_impl> crc;
  if (crc_poly >= 0) {
    crc = std::make_unique<crc_calculator_generic_impl>(static_cast<crc_generator_poly>(crc_poly));
  }
  std::optional<unsigned> r = dec->decode(out, llr_in(llr, llr_len), crc.get(), cfg);
  return r.has_value() ? static_cast<int>(*r) : 0;
}

/* ldpc_rate_dematcher_impl::rate_dematch, in place on the soft buffer `out` (cb_len LLRs). */
int ref_rate_dematch(int8_t*       out,
                     unsigned      cb_len,
                     const int8_t* in,
                     unsigned      E,
                     int           new_data,
                     unsigned      rv,
                     unsigned      Qm,
                     unsigned      Nref,
                     unsigned      F)
{
  auto dm = std::make_unique<ldpc_rate_dematcher_impl>();
  dm->rate_dematch(llr_out(out, cb_len), llr_in(in, E), new_data != 0, metadata(1, 2, rv, Qm, Nref, F, 24));
  return 0;
}

/* ldpc_encoder_generic::encode. msg_packed: K*Z bits (fillers zero), cw_packed: cb_len bits, both MSB first. */
int ref_ldpc_encode(int bg, unsigned Z, const uint8_t* msg_packed, uint8_t* cw_packed, unsigned cb_len)
{
  auto                 enc   = std::make_unique<ldpc_encoder_generic>();
  unsigned             nbits = (bg == 1 ? 22 : 10) * Z;
  std::vector<uint8_t> msg(msg_packed, msg_packed + (nbits + 7) / 8);
  bit_buffer           in  = bit_buffer::from_bytes(msg).first(nbits);
  bit_buffer           out = bit_buffer::from_bytes({cw_packed, (cb_len + 7) / 8}).first(cb_len);
  enc->encode(out, in, metadata(bg, Z, 0, 1, 0, 0, 24).tb_common);
  return 0;
}

/* ldpc_rate_matcher_impl::rate_match. cw_packed: N codeblock bits (fillers zero), out_packed: E bits. */
int ref_rate_match(uint8_t*       out_packed,
                   unsigned       E,
                   const uint8_t* cw_packed,
                   unsigned       N,
                   unsigned       rv,
                   unsigned       Qm,
                   unsigned       Nref,
                   int            bg,
                   unsigned       F)
{
  auto                 rm = std::make_unique<ldpc_rate_matcher_impl>();
  std::vector<uint8_t> cw(cw_packed, cw_packed + (N + 7) / 8);
  bit_buffer           in  = bit_buffer::from_bytes(cw).first(N);
  bit_buffer           out = bit_buffer::from_bytes({out_packed, (E + 7) / 8}).first(E);
  rm->rate_match(out, in, metadata(bg, 2, rv, Qm, Nref, F, 24));
  return 0;
}

/* demodulation_mapper_impl::demodulate_soft. mod: modulation_scheme value. */
int ref_demodulate_soft(int mod, unsigned nof_symbols, const float* sym, const float* nv, int8_t* llr)
{
  demodulation_mapper_impl dm;
  modulation_scheme        m = static_cast<modulation_scheme>(mod);
  dm.demodulate_soft(llr_out(llr, nof_symbols * get_bits_per_symbol(m)),
                     {reinterpret_cast<const cf_t*>(sym), nof_symbols},
                     {nv, nof_symbols},
                     m);
  return 0;
}

/* pseudo_random_generator_impl: init(c_init), advance(offset), apply_xor on LLRs. */
int ref_descramble(unsigned c_init, unsigned offset, unsigned n, const int8_t* in, int8_t* out)
{
  pseudo_random_generator_impl prg;
  prg.init(c_init);
  prg.advance(offset);
  prg.apply_xor(llr_out(out, n), llr_in(in, n));
  return 0;
}

/* The same generator's apply_xor on packed bits (nbits, MSB first). */
int ref_scramble_packed(unsigned c_init, unsigned offset, unsigned nbits, const uint8_t* in, uint8_t* out)
{
  pseudo_random_generator_impl prg;
  prg.init(c_init);
  prg.advance(offset);
  std::vector<uint8_t> src(in, in + (nbits + 7) / 8);
  bit_buffer           bin  = bit_buffer::from_bytes(src).first(nbits);
  bit_buffer           bout = bit_buffer::from_bytes({out, (nbits + 7) / 8}).first(nbits);
  prg.apply_xor(bout, bin);
  return 0;
}

/* crc_calculator_generic_impl::calculate_bit (one bit per byte) and ::calculate (packed). */
uint32_t ref_crc_bits(int poly, const uint8_t* bits, unsigned nbits)
{
  crc_calculator_generic_impl crc(static_cast<crc_generator_poly>(poly));
  return crc.calculate_bit({bits, nbits});
}

uint32_t ref_crc_packed(int poly, const uint8_t* packed, unsigned nbits)
{
  crc_calculator_generic_impl crc(static_cast<crc_generator_poly>(poly));
  std::vector<uint8_t>        src(packed, packed + (nbits + 7) / 8);
  return crc.calculate(bit_buffer::from_bytes(src).first(nbits));
}

/* log_likelihood_ratio's saturating operators, for the arithmetic pins. */
int8_t ref_llr_add(int8_t a, int8_t b)
{
  log_likelihood_ratio x = a;
  x += log_likelihood_ratio(b);
  return x.to_value_type();
}

int8_t ref_llr_promotion_sum(int8_t a, int8_t b)
{
  return log_likelihood_ratio::promotion_sum(a, b).to_value_type();
}

int8_t ref_llr_quantize(float value, float range)
{
  return log_likelihood_ratio::quantize(value, range).to_value_type();
}

} // extern "C"
