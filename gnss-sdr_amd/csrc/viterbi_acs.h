// The arithmetic of gnss-sdr's Galileo telemetry page decoder, restated as plain C++: the same text runs on the lanes of tlm_pages_kernel
// (telemetry_viterbi.hip, one wave64 per channel, one lane per trellis state) and -- for tests/test_viterbi_acs_host.py -- on the host, with
// -ffp-contract=off on both sides (the pattern of kalman_step.h and exact_division.h).
//   tlm_out_symbol      nsc_enc_bit / nsc_transit                       viterbi_decoder.cc:134-148, 183-204
//   tlm_gamma           Gamma                                           viterbi_decoder.cc:151-166
//   tlm_acs             one next state of the trellis step              viterbi_decoder.cc:70-93
//   tlm_traceback       the trace-back                                  viterbi_decoder.cc:106-119
//   tlm_soft            deinterleaver, G2's NOT gate, the 180 deg lock  galileo_telemetry_decoder_gs.cc:352-377, 1033-1046
//   tlm_crc24q_bit      boost::crc_optimal<24, 0x1864CFBU, 0, 0, false, false>, bit by bit (galileo_{inav,fnav,cnav}_message.cc)
//   tlm_decode_page     the page as the kernel walks it, on one thread (host side of the tests)
// K = 7, rate 1/2, generators 121 and 91 (decimal), 64 states.  A state's word is (input << 6) ^ state and its successor word >> 1, so the two
// predecessors of state s are 2 * (s & 31) and 2 * (s & 31) + 1, both with input bit s >> 5.  The reference walks the predecessors in ascending order and
// keeps a candidate only if it is strictly greater than what the next state holds (-1e7f to begin with): the lower predecessor is taken if > -1e7f, the
// higher one replaces it only if strictly greater.  A next state neither candidate reached keeps -1e7f; its decision is recorded as 0 here (the reference
// leaves its d_prev_state entry as it was: with |symbol| <= 1e5 no survivor through state 0 at the end passes such an entry).
// TWO METRIC MODES.  GSH_TLM_METRIC_FULL: both symbols of a pair enter Gamma and a page starts from state 0 alone (all others -1e7f): a maximum-likelihood
// decoder.  GSH_TLM_METRIC_REFERENCE: the reference as it runs -- decode() copies d_nn - 1 = 1 element per pair (viterbi_decoder.cc:61), so rec[1] stays 0
// and the G2 stream never enters the metric; and apart from element 0 being set to 0 (:56) a page starts from the normalised metrics the object's previous
// page ended with.
#ifndef GSH_VITERBI_ACS_H
#define GSH_VITERBI_ACS_H

#include <cstdint>

#ifdef __HIPCC__
#define GSH_TLM_FN __device__ __host__ inline __attribute__((always_inline))
#else
#define GSH_TLM_FN inline
#endif

namespace gsh
{
constexpr float TLM_MAXLOG = 1e7f;  // d_MAXLOG, viterbi_decoder.h
constexpr int TLM_STATES = 64;
constexpr int TLM_MEMORY = 6;            // d_mm: the tail
constexpr int TLM_G1 = 121, TLM_G2 = 91;  // g_encoder, galileo_telemetry_decoder_gs.cc:161
constexpr int TLM_MAX_SYMBOLS = 984;     // C/NAV
constexpr int TLM_MAX_STEPS = 492;
constexpr int TLM_BIT_WORDS = 16;        // 486 information bits at most, MSB first
constexpr uint32_t TLM_CRC24Q_POLY = 0x864CFBu;  // 0x1864CFB without its leading term

constexpr int TLM_METRIC_FULL = 0, TLM_METRIC_REFERENCE = 1;
constexpr uint32_t TLM_JOB_INVERT = 1u, TLM_JOB_CRC_CONTINUE = 2u, TLM_JOB_INAV_AUTO = 4u;

struct TlmGeometry
{
    int symbols;       // d_frame_length_symbols: what follows the preamble
    int steps;         // symbols / 2 = d_LL + d_mm
    int info_bits;     // d_datalength
    int rows, cols;    // the block interleaver
    int preamble_len;  // d_samples_per_preamble
};

// d_frame_type 1 I/NAV page part, 2 F/NAV, 3 C/NAV (galileo_telemetry_decoder_gs.cc:177-223)
GSH_TLM_FN bool tlm_geometry(int frame_type, TlmGeometry& g)
{
    switch (frame_type)
        {
        case 1:
            g = TlmGeometry{240, 120, 114, 8, 30, 10};
            return true;
        case 2:
            g = TlmGeometry{488, 244, 238, 8, 61, 12};
            return true;
        case 3:
            g = TlmGeometry{984, 492, 486, 8, 123, 16};
            return true;
        default:
            g = TlmGeometry{0, 0, 0, 0, 0, 0};
            return false;
        }
}

// preamble chip k as +1 / -1: "0101100000", "101101110000", "1011011101110000" as 16-bit words, first chip in the top bit of its length
GSH_TLM_FN int tlm_preamble_chip(int frame_type, int k)
{
    const unsigned word = frame_type == 1 ? 0x160u : (frame_type == 2 ? 0xB70u : 0xB770u);
    const int len = frame_type == 1 ? 10 : (frame_type == 2 ? 12 : 16);
    return ((word >> (len - 1 - k)) & 1u) ? 1 : -1;
}

GSH_TLM_FN int tlm_parity7(int w)
{
    w ^= w >> 4;
    w ^= w >> 2;
    w ^= w >> 1;
    return w & 1;
}

// nsc_enc_bit's output symbol for `input` entering `state`: (parity(word & G1) << 1) + parity(word & G2)
GSH_TLM_FN int tlm_out_symbol(int input, int state)
{
    const int word = (input << TLM_MEMORY) ^ state;
    return (tlm_parity7(word & TLM_G1) << 1) + tlm_parity7(word & TLM_G2);
}

// Gamma, in its own order: rm = 0; bit 0 of the symbol adds rec[1], then bit 1 adds rec[0]
GSH_TLM_FN float tlm_gamma(int symbol, float rec0, float rec1)
{
    float rm = 0.0f;
    if (symbol & 1) rm += rec1;
    if (symbol & 2) rm += rec0;
    return rm;
}

// the metric next state s holds after the step's two candidates, before normalisation; decision = 1 when the higher predecessor won
GSH_TLM_FN float tlm_acs(int sym_lo, int sym_hi, float prev_lo, float prev_hi, float rec0, float rec1, int& decision)
{
    float next = -TLM_MAXLOG;
    decision = 0;
    const float m_lo = prev_lo + tlm_gamma(sym_lo, rec0, rec1);
    if (m_lo > next) next = m_lo;
    const float m_hi = prev_hi + tlm_gamma(sym_hi, rec0, rec1);
    if (m_hi > next)
        {
            next = m_hi;
            decision = 1;
        }
    return next;
}

// soft value i of a page: in[] are the symbols after the preamble as received.  Every value is negated for a 180 deg lock (:1040-1046), the block
// deinterleaver reads soft[c * rows + r] = in[r * cols + c] (:352-361), every second value is negated for the NOT gate of G2 (:371-377)
GSH_TLM_FN float tlm_soft(const float* in, int i, int rows, int cols, bool invert)
{
    const int c = i / rows;
    const int r = i - c * rows;
    float v = in[r * cols + c];
    if (invert) v = -v;
    if (i & 1) v = -v;
    return v;
}

GSH_TLM_FN uint32_t tlm_crc24q_bit(uint32_t reg, uint32_t bit)
{
    const uint32_t top = (reg >> 23) & 1u;
    reg = (reg << 1) & 0xFFFFFFu;
    if (top ^ (bit & 1u)) reg ^= TLM_CRC24Q_POLY;
    return reg;
}

GSH_TLM_FN uint32_t tlm_bit(const uint32_t* words, int t) { return (words[t >> 5] >> (31 - (t & 31))) & 1u; }

// from state 0 after the last step back to the first: the output bit of step t is the input bit that led into the survivor's state, state >> 5 (what
// d_prev_bit holds); bits[] receives the information bits MSB first (bit t is bit 31 - t % 32 of word t / 32), the rest of the 16 words is 0
GSH_TLM_FN void tlm_traceback(const uint64_t* words, int steps, int info_bits, uint32_t* bits)
{
    int state = 0;
    uint32_t cur = 0;
    for (int w = 0; w < TLM_BIT_WORDS; w++) bits[w] = 0;
    for (int t = steps - 1; t >= 0; t--)
        {
            const int dec = static_cast<int>((words[t] >> state) & 1ull);
            if (t < info_bits)
                {
                    cur |= static_cast<uint32_t>(state >> 5) << (31 - (t & 31));
                    if ((t & 31) == 0)
                        {
                            bits[t >> 5] = cur;
                            cur = 0;
                        }
                }
            state = 2 * (state & 31) + dec;
        }
}

// what a job asks of the CRC once its bits are known: with TLM_JOB_INAV_AUTO the page's first bit chooses (Even/Odd, galileo_inav_message.cc:146):
// an even part starts the register and feeds its 114 bits, an odd part continues with its first 82 and compares the next 24 (:153-177)
GSH_TLM_FN void tlm_crc_plan(uint32_t flags, int crc_bits, int crc_check, const uint32_t* bits, bool& cont, int& n_bits, bool& check)
{
    cont = (flags & TLM_JOB_CRC_CONTINUE) != 0;
    n_bits = crc_bits;
    check = crc_check != 0;
    if (flags & TLM_JOB_INAV_AUTO)
        {
            const bool odd = tlm_bit(bits, 0) != 0;
            cont = odd;
            n_bits = odd ? 82 : 114;
            check = odd;
        }
}

// feeds bits [0, n_bits) to the register; crc_ok = -1 when nothing is compared, else whether bits [n_bits, n_bits + 24) equal the register
GSH_TLM_FN uint32_t tlm_crc_run(uint32_t reg, const uint32_t* bits, int n_bits, bool check, int& crc_ok)
{
    for (int t = 0; t < n_bits; t++) reg = tlm_crc24q_bit(reg, tlm_bit(bits, t));
    crc_ok = -1;
    if (check)
        {
            uint32_t sent = 0;
            for (int t = 0; t < 24; t++) sent = (sent << 1) | tlm_bit(bits, n_bits + t);
            crc_ok = sent == reg ? 1 : 0;
        }
    return reg;
}

#ifndef __HIP_DEVICE_COMPILE__
// One page on one thread, step for step what tlm_pages_kernel does with 64 lanes.  metrics[64] is the channel's carried block: read (but for element 0)
// and written back in reference mode, ignored in full mode.  words[] needs `steps` entries.
inline void tlm_decode_page(int metric_mode, const TlmGeometry& g, const float* in, bool invert, float* metrics, uint64_t* words, uint32_t* bits)
{
    float soft[TLM_MAX_SYMBOLS];
    for (int i = 0; i < g.symbols; i++) soft[i] = tlm_soft(in, i, g.rows, g.cols, invert);
    float prev[TLM_STATES], next[TLM_STATES];
    for (int s = 0; s < TLM_STATES; s++) prev[s] = (metric_mode == TLM_METRIC_REFERENCE) ? metrics[s] : -TLM_MAXLOG;
    prev[0] = 0.0f;
    for (int t = 0; t < g.steps; t++)
        {
            const float rec0 = soft[2 * t];
            const float rec1 = (metric_mode == TLM_METRIC_REFERENCE) ? 0.0f : soft[2 * t + 1];
            uint64_t word = 0;
            float max_val = 0.0f;
            for (int s = 0; s < TLM_STATES; s++)
                {
                    const int lo = 2 * (s & 31);
                    int dec;
                    next[s] = tlm_acs(tlm_out_symbol(s >> 5, lo), tlm_out_symbol(s >> 5, lo + 1), prev[lo], prev[lo + 1], rec0, rec1, dec);
                    word |= static_cast<uint64_t>(dec) << s;
                    if (s == 0 || next[s] > max_val) max_val = next[s];
                }
            for (int s = 0; s < TLM_STATES; s++) prev[s] = next[s] - max_val;
            words[t] = word;
        }
    if (metric_mode == TLM_METRIC_REFERENCE)
        for (int s = 0; s < TLM_STATES; s++) metrics[s] = prev[s];
    tlm_traceback(words, g.steps, g.info_bits, bits);
}
#endif
}  // namespace gsh

#endif
