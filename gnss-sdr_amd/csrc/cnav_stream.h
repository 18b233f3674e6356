// The arithmetic of gnss-sdr's GPS CNAV decoder (L2C, L5), restated as plain C++: libswiftcnav's cnav_msg.c, viterbi27.c, bits.c and edc.c under
// src/algorithms/telemetry_decoder/libs/libswiftcnav/.  The same text runs on the lanes of cnav_stream_kernel (cnav_stream.hip, one wave64 per channel,
// one lane per trellis state) and -- for tests/test_cnav_stream_host.py -- on the host (the pattern of viterbi_acs.h and kalman_step.h).  Unlike the
// Galileo page decoder this one is a continuous stream: no tail, no interleaver, integer metrics, state that lives from symbol to symbol.
//   cnav_branch_bits       c0 / c1 of v27_poly_init with the reversed polynomials 0x4F, 0x6D              viterbi27.c:40-49, cnav_msg.c:38-41
//   cnav_acs               one new state of a trellis step (both halves of the butterfly)                 viterbi27.c:85-102
//   cnav_norm_floor        what a step subtracts once new metric 0 has passed 2^30                        viterbi27.c:158-176
//   cnav_traceback         64 steps back from a given state, the older 32 bits                            viterbi27.c:200-222, cnav_msg.c:190-199
//   cnav_part_add_symbol   block cadence (128 symbols, then 64) and what follows a decode                 cnav_msg.c:162-199
//   cnav_rescan            search for either preamble from bit 1                                          cnav_msg.c:117-145
//   cnav_lock_machine      preamble, 300 bits, CRC, lock, failure counter, the retry loop                 cnav_msg.c:217-280
//   cnav_deliver           un-inverted bits, fields, delay, the shift by 300                              cnav_msg.c:323-361
//   cnav_channel_add_symbol  both parts take the symbol, the locked one starves the other                 cnav_msg.c:415-439
//   cnav_channel_init      cnav_msg_decoder_init, part 2 primed with 0x80                                 cnav_msg.c:374-390, viterbi27.c:63-81
//   cnav_quantise          HARD: gps_l2c_telemetry_decoder_gs.cc:178, gps_l5_telemetry_decoder_gs.cc:213; SOFT: for callers who have soft symbols
// The functions that walk a part are templates over an Ops object that owns the part's arrays: CnavHostOps below keeps them in a
// gsh_cnav_part_state and loops over the 64 states, the kernel's Ops keeps the metrics in the lanes and the rest in LDS.  Everything a branch
// depends on (CnavRegs) is uniform across the wave.
// THE STALE-METRICS QUIRK.  v27_chainback_likely ranks v->new_metrics, and v27_update has swapped the pointers after its last step
// (viterbi27.c:184-187, 232-248): the "most likely state" is chosen by the metrics of the step BEFORE the last one, and the trace-back then starts
// from that state in the last step's decisions.  Reproduced as it is, which is why a part keeps both arrays: old_metrics (after the last step) and
// new_metrics (after the one before).
// THE CRC.  crc24q_bits (edc.c:105-131) feeds four zero bits and then the 276 bits, XORed with the invert flag, through the table form of CRC-24Q from
// a register of zero; leading zeros leave a zero register alone, so the bit-serial tlm_crc24q_bit of viterbi_acs.h over the 276 bits is the same
// value (checked against the reference on every message of tests/golden/cnav.npz, inverted ones included).
#ifndef GSH_CNAV_STREAM_H
#define GSH_CNAV_STREAM_H

#include "gnss_sdr_hip.h"
#include "viterbi_acs.h"
#include <cmath>
#include <cstdint>

namespace gsh
{
constexpr int CNAV_STATES = 64;
constexpr uint32_t CNAV_HISTORY = 64;        // GPS_L2_V27_HISTORY_LENGTH_BITS, cnav_msg.h:40
constexpr uint32_t CNAV_FIRST_SYMBOLS = 128;  // (GPS_L2C_V27_INIT_BITS + GPS_L2C_V27_DECODE_BITS) * 2, cnav_msg.c:169
constexpr uint32_t CNAV_BLOCK_SYMBOLS = 64;   // GPS_L2C_V27_DECODE_BITS * 2, cnav_msg.c:175
constexpr uint32_t CNAV_DECODE_BITS = 32, CNAV_DELAY_BITS = 32;
constexpr int CNAV_DECODED_WORDS = 16;  // the 64-byte decode buffer, MSB first
constexpr uint32_t CNAV_DECODED_BITS = 512;
constexpr uint32_t CNAV_MSG_BITS = 300, CNAV_DATA_BITS = 276, CNAV_PREAMBLE_BITS = 8;
constexpr int CNAV_MSG_WORDS = 10;
constexpr uint32_t CNAV_PREAMBLE = 0x8Bu, CNAV_PREAMBLE_INV = 0x74u;  // cnav_msg.c:47-49
constexpr uint32_t CNAV_MAX_CRC_FAILS = 10;                          // cnav_msg.c:59
constexpr uint32_t CNAV_POLY_A = 0x4Fu, CNAV_POLY_B = 0x6Du;
constexpr uint32_t CNAV_FLAG_PREAMBLE = GSH_CNAV_FLAG_PREAMBLE_SEEN, CNAV_FLAG_INVERT = GSH_CNAV_FLAG_INVERT, CNAV_FLAG_LOCK = GSH_CNAV_FLAG_MESSAGE_LOCK,
                   CNAV_FLAG_CRC_OK = GSH_CNAV_FLAG_CRC_OK, CNAV_FLAG_INIT = GSH_CNAV_FLAG_INIT;

// what a part's control flow depends on; on the device these are uniform across the wave
struct CnavRegs
{
    uint32_t n_symbols, n_decoded, flags, n_crc_fail, decisions_index;
};

struct CnavDelivery
{
    uint32_t delay, tow, prn, msg_id, alert, invert;
};

GSH_TLM_FN uint32_t cnav_parity(uint32_t x)
{
    x ^= x >> 4;
    x ^= x >> 2;
    x ^= x >> 1;
    return x & 1u;
}

// c0[i], c1[i] of butterfly i (0..31): 255 where the parity of (2 i) & polynomial is odd
GSH_TLM_FN void cnav_branch_bits(uint32_t i, uint32_t& c0, uint32_t& c1)
{
    c0 = cnav_parity((2u * i) & CNAV_POLY_A) ? 255u : 0u;
    c1 = cnav_parity((2u * i) & CNAV_POLY_B) ? 255u : 0u;
}

// new state n of one step from its predecessors' metrics old[n >> 1] and old[(n >> 1) + 32].  All sums wrap as unsigned, the comparison is the
// signed difference, as in the reference.
GSH_TLM_FN uint32_t cnav_acs(uint32_t n, uint32_t old_lo, uint32_t old_hi, uint32_t sym0, uint32_t sym1, uint32_t& decision)
{
    uint32_t c0, c1;
    cnav_branch_bits(n >> 1, c0, c1);
    const uint32_t m = (c0 ^ sym0) + (c1 ^ sym1);
    const uint32_t with = (n & 1u) ? 510u - m : m;
    const uint32_t m0 = old_lo + with;
    const uint32_t m1 = old_hi + (510u - with);
    decision = static_cast<int32_t>(m0 - m1) > 0 ? 1u : 0u;
    return decision ? m1 : m0;
}

GSH_TLM_FN bool cnav_norm_due(uint32_t new_metric0) { return new_metric0 > (1u << 30); }

// the reference's minimum starts at 2^31 and only smaller metrics replace it
GSH_TLM_FN uint32_t cnav_norm_floor(uint32_t min_of_64) { return min_of_64 < (1u << 31) ? min_of_64 : (1u << 31); }

// 64 steps back from `state` through the ring, newest entry at index - 1.  The reference writes the survivor's bits in time order and the caller keeps
// the first 32 of the 64: the bits of the older half, first bit in the top bit of the result.
template <class Ring>
GSH_TLM_FN uint32_t cnav_traceback(const Ring& ring, uint32_t index, uint32_t state)
{
    uint32_t reg = (state & 63u) << 2;  // final_state, an 8-bit register whose top six bits are the state
    uint32_t out = 0;
    for (int b = static_cast<int>(CNAV_HISTORY) - 1; b >= 0; b--)
        {
            index = (index + CNAV_HISTORY - 1u) & (CNAV_HISTORY - 1u);
            const uint32_t k = static_cast<uint32_t>((ring[index] >> (reg >> 2)) & 1ull);
            reg = (reg >> 1) | (k << 7);
            if (b < static_cast<int>(CNAV_DECODE_BITS)) out |= k << (31 - b);
        }
    return out;
}

// len <= 32 bits at bit pos of the decode buffer (getbitu, bits.c:56-67); pos + len <= 512
template <class Ops>
GSH_TLM_FN uint32_t cnav_bits(Ops& o, uint32_t pos, uint32_t len)
{
    const uint32_t w = pos >> 5;
    const uint64_t two = (static_cast<uint64_t>(o.word(w)) << 32) | (w + 1 < static_cast<uint32_t>(CNAV_DECODED_WORDS) ? o.word(w + 1) : 0u);
    return static_cast<uint32_t>((two << (pos & 31u)) >> (64u - len));
}

// word j of the buffer after a shift left by k bits (bitshl, bits.c:146-185), from the words before it
GSH_TLM_FN uint32_t cnav_shifted_word(const uint32_t* dec, uint32_t j, uint32_t k)
{
    const uint32_t q = k >> 5, r = k & 31u;
    const uint32_t a = j + q < static_cast<uint32_t>(CNAV_DECODED_WORDS) ? dec[j + q] : 0u;
    const uint32_t b = j + q + 1 < static_cast<uint32_t>(CNAV_DECODED_WORDS) ? dec[j + q + 1] : 0u;
    return r ? (a << r) | (b >> (32u - r)) : a;
}

// whether the 8 bits at position i are a preamble (cnav_msg.c:127-128); inv = the inverted one
GSH_TLM_FN bool cnav_preamble_at(const uint32_t* dec, uint32_t i, bool& inv)
{
    const uint32_t w = i >> 5;
    const uint64_t two = (static_cast<uint64_t>(dec[w]) << 32) | (w + 1 < static_cast<uint32_t>(CNAV_DECODED_WORDS) ? dec[w + 1] : 0u);
    const uint32_t c = static_cast<uint32_t>((two << (i & 31u)) >> 56);
    inv = c == CNAV_PREAMBLE_INV;
    return c == CNAV_PREAMBLE || c == CNAV_PREAMBLE_INV;
}

// 32 new bits at bit n of the buffer (bitcopy / setbitu, bits.c:100-120, 203-221): the other bits stay
GSH_TLM_FN void cnav_append_words(uint32_t* dec, uint32_t n, uint32_t v)
{
    const uint32_t w = n >> 5, r = n & 31u;
    if (w >= static_cast<uint32_t>(CNAV_DECODED_WORDS)) return;
    if (r == 0)
        {
            dec[w] = v;
            return;
        }
    dec[w] = (dec[w] & ~(0xFFFFFFFFu >> r)) | (v >> r);
    if (w + 1 < static_cast<uint32_t>(CNAV_DECODED_WORDS)) dec[w + 1] = (dec[w + 1] & (0xFFFFFFFFu >> r)) | (v << (32u - r));
}

// CRC-24Q over bits 0..275 XOR invert (cnav_compute_crc_, cnav_msg.c:72-78)
template <class Ops>
GSH_TLM_FN uint32_t cnav_crc(Ops& o, bool invert)
{
    uint32_t reg = 0;
    for (uint32_t w = 0; w * 32u < CNAV_DATA_BITS; w++)
        {
            const uint32_t word = o.word(w) ^ (invert ? 0xFFFFFFFFu : 0u);
            const uint32_t nb = CNAV_DATA_BITS - w * 32u < 32u ? CNAV_DATA_BITS - w * 32u : 32u;
            for (uint32_t b = 0; b < nb; b++) reg = tlm_crc24q_bit(reg, (word >> (31u - b)) & 1u);
        }
    return reg;
}

template <class Ops>
GSH_TLM_FN void cnav_rescan(CnavRegs& r, Ops& o)
{
    r.flags &= ~CNAV_FLAG_PREAMBLE;
    if (r.n_decoded > CNAV_PREAMBLE_BITS + 1)
        {
            bool inv = false;
            const uint32_t i = o.find_preamble(r.n_decoded - CNAV_PREAMBLE_BITS, inv);  // the first i in 1 .. n_decoded - 9, or 0
            if (i)
                {
                    r.flags = (r.flags & ~CNAV_FLAG_INVERT) | CNAV_FLAG_PREAMBLE | (inv ? CNAV_FLAG_INVERT : 0u);
                    o.shift(i);
                    r.n_decoded -= i;
                }
        }
    if (!(r.flags & CNAV_FLAG_PREAMBLE) && r.n_decoded >= CNAV_PREAMBLE_BITS)
        {
            o.shift(r.n_decoded - CNAV_PREAMBLE_BITS + 1);
            r.n_decoded = CNAV_PREAMBLE_BITS - 1;
        }
}

// Every retry has either dropped a preamble that sat at bit 0, so that the rescan from bit 1 shortens the buffer, or found none, which ends the
// loop: at most n_decoded passes, bounded here by the buffer's length whatever the state holds.
template <class Ops>
GSH_TLM_FN void cnav_lock_machine(CnavRegs& r, Ops& o)
{
    bool retry = true;
    for (uint32_t pass = 0; retry && pass < CNAV_DECODED_BITS; pass++)
        {
            retry = false;
            if (!(r.flags & CNAV_FLAG_PREAMBLE)) cnav_rescan(r, o);
            if ((r.flags & CNAV_FLAG_PREAMBLE) && r.n_decoded >= CNAV_MSG_BITS)
                {
                    const bool invert = (r.flags & CNAV_FLAG_INVERT) != 0;
                    const uint32_t crc = cnav_crc(o, invert);
                    const uint32_t sent = cnav_bits(o, CNAV_DATA_BITS, 24) ^ (invert ? 0xFFFFFFu : 0u);  // cnav_extract_crc_, cnav_msg.c:91-100
                    const bool ok = o.uniform(crc == sent);
                    if (r.flags & CNAV_FLAG_LOCK)
                        {
                            r.flags = (r.flags & ~CNAV_FLAG_CRC_OK) | (ok ? CNAV_FLAG_CRC_OK : 0u);
                            if (ok)
                                r.n_crc_fail = 0;
                            else if (++r.n_crc_fail > CNAV_MAX_CRC_FAILS)
                                {
                                    r.n_crc_fail = 0;
                                    r.flags &= ~(CNAV_FLAG_LOCK | CNAV_FLAG_PREAMBLE);
                                    retry = true;
                                }
                        }
                    else if (ok)
                        {
                            r.flags |= CNAV_FLAG_LOCK | CNAV_FLAG_CRC_OK;
                            r.n_crc_fail = 0;
                        }
                    else
                        {
                            r.flags &= ~(CNAV_FLAG_CRC_OK | CNAV_FLAG_PREAMBLE);
                            retry = true;
                        }
                }
        }
}

template <class Ops>
GSH_TLM_FN void cnav_part_add_symbol(CnavRegs& r, Ops& o, uint32_t symbol)
{
    if (r.n_symbols < CNAV_FIRST_SYMBOLS) o.put_symbol(r.n_symbols, symbol);
    r.n_symbols++;
    if (r.flags & CNAV_FLAG_INIT)
        {
            if (r.n_symbols < CNAV_FIRST_SYMBOLS) return;
            r.flags &= ~CNAV_FLAG_INIT;
        }
    else if (r.n_symbols < CNAV_BLOCK_SYMBOLS)
        return;
    const uint32_t steps = (r.n_symbols < CNAV_FIRST_SYMBOLS ? r.n_symbols : CNAV_FIRST_SYMBOLS) / 2;
    const uint32_t v = o.decode_block(steps, r.decisions_index);  // v27_update, then v27_chainback_likely over 64 bits, of which the older 32
    r.n_symbols = 0;
    o.append(r.n_decoded, v);
    r.n_decoded += CNAV_DECODE_BITS;
    cnav_lock_machine(r, o);
}

// cnav_msg_decode_: the message if the part holds 300 bits and its last CRC was good; the 300 bits leave the buffer either way.  bits_out is where the
// Ops writes the 10 words (nullptr: the caller has no room, nothing is written)
template <class Ops>
GSH_TLM_FN bool cnav_deliver(CnavRegs& r, Ops& o, CnavDelivery& d, uint32_t* bits_out)
{
    if (r.n_decoded < CNAV_MSG_BITS) return false;
    const bool ok = (r.flags & CNAV_FLAG_CRC_OK) != 0;
    if (ok)
        {
            const bool inv = (r.flags & CNAV_FLAG_INVERT) != 0;
            const uint32_t head = o.uniform(cnav_bits(o, 8, 30) ^ (inv ? 0x3FFFFFFFu : 0u));  // bits 8..37
            d.prn = head >> 24;
            d.msg_id = (head >> 18) & 0x3Fu;
            d.tow = (head >> 1) & 0x1FFFFu;
            d.alert = head & 1u;
            d.invert = inv ? 1u : 0u;
            d.delay = (r.n_decoded - CNAV_MSG_BITS + CNAV_DELAY_BITS) * 2u + r.n_symbols;
            if (bits_out) o.write_message(bits_out, inv);
        }
    o.shift(CNAV_MSG_BITS);
    r.n_decoded -= CNAV_MSG_BITS;
    return ok;
}

// cnav_msg_decoder_add_symbol: 0 nothing, 1 part 1 delivered, 2 part 2 delivered.  The part that holds the lock empties the other part's symbol and
// decode counts on every symbol, so the other one never reaches a decode block: it resumes, from a frozen trellis, only after the lock is lost.
template <class Ops>
GSH_TLM_FN int cnav_channel_add_symbol(CnavRegs& r1, Ops& o1, CnavRegs& r2, Ops& o2, uint32_t symbol, CnavDelivery& d, uint32_t* bits_out)
{
    cnav_part_add_symbol(r1, o1, symbol);
    cnav_part_add_symbol(r2, o2, symbol);
    if (r1.flags & CNAV_FLAG_LOCK)
        {
            r2.n_decoded = 0;
            r2.n_symbols = 0;
            return cnav_deliver(r1, o1, d, bits_out) ? 1 : 0;
        }
    if (r2.flags & CNAV_FLAG_LOCK)
        {
            r1.n_decoded = 0;
            r1.n_symbols = 0;
            return cnav_deliver(r2, o2, d, bits_out) ? 2 : 0;
        }
    return 0;
}

// HARD is what both telemetry blocks feed the library; SOFT(scale) maps [-scale, scale] onto 0..255 in float32, one rounding per operation
// (contraction off), ties to even; a NaN quantises as -scale does
GSH_TLM_FN uint32_t cnav_quantise(float x, int mode, float scale)
{
    if (mode == GSH_CNAV_QUANTISER_HARD) return x > 0.0f ? 255u : 0u;
    const float t = fminf(fmaxf(x / scale, -1.0f), 1.0f);
    const float scaled = 127.5f * t;
    return static_cast<uint32_t>(rintf(127.5f + scaled));
}

inline void cnav_regs_load(const gsh_cnav_part_state& s, CnavRegs& r)
{
    r = CnavRegs{s.n_symbols, s.n_decoded, s.flags, s.n_crc_fail, s.decisions_index};
}

inline void cnav_regs_store(const CnavRegs& r, gsh_cnav_part_state& s)
{
    s.n_symbols = r.n_symbols;
    s.n_decoded = r.n_decoded;
    s.flags = r.flags;
    s.n_crc_fail = r.n_crc_fail;
    s.decisions_index = r.decisions_index;
}

// whether a state can be walked without leaving its arrays (every reachable state passes)
inline bool cnav_state_valid(const gsh_cnav_channel_state& s)
{
    for (const gsh_cnav_part_state& p : s.part)
        {
            const uint32_t room = (p.flags & CNAV_FLAG_INIT) ? CNAV_FIRST_SYMBOLS : CNAV_BLOCK_SYMBOLS;
            if (p.decisions_index >= CNAV_HISTORY || p.n_symbols >= room || p.n_decoded > CNAV_DECODED_BITS - CNAV_DECODE_BITS) return false;
            if (p.flags & ~(CNAV_FLAG_PREAMBLE | CNAV_FLAG_INVERT | CNAV_FLAG_LOCK | CNAV_FLAG_CRC_OK | CNAV_FLAG_INIT)) return false;
        }
    return true;
}

// one part on one thread: the arrays are those of the state
struct CnavHostOps
{
    gsh_cnav_part_state& s;
    static bool uniform(bool v) { return v; }
    static uint32_t uniform(uint32_t v) { return v; }
    uint32_t word(uint32_t j) const { return s.decoded[j]; }
    void put_symbol(uint32_t i, uint32_t symbol) { s.symbols[i] = static_cast<uint8_t>(symbol); }
    void append(uint32_t n, uint32_t v) { cnav_append_words(s.decoded, n, v); }
    void shift(uint32_t k)
    {
        for (uint32_t j = 0; j < static_cast<uint32_t>(CNAV_DECODED_WORDS); j++) s.decoded[j] = cnav_shifted_word(s.decoded, j, k);  // reads only words >= j
    }
    uint32_t find_preamble(uint32_t end, bool& inv) const
    {
        for (uint32_t i = 1; i < end; i++)
            if (cnav_preamble_at(s.decoded, i, inv)) return i;
        return 0;
    }
    void write_message(uint32_t* out, bool inv) const
    {
        for (int j = 0; j < CNAV_MSG_WORDS; j++)
            {
                const uint32_t mask = j == CNAV_MSG_WORDS - 1 ? ~(0xFFFFFFFFu >> (CNAV_MSG_BITS & 31u)) : 0xFFFFFFFFu;
                out[j] = (s.decoded[j] ^ (inv ? 0xFFFFFFFFu : 0u)) & mask;
            }
    }
    uint32_t decode_block(uint32_t steps, uint32_t& index)
    {
        for (uint32_t t = 0; t < steps; t++)
            {
                uint32_t next[CNAV_STATES];
                uint64_t word = 0;
                for (uint32_t n = 0; n < static_cast<uint32_t>(CNAV_STATES); n++)
                    {
                        uint32_t dec;
                        next[n] = cnav_acs(n, s.old_metrics[n >> 1], s.old_metrics[(n >> 1) + 32], s.symbols[2 * t], s.symbols[2 * t + 1], dec);
                        word |= static_cast<uint64_t>(dec) << n;
                    }
                s.decisions[index] = word;
                if (cnav_norm_due(next[0]))
                    {
                        uint32_t lowest = next[0];
                        for (uint32_t m : next) lowest = m < lowest ? m : lowest;
                        const uint32_t floor = cnav_norm_floor(lowest);
                        for (uint32_t& m : next) m -= floor;
                    }
                index = (index + 1u) & (CNAV_HISTORY - 1u);
                for (int n = 0; n < CNAV_STATES; n++)
                    {
                        s.new_metrics[n] = s.old_metrics[n];  // the pointer swap
                        s.old_metrics[n] = next[n];
                    }
            }
        uint32_t best = 0, best_metric = 0xFFFFFFFFu;  // over new_metrics: see THE STALE-METRICS QUIRK
        for (uint32_t n = 0; n < static_cast<uint32_t>(CNAV_STATES); n++)
            if (s.new_metrics[n] < best_metric)
                {
                    best_metric = s.new_metrics[n];
                    best = n;
                }
        return cnav_traceback(s.decisions, index, best);
    }
};

inline void cnav_channel_init(gsh_cnav_channel_state& s)
{
    s = gsh_cnav_channel_state{};
    for (gsh_cnav_part_state& p : s.part)
        {
            for (int n = 1; n < CNAV_STATES; n++) p.old_metrics[n] = 63;  // v27_init: state 0 starts at 0
            p.flags = CNAV_FLAG_INIT;
        }
    CnavRegs r;
    CnavHostOps o{s.part[1]};
    cnav_regs_load(s.part[1], r);
    cnav_part_add_symbol(r, o, 0x80u);  // cnav_msg.c:389
    cnav_regs_store(r, s.part[1]);
}

// The result entries a job of n symbols needs.  The part that holds the lock gains 32 bits per 64 symbols and holds fewer than 300 between two
// symbols (300 bits are delivered on the symbol that completes them), so d deliveries within n symbols need 32 * ceil(n / 64) >= 300 d - 299: two
// need 577 symbols, three 1 153, four 1 793, and from there on each further one at least 576 more.  (n + 575) / 576 covers all of them, and is never
// below n / 600 + 1.  Only a state imported with more than 299 decoded bits can deliver sooner; the count then runs past the capacity and says so.
GSH_TLM_FN uint64_t cnav_result_capacity(uint64_t n) { return n == 0 ? 1u : (n + 575u) / 576u; }

// `n` symbols through one channel on one thread; messages beyond `capacity` are counted but not written.  Returns the messages delivered.
inline uint32_t cnav_channel_push(gsh_cnav_channel_state& s, const uint8_t* symbols, uint32_t n, gsh_cnav_message* out, uint32_t capacity)
{
    CnavRegs r1, r2;
    CnavHostOps o1{s.part[0]}, o2{s.part[1]};
    cnav_regs_load(s.part[0], r1);
    cnav_regs_load(s.part[1], r2);
    uint32_t count = 0;
    for (uint32_t k = 0; k < n; k++)
        {
            CnavDelivery d{};
            gsh_cnav_message* slot = count < capacity ? out + count : nullptr;
            const int part = cnav_channel_add_symbol(r1, o1, r2, o2, symbols[k], d, slot ? slot->bits : nullptr);
            if (part) count++;
            if (part && slot)
                {
                    slot->symbol_index = k;
                    slot->delay = d.delay;
                    slot->tow = d.tow;
                    slot->prn = static_cast<uint8_t>(d.prn);
                    slot->msg_id = static_cast<uint8_t>(d.msg_id);
                    slot->alert = static_cast<uint8_t>(d.alert);
                    slot->part = static_cast<uint8_t>(part);
                    slot->invert = static_cast<uint8_t>(d.invert);
                    slot->invert_or = ((r1.flags | r2.flags) & CNAV_FLAG_INVERT) ? 1 : 0;
                    slot->reserved[0] = slot->reserved[1] = 0;
                }
        }
    cnav_regs_store(r1, s.part[0]);
    cnav_regs_store(r2, s.part[1]);
    return count;
}
}  // namespace gsh

#endif
