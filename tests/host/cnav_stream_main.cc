// Stand-alone run of the host side of csrc/cnav_stream.h, meant to be built with -fsanitize=address,undefined and started as a program of its own
// (tests/test_cnav_stream_host.py::test_sanitizer_program).  A pseudo-random stream -- one garbage symbol, four encoded messages, thirteen messages'
// worth of random bits, three more messages, then 3 000 random soft symbols -- is decoded in one push and in ragged pushes; any difference in the
// messages or in the final state, and any message count other than the expected one, ends the program with a non-zero status.
#include "cnav_stream.h"
#include "gnss_sdr_hip.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace
{
uint32_t lcg_state = 0x2545F491u;
uint32_t lcg()
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}

void put(std::vector<uint8_t>& bits, uint32_t value, int width)
{
    for (int i = width - 1; i >= 0; i--) bits.push_back((value >> i) & 1u);
}

void message(std::vector<uint8_t>& bits, uint32_t tow)
{
    const size_t start = bits.size();
    put(bits, gsh::CNAV_PREAMBLE, 8);
    put(bits, 1 + tow % 32, 6);
    put(bits, 10 + tow % 5, 6);
    put(bits, tow, 17);
    put(bits, tow & 1u, 1);
    for (int i = 0; i < 238; i++) bits.push_back(lcg() & 1u);
    uint32_t reg = 0;
    for (size_t i = start; i < start + gsh::CNAV_DATA_BITS; i++) reg = gsh::tlm_crc24q_bit(reg, bits[i]);
    put(bits, reg, 24);
}

std::vector<uint8_t> make_stream()
{
    std::vector<uint8_t> bits;
    for (uint32_t k = 0; k < 4; k++) message(bits, 500 + k);
    for (int i = 0; i < 13 * 300; i++) bits.push_back(lcg() & 1u);
    for (uint32_t k = 0; k < 3; k++) message(bits, 600 + k);
    std::vector<uint8_t> sym;
    sym.push_back(lcg() & 0xFFu);
    uint32_t sr = 0;
    for (uint8_t b : bits)
        {
            sr = ((sr << 1) | b) & 0x7Fu;
            sym.push_back(gsh::cnav_parity(sr & gsh::CNAV_POLY_A) ? 255 : 0);
            sym.push_back(gsh::cnav_parity(sr & gsh::CNAV_POLY_B) ? 255 : 0);
        }
    for (int i = 0; i < 3000; i++) sym.push_back(lcg() & 0xFFu);
    return sym;
}

struct Run
{
    std::vector<gsh_cnav_message> messages;
    gsh_cnav_channel_state state;
};

Run decode(const std::vector<uint8_t>& sym, bool ragged)
{
    Run run;
    gsh::cnav_channel_init(run.state);
    size_t at = 0;
    while (at < sym.size())
        {
            const size_t n = ragged ? std::min<size_t>(sym.size() - at, 1 + lcg() % 700) : sym.size();
            std::vector<gsh_cnav_message> out(gsh::cnav_result_capacity(n));
            const uint32_t count = gsh::cnav_channel_push(run.state, sym.data() + at, static_cast<uint32_t>(n), out.data(), static_cast<uint32_t>(out.size()));
            if (count > out.size())
                {
                    std::printf("cnav stream: %u messages within %zu symbols, above the capacity rule's %zu\n", count, n, out.size());
                    std::exit(3);
                }
            for (uint32_t i = 0; i < count; i++)
                {
                    out[i].symbol_index += static_cast<uint32_t>(at);
                    run.messages.push_back(out[i]);
                }
            at += n;
        }
    return run;
}
}  // namespace

int main()
{
    const std::vector<uint8_t> sym = make_stream();
    const Run whole = decode(sym, false);
    if (whole.messages.size() < 5 || whole.messages.front().tow != 500 || whole.messages.back().tow < 600)
        {
            std::printf("cnav stream: %zu messages, first tow %u\n", whole.messages.size(), whole.messages.empty() ? 0u : whole.messages.front().tow);
            return 1;
        }
    for (int round = 0; round < 8; round++)
        {
            const Run pieces = decode(sym, true);
            if (pieces.messages.size() != whole.messages.size() ||
                std::memcmp(pieces.messages.data(), whole.messages.data(), sizeof(gsh_cnav_message) * whole.messages.size()) != 0 ||
                std::memcmp(&pieces.state, &whole.state, sizeof(whole.state)) != 0)
                {
                    std::printf("cnav stream: ragged round %d differs from one push\n", round);
                    return 2;
                }
        }
    std::printf("cnav stream: ok, %zu messages over %zu symbols\n", whole.messages.size(), sym.size());
    return 0;
}
