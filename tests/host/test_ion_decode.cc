// Stand-alone run of the host decoder of csrc/ion_gsms.h over a grid of layouts, meant to be built with -fsanitize=address,undefined and started
// directly (tests/test_ion_gsms_formats.py does both): every word size, both endiannesses, head padding and none, field widths 1..16, all eleven
// encodings, alignments 0 / 1 / 2, real / IQ / QI, blocks allocated at their exact size so that a byte read past a chunk or a block is caught, and a
// cycle of 4096 bytes of 64-bit words.  Every field is also read bit by bit from the block and compared (through encoding OB, whose value is the code
// minus 2^(q-1)); the values of the other encodings are checked against the header's closed forms by the Python tests.
#include "ion_gsms.h"
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

namespace
{
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
unsigned rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<unsigned>(rng_state >> 32);
}

// bit i of the chunk's bit stream, straight from the definition: word i / (8 W), its bit from the top
int stream_bit(const unsigned char* chunk, int size_word, int big_endian, unsigned i)
{
    const unsigned word = i / (8u * size_word), in_word = i % (8u * size_word), byte = in_word / 8u;
    const unsigned mem = word * size_word + (big_endian ? byte : size_word - 1u - byte);
    return (chunk[mem] >> (7u - in_word % 8u)) & 1;
}

int failures = 0;
long checked = 0;

void run(const std::vector<gsh_ion_chunk>& chunks, const std::vector<gsh_ion_stream>& streams, int cycles)
{
    gsh::IonLayout L;
    char why[256] = "";
    const int rc = gsh::ion_reduce(chunks.data(), static_cast<int>(chunks.size()), streams.data(), static_cast<int>(streams.size()), &L, why, sizeof(why));
    if (rc != GSH_OK)
        {
            std::printf("refused (%d): %s\n", rc, why);
            failures++;
            return;
        }
    const size_t nbytes = static_cast<size_t>(cycles) * L.cycle_bytes;
    std::unique_ptr<unsigned char[]> block(new unsigned char[nbytes]);  // exactly the block: one byte further is outside
    for (size_t i = 0; i < nbytes; i++) block[i] = static_cast<unsigned char>(rnd());
    for (int s = 0; s < L.n_streams; s++)
        {
            const gsh::IonStream& st = L.s[s];
            const unsigned long long total = static_cast<unsigned long long>(cycles) * st.fields;
            std::vector<float> out(total);
            // the whole block, then a window that starts and ends inside a cycle (complex: at whole samples)
            gsh::ion_decode_fields(L, s, block.get(), 0, total, out.data());
            const unsigned long long per = st.cplx ? 2 : 1, first = per, n = total > 3 * per ? total - 3 * per : 0;
            std::vector<float> win(n);
            gsh::ion_decode_fields(L, s, block.get(), first, n, win.data());
            for (unsigned long long i = 0; i < n; i++)
                if (win[i] != out[first + i]) failures++;
            if (st.e.enc != GSH_ION_OB) continue;
            // which chunk: the one whose offset the entry carries
            int size_word = 1, big = 0;
            unsigned off = 0;
            for (const gsh_ion_chunk& c : chunks)
                {
                    if (off == st.e.chunk_off)
                        {
                            size_word = c.size_word;
                            big = c.big_endian;
                        }
                    off += static_cast<unsigned>(c.size_word * c.count_words);
                }
            for (unsigned long long f = 0; f < total; f++)
                {
                    const unsigned long long cyc = f / st.fields;
                    const unsigned j = static_cast<unsigned>(f % st.fields);
                    const unsigned char* chunk = block.get() + cyc * L.cycle_bytes + st.e.chunk_off;
                    const gsh_ion_stream& d = streams[s];
                    const unsigned w = st.e.w, q = st.e.q, lead = d.alignment == 2 ? w - q : 0;
                    int code = 0;
                    for (unsigned b = 0; b < q; b++) code = 2 * code + stream_bit(chunk, size_word, big, st.e.bit0 + j * w + lead + b);
                    int v = code - (1 << (q - 1));
                    const bool is_q = st.cplx && ((j & 1u) != 0) != (d.format == GSH_PACKED_QI);
                    if (d.negate & (is_q ? 2 : 1)) v = -v;
                    const unsigned long long at = st.cplx ? (f & ~1ull) + (is_q ? 1 : 0) : f;
                    if (out[at] != static_cast<float>(v)) failures++;
                    checked++;
                }
        }
}
}  // namespace

int main()
{
    for (int size_word : {1, 2, 4, 8})
        for (int big = 0; big < 2; big++)
            for (int head = 0; head < 2; head++)
                for (int w = 1; w <= 16; w++)
                    for (int format = 0; format < 3; format++)
                        {
                            std::vector<gsh_ion_stream> streams;
                            int used = 0;
                            for (int enc = 0; enc <= GSH_ION_OGA; enc++)
                                for (int alignment = 0; alignment < 3; alignment++)
                                    {
                                        if (enc == GSH_ION_SIGN && alignment == 0 && w > 1) continue;
                                        gsh_ion_stream s{};
                                        s.rate_factor = 2 + alignment;
                                        s.packed_bits = w * s.rate_factor * (format ? 2 : 1);
                                        s.quantization = enc == GSH_ION_SIGN ? 1 : alignment == 0 ? w : 1 + (w - 1) * (enc % 3) / 2;
                                        s.encoding = enc;
                                        s.format = format;
                                        s.alignment = alignment;
                                        s.negate = (enc + w) % (format ? 4 : 2);
                                        streams.push_back(s);
                                        used += s.packed_bits;
                                        if (alignment != 0) continue;
                                        gsh_ion_stream skip{};  // 3 bits between the encodings: the next streams start at another bit
                                        skip.packed_bits = 3;
                                        skip.rate_factor = 1;
                                        skip.quantization = 3;
                                        skip.encoding = GSH_ION_OB;
                                        streams.push_back(skip);
                                        used += 3;
                                    }
                            gsh_ion_chunk c{};
                            c.size_word = size_word;
                            c.big_endian = big;
                            c.padding = head;
                            c.count_words = (used + (head ? 5 : 0) + 8 * size_word - 1) / (8 * size_word);
                            c.n_streams = static_cast<int>(streams.size());
                            run({c}, streams, 3);
                        }
    {
        // the largest cycle: one chunk of 512 64-bit words, 16-bit fields across them (a 5-bit stream in front)
        gsh_ion_stream lead{}, big{};
        lead.packed_bits = 5;
        lead.rate_factor = 1;
        lead.quantization = 5;
        lead.encoding = GSH_ION_OB;
        big.packed_bits = 16 * 2 * 1023;
        big.rate_factor = 1023;
        big.quantization = 16;
        big.encoding = GSH_ION_OB;
        big.format = GSH_PACKED_QI;
        gsh_ion_chunk c{};
        c.size_word = 8;
        c.count_words = 512;
        c.n_streams = 2;
        run({c}, {lead, big}, 2);
    }
    if (failures != 0 || checked == 0)
        {
            std::printf("ion decode: %d mismatches over %ld fields\n", failures, checked);
            return 1;
        }
    std::printf("ion decode: ok (%ld fields read bit by bit)\n", checked);
    return 0;
}
