// ION GNSS SDR metadata standard (ION_GSMS) layouts, gsh_ion_* of include/gnss_sdr_hip.h (the bit stream, the values, the reference lines and the
// deviations are stated there): the descriptor's reduction to a table and the one decoder that the host decode (gsh_ion_decode_host) and the unpack
// kernel (ion_unpack.hip) share, so that both yield the same value for field j of a cycle by construction.  Plain C++ over 32-bit integers: the same
// text compiles for the device, for the host half of the library and -- for tests/host/test_ion_decode.cc, under the address and undefined-behaviour
// sanitizers -- with a host compiler alone.  No table in memory; no shift by a count that can reach the operand's width (every shifted operand is a
// 32-bit unsigned and every count is at most 23).
#ifndef GSH_ION_GSMS_H
#define GSH_ION_GSMS_H
#include "gnss_sdr_hip.h"
#include <cstdio>

#ifdef __HIPCC__
#define GSH_ION_FN __host__ __device__ __forceinline__
#else
#define GSH_ION_FN inline
#endif

namespace gsh
{
// one stream, reduced to what the decoder needs (the kernel takes up to GSH_ION_MAX_SELECTED of these as arguments)
struct IonEntry
{
    unsigned chunk_off;    // the chunk's byte offset in the cycle
    unsigned bit0;         // bit of the chunk's bit stream at which the stream's first field starts (head padding and earlier streams skipped)
    unsigned char xmask;   // stream byte b of the chunk is memory byte b ^ xmask: size_word - 1 for little-endian words, 0 for big-endian ones
    unsigned char w;       // bits of a field (the stride from one field to the next)
    unsigned char cshift;  // the code is (field >> cshift) & (2^q - 1): w - q for alignment left, else 0
    unsigned char q;       // bits of the code: w for alignment 0, else quantization
    unsigned char enc;     // GSH_ION_*
    unsigned char flags;   // bit 0: negate I (or the real value), bit 1: negate Q, bit 2: the first field of a sample is Q (format QI)
    unsigned char pad[2];
};
struct IonStream
{
    IonEntry e;
    unsigned fields;  // fields per cycle: rate_factor, doubled when complex
    int rate, cplx;
};
struct IonLayout
{
    unsigned cycle_bytes, align;  // align: the largest size_word
    int n_streams;
    IonStream s[GSH_ION_MAX_STREAMS];
};

// the descriptor -> *out; GSH_OK, or GSH_ERR_INVALID / GSH_ERR_UNSUPPORTED with the reason in why[n]
inline int ion_reduce(const gsh_ion_chunk* chunks, int n_chunks, const gsh_ion_stream* streams, int n_streams, IonLayout* out, char* why, size_t n)
{
#define GSH_ION_REFUSE(code, ...)            \
    do                                       \
        {                                    \
            std::snprintf(why, n, __VA_ARGS__); \
            return code;                     \
        }                                    \
    while (0)
    if (chunks == nullptr || streams == nullptr || out == nullptr) GSH_ION_REFUSE(GSH_ERR_INVALID, "null argument");
    if (n_chunks < 1 || n_chunks > GSH_ION_MAX_CHUNKS) GSH_ION_REFUSE(GSH_ERR_INVALID, "%d chunks outside 1..%d", n_chunks, GSH_ION_MAX_CHUNKS);
    if (n_streams < 1 || n_streams > GSH_ION_MAX_STREAMS) GSH_ION_REFUSE(GSH_ERR_INVALID, "%d streams outside 1..%d", n_streams, GSH_ION_MAX_STREAMS);
    IonLayout L{};
    L.n_streams = n_streams;
    L.align = 1;
    int at = 0;
    long long cycle = 0;
    for (int c = 0; c < n_chunks; c++)
        {
            const gsh_ion_chunk& k = chunks[c];
            if (k.size_word != 1 && k.size_word != 2 && k.size_word != 4 && k.size_word != 8)
                GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: size_word %d is not 1, 2, 4 or 8 bytes", c, k.size_word);
            if (k.count_words < 1 || k.count_words > GSH_ION_MAX_CYCLE_BYTES) GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: count_words %d outside 1..%d", c, k.count_words, GSH_ION_MAX_CYCLE_BYTES);
            if (k.big_endian != 0 && k.big_endian != 1) GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: big_endian %d is not 0 or 1", c, k.big_endian);
            if (k.padding != 0 && k.padding != 1) GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: padding %d is not 0 (none / tail) or 1 (head)", c, k.padding);
            if (k.shift != 0 && k.shift != 1) GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: shift %d is not 0 (Left) or 1 (Right)", c, k.shift);
            if (k.n_streams < 0 || k.n_streams > n_streams - at)
                GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: n_streams %d, but %d of the %d streams are left", c, k.n_streams, n_streams - at, n_streams);
            const long long chunk_bits = 8ll * k.size_word * k.count_words;
            long long used = 0;
            for (int i = 0; i < k.n_streams; i++)
                {
                    const gsh_ion_stream& s = streams[at + i];
                    const int id = at + i;
                    if (s.format != GSH_PACKED_REAL && s.format != GSH_PACKED_IQ && s.format != GSH_PACKED_QI)
                        GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: format %d is not GSH_PACKED_REAL, _IQ or _QI", id, s.format);
                    const int cplx = s.format != GSH_PACKED_REAL;
                    if (s.rate_factor < 1 || s.rate_factor > 8 * GSH_ION_MAX_CYCLE_BYTES) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: rate_factor %d outside 1..%d", id, s.rate_factor, 8 * GSH_ION_MAX_CYCLE_BYTES);
                    if (s.packed_bits < 1 || s.packed_bits > 8 * GSH_ION_MAX_CYCLE_BYTES) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: packed_bits %d outside 1..%d", id, s.packed_bits, 8 * GSH_ION_MAX_CYCLE_BYTES);
                    const int fields = s.rate_factor * (cplx ? 2 : 1);
                    if (s.packed_bits % fields != 0)
                        GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: packed_bits %d is not a whole number of bits for each of %d %s fields", id, s.packed_bits, fields, cplx ? "complex" : "real");
                    const int w = s.packed_bits / fields;
                    if (w > 16) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: fields of %d bits: 1..16 are built", id, w);
                    if (s.quantization < 1 || s.quantization > w) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: quantization %d outside 1..%d, the bits of a field", id, s.quantization, w);
                    if (s.alignment < 0 || s.alignment > 2) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: alignment %d is not 0 (undefined), 1 (left) or 2 (right)", id, s.alignment);
                    if (s.encoding < 0 || s.encoding > GSH_ION_FP) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: encoding %d outside 0..%d", id, s.encoding, GSH_ION_FP);
                    if (s.lump_shift != 0 && s.lump_shift != 1) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: lump_shift %d is not 0 (Left / undefined) or 1 (Right)", id, s.lump_shift);
                    if (s.negate < 0 || s.negate > (cplx ? 3 : 1)) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: negate %d outside 0..%d", id, s.negate, cplx ? 3 : 1);
                    const int q = s.alignment == 0 ? w : s.quantization;
                    if (s.encoding == GSH_ION_SIGN && q != 1) GSH_ION_REFUSE(GSH_ERR_INVALID, "stream %d: encoding SIGN with a code of %d bits: it has 1", id, q);
                    used += s.packed_bits;
                    if (used > chunk_bits)
                        GSH_ION_REFUSE(GSH_ERR_INVALID, "chunk %d: its streams up to stream %d hold %lld bits, its %d words of %d bytes %lld", c, id, used, k.count_words, k.size_word, chunk_bits);
                }
            const long long pad = chunk_bits - used;
            long long bit = k.padding == 1 ? pad : 0;
            for (int i = 0; i < k.n_streams; i++)
                {
                    const gsh_ion_stream& s = streams[at + i];
                    IonStream& o = L.s[at + i];
                    o.cplx = s.format != GSH_PACKED_REAL;
                    o.rate = s.rate_factor;
                    o.fields = static_cast<unsigned>(s.rate_factor * (o.cplx ? 2 : 1));
                    const int w = s.packed_bits / static_cast<int>(o.fields), q = s.alignment == 0 ? w : s.quantization;
                    o.e.chunk_off = static_cast<unsigned>(cycle);
                    o.e.bit0 = static_cast<unsigned>(bit);
                    o.e.xmask = static_cast<unsigned char>(k.big_endian ? 0 : k.size_word - 1);
                    o.e.w = static_cast<unsigned char>(w);
                    o.e.cshift = static_cast<unsigned char>(s.alignment == 1 ? w - q : 0);
                    o.e.q = static_cast<unsigned char>(q);
                    o.e.enc = static_cast<unsigned char>(s.encoding);
                    o.e.flags = static_cast<unsigned char>(s.negate | (s.format == GSH_PACKED_QI ? 4 : 0));
                    bit += s.packed_bits;
                }
            at += k.n_streams;
            cycle += static_cast<long long>(k.size_word) * k.count_words;
            if (cycle > GSH_ION_MAX_CYCLE_BYTES) GSH_ION_REFUSE(GSH_ERR_INVALID, "a cycle of more than %d bytes (chunks 0..%d hold %lld)", GSH_ION_MAX_CYCLE_BYTES, c, cycle);
            if (static_cast<unsigned>(k.size_word) > L.align) L.align = static_cast<unsigned>(k.size_word);
        }
    if (at != n_streams) GSH_ION_REFUSE(GSH_ERR_INVALID, "the chunks hold %d streams, %d are described", at, n_streams);
    // what is described but not built, after every rule: a descriptor is refused as unsupported only when nothing else is wrong with it
    for (int c = 0; c < n_chunks; c++)
        if (chunks[c].shift == 1) GSH_ION_REFUSE(GSH_ERR_UNSUPPORTED, "chunk %d: word shift Right is not built (the reference starts one word past the buffer there)", c);
    for (int i = 0; i < n_streams; i++)
        {
            if (streams[i].lump_shift == 1) GSH_ION_REFUSE(GSH_ERR_UNSUPPORTED, "stream %d: lump shift Right is not built (the reference writes items count .. 1 there)", i);
            if (streams[i].encoding == GSH_ION_FP) GSH_ION_REFUSE(GSH_ERR_UNSUPPORTED, "stream %d: encoding FP is not built", i);
        }
    L.cycle_bytes = static_cast<unsigned>(cycle);
    *out = L;
    return GSH_OK;
#undef GSH_ION_REFUSE
}

// the value of a code of q bits (1..16) under encoding enc: the closed forms of the header
GSH_ION_FN int ion_value(unsigned enc, unsigned q, unsigned c)
{
    const unsigned top = 1u << (q - 1u);  // the code's leading bit
    if (enc == GSH_ION_OG || enc == GSH_ION_OGA)
        {
            c ^= c >> 1;  // Gray -> binary: bit i becomes the parity of bits i .. 15
            c ^= c >> 2;
            c ^= c >> 4;
            c ^= c >> 8;
        }
    const int ic = static_cast<int>(c), itop = static_cast<int>(top);
    switch (enc)
        {
        case GSH_ION_OB:
        case GSH_ION_OG:
            return ic - itop;
        case GSH_ION_OBA:
        case GSH_ION_OGA:
            return 2 * ic - (2 * itop - 1);
        case GSH_ION_TC:
            return (c & top) ? ic - 2 * itop : ic;
        case GSH_ION_TCA:
            return 2 * ((c & top) ? ic - 2 * itop : ic) + 1;
        case GSH_ION_SM:
            {
                const int m = static_cast<int>(c & (top - 1u));
                return (c & top) ? -m : m;
            }
        case GSH_ION_SMA:
            {
                const int m = 2 * static_cast<int>(c & (top - 1u)) + 1;
                return (c & top) ? -m : m;
            }
        case GSH_ION_MS:
            {
                const int m = static_cast<int>(c >> 1);
                return (c & 1u) ? -m : m;
            }
        case GSH_ION_MSA:
            {
                const int m = 2 * static_cast<int>(c >> 1) + 1;
                return (c & 1u) ? -m : m;
            }
        default:  // SIGN, q = 1
            return (c & 1u) ? -1 : 1;
        }
}

// field j (0 .. fields - 1) of the stream in one cycle as its value, `negate` not applied.  byte_at(i) is memory byte i of the CYCLE.  A field of at
// most 16 bits at bit o (0..7) of stream byte b lies in bytes b .. b + 2: they are read only as far as the field reaches, so never past the chunk.
template <typename BYTE_AT>
GSH_ION_FN int ion_field_value(const IonEntry& e, unsigned j, const BYTE_AT& byte_at)
{
    const unsigned w = e.w, bit = e.bit0 + j * w, b = bit >> 3, o = bit & 7u, end = o + w;  // end <= 23
    const unsigned x = e.xmask;
    unsigned v = static_cast<unsigned>(byte_at(e.chunk_off + (b ^ x))) << 16;
    if (end > 8u) v |= static_cast<unsigned>(byte_at(e.chunk_off + ((b + 1u) ^ x))) << 8;
    if (end > 16u) v |= static_cast<unsigned>(byte_at(e.chunk_off + ((b + 2u) ^ x)));
    const unsigned field = (v >> (24u - end)) & ((1u << w) - 1u);
    const unsigned code = (field >> e.cshift) & ((1u << e.q) - 1u);
    return ion_value(e.enc, e.q, code);
}

// fields [first, first + n) of the stream, counted from the start of the block `bytes` (cycle 0 at its first byte), as floats in OUTPUT order: for a
// complex stream field 2k, 2k + 1 are I and Q of sample k, or Q and I when the format is QI (first and n are even then)
inline void ion_decode_fields(const IonLayout& L, int stream, const unsigned char* bytes, unsigned long long first, unsigned long long n, float* out)
{
    const IonStream& s = L.s[stream];
    for (unsigned long long i = 0; i < n; i++)
        {
            const unsigned long long f = first + i, cycle = f / s.fields;
            const unsigned j = static_cast<unsigned>(f - cycle * s.fields);
            const unsigned char* p = bytes + cycle * L.cycle_bytes;
            int v = ion_field_value(s.e, j, [p](unsigned k) { return p[k]; });
            const bool is_q = s.cplx && (((j & 1u) != 0) != ((s.e.flags & 4) != 0));
            if (s.e.flags & (is_q ? 2 : 1)) v = -v;
            const unsigned long long at = s.cplx ? (i & ~1ull) + (is_q ? 1u : 0u) : i;
            out[at] = static_cast<float>(v);
        }
}
}  // namespace gsh
#endif
