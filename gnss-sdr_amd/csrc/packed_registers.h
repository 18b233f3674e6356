// Register-oriented packed families (included by packed_unpack.h behind PackedCode): LabSat 2 / 3, LabSat 3 Wideband and SPIR 1-bit captures.  The byte
// decoder of packed_unpack.h counts samples per BYTE; these formats pack spr samples into a little-endian REGISTER of rbytes bytes, with `spare` unused
// bits at its top and fields that straddle bytes.  One decoder, register_decode, maps (register value, code, sample in register, RF channel) to (I, Q);
// the host decode, the unpack kernels (labsat_unpack.hip), the packed FIR and the conditioner all reach it, the last three through packed_sample.
// The 16-bit items of LabSat 2 / 3 and the 32-bit items of SPIR go through it as registers of 16 and 32 bits (spare 0), not through the byte decoder.
// Reference (src/algorithms/signal_source/gnuradio_blocks/, "blocks/" below): labsat23_source.cc, unpack_intspir_1bit_samples.cc.
// LabSat 4 is the one family here that is NOT a run of equal registers: see "LabSat 4" below.
//
// DEVIATION from the reference as compiled, LabSat 3 Wideband only: extract_bits (blocks/labsat23_source.cc:67-74) indexes bs[64 - start - i + 1], bit
// 65 - start - i of the 64-bit std::bitset: outside the bitset for offsets 0 and 1 (undefined behaviour) and elsewhere two bits above the position the
// surrounding code implies (:1039 "Earlier samples are written in the MSBs", the spare bits counted from the top at :944-948, the LabSat 4 path that
// takes "48 MSBs" with offsets 0 and 24).  Here bit i of a field that starts at offset `start` is bit 63 - start - i.
#ifndef GSH_PACKED_REGISTERS_H
#define GSH_PACKED_REGISTERS_H

namespace gsh
{
__host__ __device__ inline bool packed_ls3w(int family) { return family >= GSH_PACKED_LS3W_1BIT && family <= GSH_PACKED_LS3W_3BIT; }

// samples per 64-bit LabSat 3 Wideband register (number_of_samples_per_ls3w_register, blocks/labsat23_source.cc:954-1034); 0: no such layout
inline int ls3w_samples_per_register(int qua, int chn, int digital_io)
{
    static const int plain[3][3] = {{32, 16, 10}, {16, 8, 5}, {10, 5, 3}}, dio[3][3] = {{30, 15, 10}, {15, 7, 5}, {10, 5, 3}};
    if (qua < 1 || qua > 3 || chn < 1 || chn > 3) return 0;
    return (digital_io ? dio : plain)[qua - 1][chn - 1];
}

// q = t / d for t < REG_DIV_LIMIT with m = 2^32 / d + 1 (integer division): the high word of t m.  With e = m d - 2^32 (0 < e <= d <= 32) the product's
// high word is floor(t / d + t e / (2^32 d)), and t e < 2^32 keeps the second term below 1 / d: exact for t < 2^27.  The launcher cuts a block into
// launches below that, so a lane divides in 32 bits and never in 64.
constexpr unsigned REG_DIV_LIMIT = 1u << 27;
// d = 1 (SPIR) has no such m in 32 bits: its magic is 0 and the quotient is t itself.
inline unsigned register_div_magic(int d) { return d == 1 ? 0u : static_cast<unsigned>((1ull << 32) / static_cast<unsigned>(d)) + 1u; }
__host__ __device__ __forceinline__ unsigned register_div(unsigned t, unsigned magic)
{
    if (magic == 0u) return t;
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(t, magic);
#else
    return static_cast<unsigned>((static_cast<unsigned long long>(t) * magic) >> 32);
#endif
}

// sample i (0 .. spr - 1) of RF channel ch in the register value `reg` (its rbytes bytes read little-endian) as (I, Q)
__host__ __device__ __forceinline__ float2 register_decode(const PackedCode& c, unsigned long long reg, int i, int ch)
{
    switch (c.family)
        {
        case GSH_PACKED_LABSAT_2BIT:
            {
                // decode_samples_one_channel, 2 bits per sample: 8 samples per 16-bit item, sample i has I = bit 15 - 2i, Q = bit 14 - 2i, value 2 b - 1
                // (blocks/labsat23_source.cc:586-658)
                const unsigned f = static_cast<unsigned>(reg) >> (14 - 2 * i);
                return make_float2(static_cast<float>(2 * static_cast<int>((f >> 1) & 1u) - 1), static_cast<float>(2 * static_cast<int>(f & 1u) - 1));
            }
        case GSH_PACKED_LABSAT_4BIT:
            {
                // 4 bits per sample: 4 samples per item, sample i has I sign = bit 15 - 4i, Q sign = bit 14 - 4i, I magnitude = bit 13 - 4i, Q magnitude =
                // bit 12 - 4i; (sign, magnitude) 00 -> +1, 01 -> +2, 11 -> -1, 10 -> -2: the two's complement field, plus 1 when it is not negative
                const unsigned f = static_cast<unsigned>(reg) >> (12 - 4 * i);
                const int si = static_cast<int>((f >> 3) & 1u), sq = static_cast<int>((f >> 2) & 1u);
                const int mi = static_cast<int>((f >> 1) & 1u), mq = static_cast<int>(f & 1u);
                return make_float2(static_cast<float>(mi - 2 * si + 1 - si), static_cast<float>(mq - 2 * sq + 1 - sq));
            }
        case GSH_PACKED_SPIR_1BIT:
            // unpack_intspir_1bit_samples with channel 1: I = bit 0, Q = bit 1 of the 32-bit item, +-32767 (blocks/unpack_intspir_1bit_samples.cc:36-68)
            return make_float2((reg & 1ull) ? 32767.0f : -32767.0f, (reg & 2ull) ? 32767.0f : -32767.0f);
        default:
            {
                // LabSat 3 Wideband: sample i of channel ch starts o = spare + i SFT + 2 QUA ch bits below the register's top (blocks/labsat23_source.cc:
                // 944-948,1037-1053); the I code is its first QUA bits, most significant first, the Q code the next QUA (bit 63 - start - i: see the
                // deviation above).  generate_mapping (:43-62): code < half -> (code + 1) / half, else (code - 2^QUA) / half, half = 2^(QUA - 1).
                const int qua = c.qua;
                const int o = c.spare + i * c.frame_bits + 2 * qua * ch;
                const unsigned f = static_cast<unsigned>(reg >> (64 - o - 2 * qua));  // (o + 2 QUA <= 64: the field lies inside the register)
                const int mask = (1 << qua) - 1, half = 1 << (qua - 1);
                const int ci = static_cast<int>(f >> qua) & mask, cq = static_cast<int>(f) & mask;
                const float scale = qua == 1 ? 1.0f : qua == 2 ? 0.5f : 0.25f;
                return make_float2(static_cast<float>(ci < half ? ci + 1 : ci - 2 * half) * scale, static_cast<float>(cq < half ? cq + 1 : cq - 2 * half) * scale);
            }
        }
}

// register r of the packed buffer at src (aligned to c.rbytes on the device: the entry points refuse any other base)
__host__ __device__ __forceinline__ unsigned long long register_load(const unsigned char* src, const PackedCode& c, unsigned long long r)
{
#ifdef __HIP_DEVICE_COMPILE__
    if (c.rbytes == 8) return reinterpret_cast<const unsigned long long*>(src)[r];
    if (c.rbytes == 4) return reinterpret_cast<const unsigned*>(src)[r];
    return reinterpret_cast<const unsigned short*>(src)[r];
#else
    unsigned long long v = 0;  // (host memory of any alignment, little-endian by construction)
    for (int b = 0; b < c.rbytes; b++) v |= static_cast<unsigned long long>(src[r * static_cast<unsigned>(c.rbytes) + b]) << (8 * b);
    return v;
#endif
}

// LabSat 4 (blocks/labsat23_source.cc:92-121 write_samples_ls4, :1262-1301 read_ls4_data / parse_ls4_data).  A block is a run of ROUNDS; a round holds one
// buffer of regs[s] 64-bit little-endian registers per recorded channel slot s, in the order A, B, C, and the buffers may differ in size.  Inside one
// buffer the registers form ONE bit stream, register 0 first and each register from its top bit down: sample j of the round starts at bit 2 QUA j, the
// I code is its first QUA bits (most significant first) and the Q code the next QUA.  For QUA 1, 2, 4, 8 a field never leaves its register; at QUA 12
// three registers hold 8 samples and samples 2 and 5 of such a triple straddle two registers (regs is a multiple of 3, so never the buffer's end).
// ls4_field: the 2 QUA bits that start `o` bits below the top of `lo` and run on into the top of `hi` (read only when o + bits > 64).
__host__ __device__ __forceinline__ unsigned ls4_field(unsigned long long lo, unsigned long long hi, unsigned o, unsigned bits)
{
    const unsigned end = o + bits;
    const unsigned long long v = end <= 64u ? lo >> (64u - end) : (lo << (end - 64u)) | (hi >> (128u - end));
    return static_cast<unsigned>(v) & ((1u << bits) - 1u);
}
// generate_mapping (:43-62) on both codes of a field: code < half -> (code + 1) / half, else (code - 2^QUA) / half; scale = 1 / half is a power of two
__host__ __device__ __forceinline__ float2 ls4_value(unsigned f, int qua, float scale)
{
    const int mask = (1 << qua) - 1, half = 1 << (qua - 1);
    const int ci = static_cast<int>(f >> qua) & mask, cq = static_cast<int>(f) & mask;
    return make_float2(static_cast<float>(ci < half ? ci + 1 : ci - 2 * half) * scale, static_cast<float>(cq < half ? cq + 1 : cq - 2 * half) * scale);
}

// sample k of the code's RF channel: the register families' half of packed_sample
__host__ __device__ __forceinline__ float2 register_sample(const unsigned char* src, const PackedCode& c, unsigned long long k)
{
    if (c.ls4)
        {
            const unsigned long long round = k / c.ls4_s;
            const unsigned b = static_cast<unsigned>(k - round * c.ls4_s) * static_cast<unsigned>(c.frame_bits), o = b & 63u;
            const unsigned long long r = round * c.ls4_round + c.ls4_base + (b >> 6);
            const unsigned long long lo = register_load(src, c, r);
            const unsigned long long hi = o + static_cast<unsigned>(c.frame_bits) > 64u ? register_load(src, c, r + 1ull) : 0ull;
            return ls4_value(ls4_field(lo, hi, o, static_cast<unsigned>(c.frame_bits)), c.qua, c.ls4_scale);
        }
    const unsigned long long r = k / static_cast<unsigned>(c.spr);
    return register_decode(c, register_load(src, c, r), static_cast<int>(k - r * static_cast<unsigned>(c.spr)), c.channel);
}
}  // namespace gsh
#endif
