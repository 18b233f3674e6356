// Packed 2-bit / 4-bit front-end samples (gsh_packed_format, include/gnss_sdr_hip.h): the one decoder that the ring write, the stand-alone unpack
// (packed_unpack.hip) and the packed FIR's load_item (fir_filter.hip) share, so that every path yields the same value for sample k by construction.
// Reference blocks restated (src/algorithms/signal_source/gnuradio_blocks/, "blocks/" below) with the GNU Radio conversion behind each (scale 1).
#ifndef GSH_PACKED_UNPACK_H
#define GSH_PACKED_UNPACK_H
#include "gsh_internal.h"

namespace gsh
{
// a validated gsh_packed_format, reduced to what the decoder needs
struct PackedCode
{
    int family;       // GSH_PACKED_*
    int cplx;         // 1: complex samples (I, Q); 0: real
    int spb;          // samples per byte and RF channel: 4 (2-bit real), 2 (2-bit complex, GSS6450 2-bit), 1 (4-bit complex, NTLab, GSS6450 4-bit)
    int item_bytes;   // bytes per input item: 2 for big-endian short items of TWO_BIT, 4 for the words of GSS6450, else 1
    int rev;          // TWO_BIT big_endian_bytes: sample order within a byte reversed
    int qi;           // TWO_BIT / FOUR_BIT_CPX sample_type qi
    int channel;      // NTLab RF channel; GSS6450: the band of the single-channel calls
    int nch;          // RF channels that share the stream item by item (GSS6450: words dealt round-robin over total_channels bands); else 1
    int swap;         // GSS6450 `endian`: the four bytes of every word are reversed before unpacking
    // the register families (packed_registers.h: LabSat 2 / 3, LabSat 3 Wideband, SPIR); rbytes 0 for every family above, whose spb they leave 0
    int rbytes;       // bytes per little-endian register: 2 (LabSat 2 / 3 item), 4 (SPIR item), 8 (LabSat 3 Wideband)
    int spr;          // samples of one RF channel per register
    int spare;        // unused bits at the top of the register (LabSat 3 Wideband: 64 - spr frame_bits)
    int frame_bits;   // bits from one sample of a channel to the next: SFT = 2 QUA nch (LabSat 3 Wideband)
    int qua;          // bits per I and per Q code (LabSat 3 Wideband: 1 .. 3)
    unsigned spr_magic;  // register_div_magic(spr)
    // LabSat 4 (ls4 = 1, rbytes 8): a block is a run of ROUNDS, each one buffer of registers per recorded channel slot.  spr: samples per register, or per
    // triple of registers at QUA 12 (8); frame_bits = 2 QUA; nch = the slots described.  The arrays are read on the host only (the launcher, the checks).
    int ls4;
    unsigned ls4_s;        // samples of the selected slot per round: its registers x 32 / QUA
    unsigned ls4_round;    // registers per round, every recorded slot together
    unsigned ls4_base;     // register of the round at which the selected slot's buffer starts (ls4_off[channel])
    float ls4_scale;       // 1 / half, half = 2^(QUA - 1)
    unsigned ls4_off[3], ls4_regs[3];
};
__host__ __device__ inline bool packed_ls4(int family) { return family >= GSH_PACKED_LS4_1BIT && family <= GSH_PACKED_LS4_12BIT; }
__host__ __device__ inline bool packed_multiband(const PackedCode& c)
{
    return c.family == GSH_PACKED_GSS6450_2BIT || c.family == GSH_PACKED_GSS6450_4BIT || (c.family >= GSH_PACKED_LS3W_1BIT && c.family <= GSH_PACKED_LS3W_3BIT) ||
           packed_ls4(c.family);
}

// validate *fmt (GSH_ERR_INVALID with a message) and reduce it; the register families are reduced by register_code (labsat_unpack.hip)
int register_code(const gsh_packed_format* fmt, PackedCode* out);
int packed_code(const gsh_packed_format* fmt, PackedCode* out);
// bytes holding n samples; GSH_ERR_INVALID when n is not a whole number of input items
int packed_size(const PackedCode& c, unsigned long long n, unsigned long long* bytes);
// samples [first, first + n) of the packed buffer at d_src -> complex64 at d_dst (conjugated when conj), or float32 at d_dst for a real family
int unpack_packed(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, void* d_dst, hipStream_t s);
// the same for n_sel bands of a multi-band family in one pass over the block: band channels[i] -> complex64 at d_dst[i] (8-byte aligned); the
// caller has validated the list (1 .. 8 distinct bands below c.nch)
int unpack_packed_multi(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s);
// both of the above for a register family (c.rbytes != 0): n_sel = 1 with the code's own channel is the single-destination unpack
int unpack_registers(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s);
// LabSat 4: the slots of one multi call (each below c.nch) are recorded and hold the same number of registers per round; GSH_OK for every other family
int ls4_check_channels(const PackedCode& c, const int* channels, int n_sel);
// alignment that packed_sample needs of a device block's base: the register size of a register family (read as one aligned load), else 1 (byte loads)
inline size_t packed_alignment(const PackedCode& c) { return c.rbytes ? static_cast<size_t>(c.rbytes) : 1; }

// a signed 2-bit field stored the reference's way -- `signed x : 2` assigned (c >> k) & 3 -- wraps in two's complement: 0, 1, -2, -1
// (blocks/unpack_2bit_samples.cc:22-28, unpack_byte_2bit_cpx_samples.cc:26-29,80-89, unpack_byte_2bit_samples.cc:21-24,54-64)
__host__ __device__ __forceinline__ int s2(unsigned v) { return static_cast<int>(v & 1u) - static_cast<int>(v & 2u); }

// byte of the packed stream that holds sample k of the code's RF channel, and the position of the sample inside it
__host__ __device__ __forceinline__ unsigned long long packed_byte_index(const PackedCode& c, unsigned long long k)
{
    const unsigned long long b = k / static_cast<unsigned>(c.spb);
    if (c.item_bytes == 4)
        {
            // GSS6450: byte b of the band's own bytes lies in the band's word b / 4, which is word (b / 4) nch + channel of the stream (deinterleave of
            // 4-byte items, spir_gss6450_file_signal_source.cc:183-233).  Sample 0 sits in the TOP byte of the word's value
            // (blocks/unpack_spir_gss6450_samples.cc:72,101: out[7 - i] / out[3 - i] while the word shifts right): the last byte in memory of a little-endian
            // word, the first one after endian_swap(4).
            const unsigned lb = static_cast<unsigned>(b & 3ull);
            return ((b >> 2) * static_cast<unsigned>(c.nch) + static_cast<unsigned>(c.channel)) * 4ull + (c.swap ? lb : 3u - lb);
        }
    // big_endian_items with short items: the two bytes of each item are swapped before unpacking (blocks/unpack_2bit_samples.cc:63-80,114-115,134-141)
    return c.item_bytes == 2 ? (b ^ 1ull) : b;
}

// sample number `pos` (0 .. spb - 1) of byte `byte` as (I, Q); Q = 0 for the real families
__host__ __device__ __forceinline__ float2 packed_decode(const PackedCode& c, unsigned byte, int pos)
{
    switch (c.family)
        {
        case GSH_PACKED_TWO_BIT:
            {
                // unpack_2bit_samples: 4 values per byte, field f of bits 2f+1:2f, value 2 s + 1 (blocks/unpack_2bit_samples.cc:150-206).  Order
                // of the fields: 0 1 2 3 (:164-177); big_endian_bytes reverses it (3 2 1 0, :152-162); reverse_interleaving (qi) swaps each pair (1 0 3 2,
                // :194-205; with big_endian_bytes 2 3 0 1, :181-191).  Real: value k is sample k (char_to_float); complex: values 2k, 2k+1 are I, Q
                // (interleaved_char_to_complex(false), two_bit_packed_file_signal_source.cc:126-136).
                auto value = [&](int p) {
                    const int f = (c.rev ? 3 - p : p) ^ (c.qi ? 1 : 0);
                    return static_cast<float>(2 * s2(byte >> (2 * f)) + 1);
                };
                if (!c.cplx) return make_float2(value(pos), 0.0f);
                return make_float2(value(2 * pos), value(2 * pos + 1));
            }
        case GSH_PACKED_TWO_BIT_CPX:
            {
                // unpack_byte_2bit_cpx_samples emits bits 5:4, 7:6, 1:0, 3:2 (blocks/unpack_byte_2bit_cpx_samples.cc:77-89, its own I/Q swap);
                // interleaved_short_to_complex(false, true) swaps every pair back (two_bit_cpx_file_signal_source.cc:75): sample 0 = (bits 7:6, bits 5:4),
                // sample 1 = (bits 3:2, bits 1:0)
                const int sh = pos ? 0 : 4;
                return make_float2(static_cast<float>(2 * s2(byte >> (sh + 2)) + 1), static_cast<float>(2 * s2(byte >> sh) + 1));
            }
        case GSH_PACKED_FOUR_BIT_CPX:
            {
                // unpack_byte_4bit_samples: low nibble first, then the high one; a nibble n >= 8 maps to 2 (n - 16) + 1, else 2 n + 1
                // (blocks/unpack_byte_4bit_samples.cc:44-64); interleaved_short_to_complex(false, qi) swaps them for qi (four_bit_cpx_file_signal_source.cc:121)
                const unsigned lo = byte & 15u, hi = (byte >> 4) & 15u;
                const float vlo = static_cast<float>(lo >= 8u ? 2 * (static_cast<int>(lo) - 16) + 1 : 2 * static_cast<int>(lo) + 1);
                const float vhi = static_cast<float>(hi >= 8u ? 2 * (static_cast<int>(hi) - 16) + 1 : 2 * static_cast<int>(hi) + 1);
                return c.qi ? make_float2(vhi, vlo) : make_float2(vlo, vhi);
            }
        case GSH_PACKED_NSR:
            // unpack_byte_2bit_samples: bits 1:0, 3:2, 5:4, 7:6, the signed field itself (-2 .. 1), no 2 s + 1 (blocks/unpack_byte_2bit_samples.cc:50-64)
            return make_float2(static_cast<float>(s2(byte >> (2 * pos))), 0.0f);
        case GSH_PACKED_GSS6450_2BIT:
            {
                // unpack_spir_gss6450_samples, adc_bits 2: one sample per nibble, the high nibble of a byte first; I = bits 1:0 of the nibble, Q = bits 3:2,
                // each the signed field itself (tmp >= 2 -> tmp - 4), no 2 s + 1 (blocks/unpack_spir_gss6450_samples.cc:46-74)
                const unsigned nib = byte >> (pos ? 0 : 4);
                return make_float2(static_cast<float>(s2(nib)), static_cast<float>(s2(nib >> 2)));
            }
        case GSH_PACKED_GSS6450_4BIT:
            {
                // adc_bits 4: one sample per byte, I = low nibble, Q = high nibble, n >= 8 -> n - 16 (blocks/unpack_spir_gss6450_samples.cc:75-103)
                const int lo = static_cast<int>(byte & 15u), hi = static_cast<int>((byte >> 4) & 15u);
                return make_float2(static_cast<float>(lo >= 8 ? lo - 16 : lo), static_cast<float>(hi >= 8 ? hi - 16 : hi));
            }
        default:
            {
                // unpack_ntlab_2bit_samples with 4 channels: channel n reads bits 7-2n (magnitude) and 6-2n (sign), value S ? +mag : -mag, mag M ? 3 : 1
                // (blocks/unpack_ntlab_2bit_samples.cc:57-77)
                const int shift = 2 * (3 - c.channel);
                const int mag = ((byte >> (shift + 1)) & 1u) ? 3 : 1;
                return make_float2(static_cast<float>(((byte >> shift) & 1u) ? mag : -mag), 0.0f);
            }
        }
}

}  // namespace gsh
#include "packed_registers.h"
namespace gsh
{
// sample k of the code's RF channel in the packed buffer `src` (sample 0 = the first of src[0])
__host__ __device__ __forceinline__ float2 packed_sample(const unsigned char* src, const PackedCode& c, unsigned long long k)
{
    if (c.rbytes) return register_sample(src, c, k);
    return packed_decode(c, src[packed_byte_index(c, k)], static_cast<int>(k % static_cast<unsigned>(c.spb)));
}
}  // namespace gsh
#endif
