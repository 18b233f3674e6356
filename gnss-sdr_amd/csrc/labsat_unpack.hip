// LabSat 2 / 3, LabSat 3 Wideband and SPIR 1-bit captures -> complex64 (ring positions): the device half of the reference's Labsat_Signal_Source and
// Spir_File_Signal_Source for the register families of packed_registers.h (the decoder, the layout and the reference lines are there).
// Store-bound: a sample costs 4 bytes in at the most (SPIR), 0.53 .. 2 for the LabSat families, and 8 out per RF channel.  So lanes map to OUTPUT samples:
// a lane decodes two adjacent samples and writes them with one 16-byte store (two 8-byte stores where the destination is not 16-byte aligned), a wave
// writes one contiguous run of 1 KiB of ONE destination per store instruction, and the 2 .. 32 lanes whose samples lie in one register load the same
// 8 bytes.  One pass over the registers of a LabSat 3 Wideband block writes up to 3 RF channels, each to a destination of its own, out of that one load.
// A block may start and end inside a register (a ring split at its capacity boundary does): every sample, whole register or not, goes through
// register_decode.  The host splits `first` into a register and an offset inside it and cuts the block into launches of fewer than REG_DIV_LIMIT
// samples, so a lane divides by spr (3, 5, 7, 10, 15, 30 ...) with one 32-bit multiply (register_div) and never in 64 bits.
#include "packed_unpack.h"

namespace gsh
{
namespace
{
constexpr int RG_THREADS = 256;
constexpr int RG_MAX = 3;  // RF channels of a LabSat 3 Wideband register
struct RegisterArgs
{
    const void* src;    // register 0 of the launch: the one that holds its first sample; aligned to the register size
    unsigned off, n;    // the first sample's number inside that register (< spr); samples to write: off + n < REG_DIV_LIMIT
    float qsign;
    int n_sel;
    int ch[RG_MAX];
    float2* dst[RG_MAX];  // dst[i][0] is the launch's first sample of channel ch[i]
};

// REG: the register as it lies in memory (unsigned short, unsigned, unsigned long long)
template <typename REG>
__global__ __launch_bounds__(RG_THREADS) void unpack_register_kernel(RegisterArgs a, PackedCode c)
{
    const unsigned j = 2u * (blockIdx.x * RG_THREADS + threadIdx.x);  // the lane's outputs j, j + 1
    if (j >= a.n) return;
    const bool two = j + 1u < a.n;
    const unsigned spr = static_cast<unsigned>(c.spr);
    const unsigned t = a.off + j;
    const unsigned r0 = register_div(t, c.spr_magic);
    const unsigned i0 = t - r0 * spr;
    const bool wrap = i0 + 1u == spr;  // the second sample opens the next register
    const unsigned i1 = wrap ? 0u : i0 + 1u;
    const REG* src = static_cast<const REG*>(a.src);
    const unsigned long long w0 = src[r0];
    const unsigned long long w1 = (two && wrap) ? static_cast<unsigned long long>(src[r0 + 1u]) : w0;  // (never a register behind the block's last sample)
#pragma unroll
    for (int i = 0; i < RG_MAX; i++)
        if (i < a.n_sel)
            {
                const float2 x0 = register_decode(c, w0, static_cast<int>(i0), a.ch[i]);
                float2* d = a.dst[i] + j;
                if (!two)
                    {
                        d[0] = make_float2(x0.x, a.qsign * x0.y);
                        continue;
                    }
                const float2 x1 = register_decode(c, w1, static_cast<int>(i1), a.ch[i]);
                if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                    *reinterpret_cast<float4*>(d) = make_float4(x0.x, a.qsign * x0.y, x1.x, a.qsign * x1.y);
                else
                    {
                        d[0] = make_float2(x0.x, a.qsign * x0.y);
                        d[1] = make_float2(x1.x, a.qsign * x1.y);
                    }
            }
}
}  // namespace

int register_code(const gsh_packed_format* f, PackedCode* out)
{
    const bool ls3w = packed_ls3w(f->family);
    const char* name = ls3w ? "LabSat 3 Wideband" : f->family == GSH_PACKED_SPIR_1BIT ? "SPIR" : "LabSat 2 / 3";
    const int item = ls3w ? 8 : f->family == GSH_PACKED_SPIR_1BIT ? 4 : 2;
    if (ls3w)
        GSH_REQUIRE((f->reserved & ~1) == 0, "reserved %d: bit 0 (digital I/O recorded) is the only flag of the LabSat 3 Wideband families", f->reserved);
    else
        GSH_REQUIRE(f->reserved == 0, "gsh_packed_format.reserved must be 0");
    GSH_REQUIRE(f->item_size == item, "item_size %d: the %s families read %d-byte little-endian %s (item_size %d)", f->item_size, name, item,
        ls3w ? "registers" : "items", item);
    GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ, "sample_type %d: %s samples are complex, sample_type must be GSH_PACKED_IQ", f->sample_type, name);
    GSH_REQUIRE(f->big_endian_bytes == 0 && f->big_endian_items == 0, "big_endian_bytes %d / big_endian_items %d: the %s families are little-endian, both must be 0",
        f->big_endian_bytes, f->big_endian_items, name);
    PackedCode c{};
    c.family = f->family;
    c.cplx = 1;
    c.item_bytes = 1;
    c.nch = 1;
    c.rbytes = item;
    if (ls3w)
        {
            GSH_REQUIRE(f->rf_channels >= 1 && f->rf_channels <= 3, "rf_channels %d: a LabSat 3 Wideband recording has CHN = 1..3 RF channels", f->rf_channels);
            GSH_REQUIRE(f->channel >= 0 && f->channel < f->rf_channels, "channel %d outside 0..%d (selected_channel - 1 of %d RF channels)", f->channel,
                f->rf_channels - 1, f->rf_channels);
            c.qua = f->family - GSH_PACKED_LS3W_1BIT + 1;
            c.nch = f->rf_channels;
            c.channel = f->channel;
            c.frame_bits = 2 * c.qua * c.nch;
            c.spr = ls3w_samples_per_register(c.qua, c.nch, f->reserved & 1);
            c.spare = 64 - c.spr * c.frame_bits;
        }
    else
        {
            GSH_REQUIRE((f->rf_channels == 0 || f->rf_channels == 1) && f->channel == 0, "rf_channels %d / channel %d: the %s families carry one RF channel",
                f->rf_channels, f->channel, name);
            c.spr = f->family == GSH_PACKED_LABSAT_2BIT ? 8 : f->family == GSH_PACKED_LABSAT_4BIT ? 4 : 1;
            c.qua = f->family == GSH_PACKED_LABSAT_4BIT ? 2 : 1;
            c.frame_bits = 2 * c.qua;
        }
    c.spr_magic = register_div_magic(c.spr);
    *out = c;
    return GSH_OK;
}

int unpack_registers(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
    GSH_REQUIRE(c.rbytes != 0 && n_sel >= 1 && n_sel <= RG_MAX && n_sel <= c.nch, "%d bands of packed family %d", n_sel, c.family);
    GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_src) & static_cast<uintptr_t>(c.rbytes - 1)) == 0, "packed %d-bit %s must be %d-byte aligned", 8 * c.rbytes,
        c.rbytes == 8 ? "registers" : "items", c.rbytes);
    const unsigned long long spr = static_cast<unsigned long long>(c.spr);
    // launches of whole registers' worth of samples, an even count (the pairing of a destination's samples into 16-byte stores carries over), below the
    // bound of the lanes' 32-bit division
    const unsigned long long chunk = (static_cast<unsigned long long>(REG_DIV_LIMIT) / 2ull - 64ull) / (2ull * spr) * (2ull * spr);
    for (unsigned long long done = 0; done < n; done += chunk)
        {
            const unsigned long long at = first + done, len = n - done < chunk ? n - done : chunk;
            const unsigned long long r = at / spr;
            RegisterArgs a{};
            a.src = static_cast<const unsigned char*>(d_src) + r * static_cast<unsigned long long>(c.rbytes);
            a.off = static_cast<unsigned>(at - r * spr);
            a.n = static_cast<unsigned>(len);
            a.qsign = conj ? -1.0f : 1.0f;
            a.n_sel = n_sel;
            for (int i = 0; i < n_sel; i++)
                {
                    a.ch[i] = channels[i];
                    a.dst[i] = d_dst[i] + done;
                }
            const unsigned blocks = static_cast<unsigned>((len + 2ull * RG_THREADS - 1ull) / (2ull * RG_THREADS));
            if (c.rbytes == 8)
                unpack_register_kernel<unsigned long long><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            else if (c.rbytes == 4)
                unpack_register_kernel<unsigned><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            else
                unpack_register_kernel<unsigned short><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            GSH_HIP(hipGetLastError());
        }
    return GSH_OK;
}
}  // namespace gsh
