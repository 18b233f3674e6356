// Packed 2-bit / 4-bit front-end samples -> complex64 (ring positions) or float32 (one RF channel of an IF stream): the device half of the
// reference's signal sources for MAX2769/MAX2771, NT1065, NSR and NTLab captures (packed_unpack.h has the decoder and the reference lines).
// HBM-bound: 1/4 .. 1 byte in per sample, 8 (complex) or 4 (real) out.  Each lane reads one whole dword of packed bytes and writes the 4 .. 16
// floats it expands to with 16-byte stores; the samples in front of the first whole dword and behind the last one (a ring split at its capacity
// boundary starts inside a byte) go one by one through the same decoder, the way convert_kernel treats head, tail and odd alignment.
// The multi-band GSS6450 families go through unpack_fanout_kernel: one pass over the block writes up to 8 bands, each to a destination of its own.
// The register families (LabSat 2 / 3, LabSat 3 Wideband, SPIR: packed_registers.h) are validated and unpacked in labsat_unpack.hip; the entry points
// at the end of this file serve both kinds.
#include "packed_unpack.h"

namespace gsh
{
namespace
{
constexpr int PK_THREADS = 256;

// SPB: samples per byte and RF channel (1, 2, 4); CPLX: complex64 output, else float32.  src is 4-byte aligned; output j is sample first + j.
template <int SPB, bool CPLX>
__global__ __launch_bounds__(PK_THREADS) void unpack_kernel(const unsigned char* __restrict__ src, PackedCode c, unsigned long long first,
    unsigned long long n, float qsign, float* __restrict__ dst)
{
    constexpr int SPW = 4 * SPB;                   // samples per dword
    constexpr int FPS = CPLX ? 2 : 1;              // floats per sample
    constexpr int F4 = SPW * FPS / 4;              // float4 stores per dword
    const unsigned long long end = first + n;
    const unsigned long long w_lo = (first + SPW - 1) / SPW, w_hi = end / SPW;
    const unsigned long long vs = w_lo < w_hi ? w_lo * SPW : end, ve = w_lo < w_hi ? w_hi * SPW : end;  // [vs, ve): whole dwords
    const unsigned long long gid = static_cast<unsigned long long>(blockIdx.x) * PK_THREADS + threadIdx.x;
    const unsigned long long h = vs - first, t = end - ve;
    if (gid < h + t)
        {
            // head / tail: one sample, its byte read on its own (never a dword that reaches outside the block)
            const unsigned long long s = gid < h ? first + gid : ve + (gid - h);
            const float2 x = packed_sample(src, c, s);
            if (CPLX)
                reinterpret_cast<float2*>(dst)[s - first] = make_float2(x.x, qsign * x.y);
            else
                dst[s - first] = x.x;
        }
    if (w_lo >= w_hi) return;
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * PK_THREADS;
    for (unsigned long long w = w_lo + gid; w < w_hi; w += stride)
        {
            const unsigned word = reinterpret_cast<const unsigned*>(src)[w];
            float v[SPW * FPS];
#pragma unroll
            for (int j = 0; j < SPW; j++)
                {
                    const int lb = j / SPB;                          // byte of the dword in stream order
                    const int pb = c.item_bytes == 2 ? lb ^ 1 : lb;  // where it lies (packed_byte_index: swapped short items)
                    const float2 x = packed_decode(c, (word >> (8 * pb)) & 0xffu, j % SPB);
                    if (CPLX)
                        {
                            v[2 * j] = x.x;
                            v[2 * j + 1] = qsign * x.y;
                        }
                    else
                        v[j] = x.x;
                }
            float* d = dst + (w * SPW - first) * FPS;
            if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                {
#pragma unroll
                    for (int k = 0; k < F4; k++) reinterpret_cast<float4*>(d)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
                }
            else if (CPLX)
                {
#pragma unroll
                    for (int k = 0; k < SPW; k++) reinterpret_cast<float2*>(d)[k] = make_float2(v[2 * k], v[2 * k + 1]);
                }
            else
                {
#pragma unroll
                    for (int k = 0; k < SPW; k++) d[k] = v[k];
                }
        }
}

template <int SPB, bool CPLX>
int launch_unpack(const unsigned char* src, const PackedCode& c, unsigned long long first, unsigned long long n, float qsign, float* dst, hipStream_t s)
{
    constexpr unsigned long long SPW = 4 * SPB;
    const unsigned long long w_lo = (first + SPW - 1) / SPW, w_hi = (first + n) / SPW;
    const unsigned long long words = w_lo < w_hi ? w_hi - w_lo : 0ull;
    unsigned long long blocks = (words + PK_THREADS - 1) / PK_THREADS;
    if (blocks < 1) blocks = 1;  // (head and tail samples)
    if (blocks > 256ull * 16ull) blocks = 256ull * 16ull;  // grid-stride beyond 16 work-groups per CU
    unpack_kernel<SPB, CPLX><<<dim3(static_cast<unsigned>(blocks)), dim3(PK_THREADS), 0, s>>>(src, c, first, n, qsign, dst);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

// ---- GSS6450: 32-bit words dealt round-robin over c.nch bands; up to FAN_MAX selected bands leave in one pass, each to its own destination.
// Store mapping: LPW = SPW / 2 adjacent lanes share one word and each stores its own two samples (16 bytes) of the word's 32 / 64 output bytes; a wave
// walks 64 / LPW consecutive words of ONE band, so every store instruction of a wave writes one contiguous run of 1 KiB of one destination (unpack_kernel's
// lane writes its dword's 16-byte pieces 32 / 64 bytes away from its neighbours').  The bands of a tile are loaded first (whole dwords, the lanes of a word
// the same one; the frames of a tile are re-read once per band out of the cache lines the first band brought in), then decoded and stored.
constexpr int FAN_MAX = 8;
struct FanoutArgs
{
    const unsigned* src;  // the packed block, 4-byte aligned, word 0 = band 0's first
    unsigned long long first, n;
    float qsign;
    int n_sel;
    int ch[FAN_MAX];
    float2* dst[FAN_MAX];  // dst[i][0] is sample `first` of band ch[i]
};

template <int ADC_BITS>
__global__ __launch_bounds__(PK_THREADS) void unpack_fanout_kernel(FanoutArgs a, PackedCode c)
{
    constexpr int SPW = 16 / ADC_BITS;  // samples per word: 8 / 4
    constexpr int SPB = SPW / 4;        // samples per byte
    constexpr int LPW = SPW / 2;        // lanes per word
    constexpr int WPI = 64 / LPW;       // words per wave and store instruction
    PackedCode k = c;
    k.family = ADC_BITS == 2 ? GSH_PACKED_GSS6450_2BIT : GSH_PACKED_GSS6450_4BIT;  // (known at compile time: packed_decode folds to one case)
    const unsigned long long first = a.first, end = a.first + a.n;
    const unsigned long long w_lo = (first + SPW - 1) / SPW, w_hi = end / SPW;
    const unsigned long long vs = w_lo < w_hi ? w_lo * SPW : end, ve = w_lo < w_hi ? w_hi * SPW : end;  // [vs, ve): whole words
    const unsigned long long gid = static_cast<unsigned long long>(blockIdx.x) * PK_THREADS + threadIdx.x;
    const unsigned long long h = vs - first, t = end - ve;
    if (gid < h + t)
        {
            // head / tail: one sample of every selected band, its byte read on its own
            const unsigned long long s = gid < h ? first + gid : ve + (gid - h);
#pragma unroll
            for (int i = 0; i < FAN_MAX; i++)
                if (i < a.n_sel)
                    {
                        k.channel = a.ch[i];
                        const float2 x = packed_sample(reinterpret_cast<const unsigned char*>(a.src), k, s);
                        a.dst[i][s - first] = make_float2(x.x, a.qsign * x.y);
                    }
        }
    if (w_lo >= w_hi) return;
    const unsigned lane = threadIdx.x & 63u, sub = lane % LPW, wl = lane / LPW;
    const unsigned long long waves = static_cast<unsigned long long>(gridDim.x) * (PK_THREADS / 64);
    const unsigned long long nch = static_cast<unsigned>(c.nch);
    for (unsigned long long w0 = w_lo + (gid >> 6) * WPI; w0 < w_hi; w0 += waves * WPI)
        {
            const unsigned long long w = w0 + wl;
            if (w >= w_hi) continue;
            unsigned raw[FAN_MAX];
#pragma unroll
            for (int i = 0; i < FAN_MAX; i++)
                if (i < a.n_sel) raw[i] = a.src[w * nch + static_cast<unsigned>(a.ch[i])];
#pragma unroll
            for (int i = 0; i < FAN_MAX; i++)
                if (i < a.n_sel)
                    {
                        const unsigned word = c.swap ? __builtin_bswap32(raw[i]) : raw[i];
                        // the lane's samples 2 sub, 2 sub + 1 of the word; sample j sits in byte 3 - j / SPB of the word's value (packed_byte_index)
                        const int j = 2 * static_cast<int>(sub);
                        const float2 x0 = packed_decode(k, (word >> (8 * (3 - j / SPB))) & 0xffu, j % SPB);
                        const float2 x1 = packed_decode(k, (word >> (8 * (3 - (j + 1) / SPB))) & 0xffu, (j + 1) % SPB);
                        float2* d = a.dst[i] + (w * SPW + j - first);
                        if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                            *reinterpret_cast<float4*>(d) = make_float4(x0.x, a.qsign * x0.y, x1.x, a.qsign * x1.y);
                        else
                            {
                                d[0] = make_float2(x0.x, a.qsign * x0.y);
                                d[1] = make_float2(x1.x, a.qsign * x1.y);
                            }
                    }
        }
}

template <int ADC_BITS>
int launch_fanout(const FanoutArgs& a, const PackedCode& c, hipStream_t s)
{
    constexpr unsigned long long SPW = 16 / ADC_BITS, WPI = 64 / (SPW / 2);
    const unsigned long long w_lo = (a.first + SPW - 1) / SPW, w_hi = (a.first + a.n) / SPW;
    const unsigned long long words = w_lo < w_hi ? w_hi - w_lo : 0ull;
    const unsigned long long tiles = (words + WPI - 1) / WPI;
    unsigned long long blocks = (tiles + PK_THREADS / 64 - 1) / (PK_THREADS / 64);
    if (blocks < 1) blocks = 1;  // (head and tail samples)
    if (blocks > 256ull * 16ull) blocks = 256ull * 16ull;  // grid-stride beyond 16 work-groups per CU
    unpack_fanout_kernel<ADC_BITS><<<dim3(static_cast<unsigned>(blocks)), dim3(PK_THREADS), 0, s>>>(a, c);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace

int packed_code(const gsh_packed_format* f, PackedCode* out)
{
    GSH_REQUIRE(f != nullptr && out != nullptr, "null packed format");
    if ((f->family >= GSH_PACKED_LABSAT_2BIT && f->family <= GSH_PACKED_SPIR_1BIT) || packed_ls4(f->family)) return register_code(f, out);  // (labsat_unpack.hip)
    GSH_REQUIRE(f->reserved == 0, "gsh_packed_format.reserved must be 0");
    const bool gss = f->family == GSH_PACKED_GSS6450_2BIT || f->family == GSH_PACKED_GSS6450_4BIT;
    if (gss)
        GSH_REQUIRE(f->item_size == 4, "item_size %d: the GSS6450 families read 4-byte words (item_size 4)", f->item_size);
    else
        GSH_REQUIRE(f->item_size == 1 || (f->item_size == 2 && f->family == GSH_PACKED_TWO_BIT),
            "item_size %d: 1 (byte), or 2 (short) for GSH_PACKED_TWO_BIT only", f->item_size);
    GSH_REQUIRE((f->big_endian_bytes == 0 || f->big_endian_bytes == 1) && (f->big_endian_items == 0 || f->big_endian_items == 1),
        "big_endian_bytes / big_endian_items must be 0 or 1");
    PackedCode c{};
    c.family = f->family;
    c.item_bytes = 1;
    c.nch = 1;
    switch (f->family)
        {
        case GSH_PACKED_TWO_BIT:
            GSH_REQUIRE(f->sample_type >= GSH_PACKED_REAL && f->sample_type <= GSH_PACKED_QI, "sample_type %d is not real / iq / qi", f->sample_type);
            c.cplx = f->sample_type != GSH_PACKED_REAL;
            c.qi = f->sample_type == GSH_PACKED_QI;
            c.rev = f->big_endian_bytes;
            // short items in little-endian order are read as bytes (two_bit_packed_file_signal_source.cc:63-77)
            c.item_bytes = (f->item_size == 2 && f->big_endian_items) ? 2 : 1;
            c.spb = c.cplx ? 2 : 4;
            break;
        case GSH_PACKED_TWO_BIT_CPX:
            GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ, "GSH_PACKED_TWO_BIT_CPX samples are complex: sample_type must be GSH_PACKED_IQ");
            c.cplx = 1;
            c.spb = 2;
            break;
        case GSH_PACKED_FOUR_BIT_CPX:
            GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ || f->sample_type == GSH_PACKED_QI, "GSH_PACKED_FOUR_BIT_CPX sample_type %d is not iq / qi",
                f->sample_type);
            c.cplx = 1;
            c.qi = f->sample_type == GSH_PACKED_QI;
            c.spb = 1;
            break;
        case GSH_PACKED_NSR:
            GSH_REQUIRE(f->sample_type == GSH_PACKED_REAL, "GSH_PACKED_NSR samples are real: sample_type must be GSH_PACKED_REAL");
            c.spb = 4;
            break;
        case GSH_PACKED_NTLAB:
            GSH_REQUIRE(f->sample_type == GSH_PACKED_REAL, "GSH_PACKED_NTLAB samples are real: sample_type must be GSH_PACKED_REAL");
            // RF_channels 1 and 2 cannot be matched: the reference block loops over noutput_items = (4 / nch) x its input items, reads past its input
            // and overwrites its own outputs (unpack_ntlab_2bit_samples.cc:38,57-77)
            GSH_REQUIRE(f->rf_channels == 4, "NTLab RF_channels %d: only 4 is supported (at 1 and 2 the reference's unpack_ntlab_2bit_samples reads past its input)",
                f->rf_channels);
            GSH_REQUIRE(f->channel >= 0 && f->channel < 4, "NTLab channel %d outside 0..3", f->channel);
            c.channel = f->channel;
            c.spb = 1;
            break;
        case GSH_PACKED_GSS6450_2BIT:
        case GSH_PACKED_GSS6450_4BIT:
            GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ, "GSS6450 samples are complex: sample_type must be GSH_PACKED_IQ");
            GSH_REQUIRE(f->big_endian_bytes == 0, "big_endian_bytes does not apply to the GSS6450 families (`endian` is big_endian_items)");
            GSH_REQUIRE(f->rf_channels >= 0 && f->rf_channels <= 8, "GSS6450 total_channels %d outside 1..8", f->rf_channels);
            c.nch = f->rf_channels == 0 ? 1 : f->rf_channels;
            GSH_REQUIRE(f->channel >= 0 && f->channel < c.nch, "GSS6450 channel %d outside 0..%d", f->channel, c.nch - 1);
            c.cplx = 1;
            c.channel = f->channel;
            c.swap = f->big_endian_items;
            c.item_bytes = 4;
            c.spb = f->family == GSH_PACKED_GSS6450_2BIT ? 2 : 1;
            break;
        default:
            return set_error(GSH_ERR_INVALID, "unknown packed family %d", f->family);
        }
    if (f->family != GSH_PACKED_NTLAB && !gss)
        GSH_REQUIRE((f->rf_channels == 0 || f->rf_channels == 1) && f->channel == 0, "rf_channels %d / channel %d: one RF channel only outside NTLab",
            f->rf_channels, f->channel);
    *out = c;
    return GSH_OK;
}

int packed_size(const PackedCode& c, unsigned long long n, unsigned long long* bytes)
{
    if (c.ls4)
        {
            // whole registers (whole triples at QUA 12) of the selected slot; a count that ends inside a round takes the whole round's bytes
            const unsigned long long unit = static_cast<unsigned long long>(c.spr), S = c.ls4_s;
            GSH_REQUIRE(n % unit == 0, "%llu samples are not a whole number of %s (%d samples of a channel in each)", n,
                c.qua == 12 ? "24-byte triples of registers" : "8-byte registers", c.spr);
            *bytes = (n + S - 1ull) / S * c.ls4_round * 8ull;
            return GSH_OK;
        }
    if (c.rbytes)
        {
            const unsigned long long spr = static_cast<unsigned long long>(c.spr);
            GSH_REQUIRE(n % spr == 0, "%llu samples are not a whole number of %d-byte %s (%d samples per RF channel in each)", n, c.rbytes,
                c.rbytes == 8 ? "registers" : "items", c.spr);
            *bytes = n / spr * static_cast<unsigned long long>(c.rbytes);  // (the RF channels of LabSat 3 Wideband share every register)
            return GSH_OK;
        }
    const unsigned long long per_item = static_cast<unsigned long long>(c.spb) * c.item_bytes;
    GSH_REQUIRE(n % per_item == 0, "%llu samples are not a whole number of input items (%llu samples per %d-byte item)", n, per_item, c.item_bytes);
    *bytes = n / static_cast<unsigned long long>(c.spb) * static_cast<unsigned long long>(c.nch);  // (nch bands share the stream word by word)
    return GSH_OK;
}

int unpack_packed_multi(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
    if (c.rbytes) return unpack_registers(d_src, c, first, n, conj, channels, n_sel, d_dst, s);
    GSH_REQUIRE(packed_multiband(c) && n_sel >= 1 && n_sel <= FAN_MAX && n_sel <= c.nch, "%d bands of packed family %d", n_sel, c.family);
    GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_src) & 3u) == 0, "packed 32-bit words must be 4-byte aligned");
    FanoutArgs a{};
    a.src = static_cast<const unsigned*>(d_src);
    a.first = first;
    a.n = n;
    a.qsign = conj ? -1.0f : 1.0f;
    a.n_sel = n_sel;
    for (int i = 0; i < n_sel; i++)
        {
            a.ch[i] = channels[i];
            a.dst[i] = d_dst[i];
        }
    return c.family == GSH_PACKED_GSS6450_2BIT ? launch_fanout<2>(a, c, s) : launch_fanout<4>(a, c, s);
}

int unpack_packed(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, void* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
    if (packed_multiband(c) || c.rbytes)
        {
            // one band of a multi-band block: the fan-out kernel with a single destination (a register family: its one kernel, labsat_unpack.hip)
            const int ch = c.channel;
            float2* dst = static_cast<float2*>(d_dst);
            return unpack_packed_multi(d_src, c, first, n, conj, &ch, 1, &dst, s);
        }
    // a 4-byte aligned base for the dword loads: the bytes in front of d_src count as samples before `first` (an item boundary for short items)
    const uintptr_t lead = reinterpret_cast<uintptr_t>(d_src) & 3u;
    GSH_REQUIRE(lead % static_cast<uintptr_t>(c.item_bytes) == 0, "packed short items must be 2-byte aligned");
    const unsigned char* base = static_cast<const unsigned char*>(d_src) - lead;
    first += static_cast<unsigned long long>(lead) * static_cast<unsigned long long>(c.spb);
    float* dst = static_cast<float*>(d_dst);
    const float qsign = conj ? -1.0f : 1.0f;
    if (c.cplx) return c.spb == 2 ? launch_unpack<2, true>(base, c, first, n, qsign, dst, s) : launch_unpack<1, true>(base, c, first, n, qsign, dst, s);
    return c.spb == 4 ? launch_unpack<4, false>(base, c, first, n, 1.0f, dst, s) : launch_unpack<1, false>(base, c, first, n, 1.0f, dst, s);
}
}  // namespace gsh

extern "C"
{
    int gsh_packed_bytes(const gsh_packed_format* fmt, uint64_t n_samples, uint64_t* bytes)
    {
        GSH_REQUIRE(bytes != nullptr, "null argument");
        gsh::PackedCode c;
        int rc = gsh::packed_code(fmt, &c);
        if (rc != GSH_OK) return rc;
        unsigned long long b = 0;
        rc = gsh::packed_size(c, n_samples, &b);
        if (rc != GSH_OK) return rc;
        *bytes = b;
        return GSH_OK;
    }

    int gsh_packed_decode_host(const gsh_packed_format* fmt, const void* bytes, uint64_t first_sample, uint64_t n_samples, float* out_iq)
    {
        gsh::PackedCode c;
        int rc = gsh::packed_code(fmt, &c);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(n_samples == 0 || (bytes != nullptr && out_iq != nullptr), "null argument");
        for (uint64_t k = 0; k < n_samples; k++)
            {
                const float2 x = gsh::packed_sample(static_cast<const unsigned char*>(bytes), c, first_sample + k);
                out_iq[2 * k] = x.x;
                out_iq[2 * k + 1] = x.y;
            }
        return GSH_OK;
    }

    int gsh_unpack_device(int device, const gsh_packed_format* fmt, const void* d_src, uint64_t first_sample, uint64_t n_samples, int inverted_spectrum,
        void* d_dst, void* hip_stream)
    {
        gsh::PackedCode c;
        int rc = gsh::packed_code(fmt, &c);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(n_samples == 0 || (d_src != nullptr && d_dst != nullptr), "null argument");
        GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_dst) & (c.cplx ? 7u : 3u)) == 0, "destination must be %d-byte aligned", c.cplx ? 8 : 4);
        GSH_REQUIRE(c.cplx || !inverted_spectrum, "inverted_spectrum applies to complex samples only");
        rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        return gsh::unpack_packed(d_src, c, first_sample, n_samples, inverted_spectrum ? 1 : 0, d_dst, static_cast<hipStream_t>(hip_stream));
    }

    int gsh_unpack_device_multi(int device, const gsh_packed_format* fmt, const void* d_src, uint64_t first_sample, uint64_t n_samples, int inverted_spectrum,
        const int32_t* channels, int n_channels, void* const* d_dst, void* hip_stream)
    {
        gsh::PackedCode c;
        GSH_REQUIRE(fmt != nullptr, "null packed format");
        gsh_packed_format f = *fmt;
        // (LabSat 4: fmt->channel is not consulted either, but the reduced format carries the round geometry of a selected slot: the first one named)
        if (gsh::packed_ls4(f.family) && channels != nullptr && n_channels >= 1) f.channel = channels[0];
        int rc = gsh::packed_code(&f, &c);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(gsh::packed_multiband(c), "packed family %d carries one band: gsh_unpack_device_multi takes the multi-band families (GSS6450)", fmt->family);
        GSH_REQUIRE(channels != nullptr && d_dst != nullptr, "null argument");
        GSH_REQUIRE(n_channels >= 1 && n_channels <= c.nch, "%d bands selected of a stream of %d", n_channels, c.nch);
        int ch[8];
        float2* dst[8];
        for (int i = 0; i < n_channels; i++)
            {
                GSH_REQUIRE(channels[i] >= 0 && channels[i] < c.nch, "band %d outside 0..%d", channels[i], c.nch - 1);
                for (int j = 0; j < i; j++) GSH_REQUIRE(channels[j] != channels[i], "band %d is named twice", channels[i]);
                GSH_REQUIRE(d_dst[i] != nullptr, "null destination for band %d", channels[i]);
                GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_dst[i]) & 7u) == 0, "destination must be 8-byte aligned");
                ch[i] = channels[i];
                dst[i] = static_cast<float2*>(d_dst[i]);
            }
        rc = gsh::ls4_check_channels(c, ch, n_channels);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(n_samples == 0 || d_src != nullptr, "null argument");
        rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        return gsh::unpack_packed_multi(d_src, c, first_sample, n_samples, inverted_spectrum ? 1 : 0, ch, n_channels, dst, static_cast<hipStream_t>(hip_stream));
    }
}
