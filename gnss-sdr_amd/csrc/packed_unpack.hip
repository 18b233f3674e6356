// Packed 2-bit / 4-bit front-end samples -> complex64 (ring positions) or float32 (one RF channel of an IF stream): the device half of the
// reference's signal sources for MAX2769/MAX2771, NT1065, NSR and NTLab captures (packed_unpack.h has the decoder and the reference lines).
// HBM-bound: 1/4 .. 1 byte in per sample, 8 (complex) or 4 (real) out.  Each lane reads one whole dword of packed bytes and writes the 4 .. 16
// floats it expands to with 16-byte stores; the samples in front of the first whole dword and behind the last one (a ring split at its capacity
// boundary starts inside a byte) go one by one through the same decoder, the way convert_kernel treats head, tail and odd alignment.
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
}  // namespace

int packed_code(const gsh_packed_format* f, PackedCode* out)
{
    GSH_REQUIRE(f != nullptr && out != nullptr, "null packed format");
    GSH_REQUIRE(f->reserved == 0, "gsh_packed_format.reserved must be 0");
    GSH_REQUIRE(f->item_size == 1 || (f->item_size == 2 && f->family == GSH_PACKED_TWO_BIT),
        "item_size %d: 1 (byte), or 2 (short) for GSH_PACKED_TWO_BIT only", f->item_size);
    GSH_REQUIRE((f->big_endian_bytes == 0 || f->big_endian_bytes == 1) && (f->big_endian_items == 0 || f->big_endian_items == 1),
        "big_endian_bytes / big_endian_items must be 0 or 1");
    PackedCode c{};
    c.family = f->family;
    c.item_bytes = 1;
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
        default:
            return set_error(GSH_ERR_INVALID, "unknown packed family %d", f->family);
        }
    if (f->family != GSH_PACKED_NTLAB)
        GSH_REQUIRE((f->rf_channels == 0 || f->rf_channels == 1) && f->channel == 0, "rf_channels %d / channel %d: one RF channel only outside NTLab",
            f->rf_channels, f->channel);
    *out = c;
    return GSH_OK;
}

int packed_size(const PackedCode& c, unsigned long long n, unsigned long long* bytes)
{
    const unsigned long long per_item = static_cast<unsigned long long>(c.spb) * c.item_bytes;
    GSH_REQUIRE(n % per_item == 0, "%llu samples are not a whole number of input items (%llu samples per %d-byte item)", n, per_item, c.item_bytes);
    *bytes = n / static_cast<unsigned long long>(c.spb);
    return GSH_OK;
}

int unpack_packed(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, void* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
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
}
