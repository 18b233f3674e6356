// ION_GSMS recordings -> complex64 (ring positions) or float32: the layout object gsh_ion_layout_t and the device half of the reference's
// ION_GSMS_Signal_Source (the layout, the values and the deviations: include/gnss_sdr_hip.h; the decoder: ion_gsms.h).
// One kernel for every layout, driven by a table of up to 8 entries (one per selected stream) that travels as kernel arguments.  The unit of work is
// the FIELD: a real sample is one field and one float, a complex sample two of each, so a run of 4 fields of a stream is 16 bytes of its destination
// whichever it is.  A work-group takes `group` consecutive floats of every destination (a multiple of 4, up to 4096), stages the whole cycles that
// hold them into LDS with 16-byte loads -- the block is read once from memory however many streams are selected, and nothing outside the cycles the
// launch touches -- and then each lane gathers 4 adjacent fields per selected stream out of LDS byte by byte (a field of <= 16 bits touches at most
// three stream bytes; stream byte b is chunk byte b ^ xmask) and writes them with one 16-byte store where the destination is 16-byte aligned, with
// 8- or 4-byte stores where it is not and at the end of a segment.  A lane divides a field number below 2^17 by the fields per cycle with one 32-bit
// multiply (register_div); a work-group divides once more, in 32 bits, to find its first cycle; the host cuts the block into launches in 64 bits.
#include "ion_layout.h"
#include "packed_unpack.h"
#include <algorithm>
#include <new>

namespace gsh
{
namespace
{
constexpr int ION_THREADS = 256;
constexpr unsigned ION_TILE_BYTES = 16384;  // whole cycles one work-group stages (>= 4 cycles of GSH_ION_MAX_CYCLE_BYTES)
constexpr unsigned ION_GROUP_MAX = 4096;    // floats of one destination per work-group at the most: 4 runs of 4 per lane
static_assert(ION_TILE_BYTES >= 4 * GSH_ION_MAX_CYCLE_BYTES, "4 fields of a stream may lie in 4 cycles");

struct IonArgs
{
    const unsigned char* src;  // cycle 0 of the launch: the one that holds its first field
    unsigned foff, nf;         // the first field's number inside that cycle (< fields); floats to write per stream (< 2^28)
    unsigned fields, magic;    // fields of a selected stream per cycle (the same for all of them) and register_div_magic of it
    unsigned cycle_bytes;
    unsigned group;            // floats per work-group and stream: a multiple of 4 whose cycles fit ION_TILE_BYTES wherever the run starts
    int cplx;
    float qsign;
    int n_sel;
    IonEntry e[GSH_ION_MAX_SELECTED];
    float* dst[GSH_ION_MAX_SELECTED];  // dst[i][0] is the launch's first float of that stream
};

struct LdsCycle
{
    const unsigned char* p;  // byte 0 of the cycle in LDS
    __device__ __forceinline__ unsigned operator()(unsigned k) const { return p[k]; }
};

__global__ __launch_bounds__(ION_THREADS) void unpack_ion_kernel(IonArgs a)
{
    __shared__ uint4 tile[ION_TILE_BYTES / 16 + 1];  // (+ 1: the tile keeps the source's position inside a 16-byte line)
    const unsigned u0 = blockIdx.x * a.group, u1 = min(u0 + a.group, a.nf);  // the work-group's floats [u0, u1) of every destination
    const unsigned cyc0 = (a.foff + u0) / a.fields, cyc_last = (a.foff + u1 - 1u) / a.fields;
    const unsigned len = (cyc_last - cyc0 + 1u) * a.cycle_bytes;  // <= ION_TILE_BYTES (the launcher's choice of group)
    const unsigned char* g = a.src + static_cast<unsigned long long>(cyc0) * a.cycle_bytes;
    const unsigned m = static_cast<unsigned>(reinterpret_cast<uintptr_t>(g) & 15u);
    unsigned char* lds = reinterpret_cast<unsigned char*>(tile);  // byte i of the staged cycles is lds[m + i]
    for (unsigned k = threadIdx.x; 16u * k < m + len; k += ION_THREADS)
        {
            const int lo = static_cast<int>(16u * k) - static_cast<int>(m);  // the line's first byte, counted from g
            if (lo >= 0 && static_cast<unsigned>(lo) + 16u <= len)
                tile[k] = *reinterpret_cast<const uint4*>(g + lo);
            else  // the first and the last line: only the bytes of the staged cycles
                for (int b = 0; b < 16; b++)
                    if (lo + b >= 0 && static_cast<unsigned>(lo + b) < len) lds[16u * k + static_cast<unsigned>(b)] = g[lo + b];
        }
    __syncthreads();
    const unsigned e0 = a.foff + u0 - cyc0 * a.fields, span = u1 - u0;  // the work-group's first field inside its first staged cycle
    for (unsigned r = 4u * threadIdx.x; r < span; r += 4u * ION_THREADS)
        {
            const unsigned cnt = min(4u, span - r);  // (complex: 2 or 4, foff and nf are even)
            unsigned c = register_div(e0 + r, a.magic), j = e0 + r - c * a.fields;
            unsigned at[4], fj[4];  // the lane's fields: the cycle's place in LDS, the field's number in the cycle
#pragma unroll
            for (int k = 0; k < 4; k++)
                {
                    at[k] = m + c * a.cycle_bytes;
                    fj[k] = j;
                    if (++j == a.fields)
                        {
                            j = 0;
                            c++;
                        }
                }
#pragma unroll
            for (int i = 0; i < GSH_ION_MAX_SELECTED; i++)
                if (i < a.n_sel)
                    {
                        const IonEntry e = a.e[i];
                        int v[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) v[k] = static_cast<unsigned>(k) < cnt ? ion_field_value(e, fj[k], LdsCycle{lds + at[k]}) : 0;
                        float x[4];
                        if (a.cplx)
                            {
                                const bool qi = (e.flags & 4) != 0;
                                const int i0 = qi ? v[1] : v[0], q0 = qi ? v[0] : v[1], i1 = qi ? v[3] : v[2], q1 = qi ? v[2] : v[3];
                                x[0] = static_cast<float>((e.flags & 1) ? -i0 : i0);
                                x[1] = a.qsign * static_cast<float>((e.flags & 2) ? -q0 : q0);
                                x[2] = static_cast<float>((e.flags & 1) ? -i1 : i1);
                                x[3] = a.qsign * static_cast<float>((e.flags & 2) ? -q1 : q1);
                            }
                        else
                            {
#pragma unroll
                                for (int k = 0; k < 4; k++) x[k] = static_cast<float>((e.flags & 1) ? -v[k] : v[k]);
                            }
                        float* d = a.dst[i] + u0 + r;
                        if (cnt == 4u && (reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                            *reinterpret_cast<float4*>(d) = make_float4(x[0], x[1], x[2], x[3]);
                        else if (a.cplx)
                            {
                                *reinterpret_cast<float2*>(d) = make_float2(x[0], x[1]);
                                if (cnt == 4u) *reinterpret_cast<float2*>(d + 2) = make_float2(x[2], x[3]);
                            }
                        else
                            {
#pragma unroll
                                for (int k = 0; k < 4; k++)
                                    if (static_cast<unsigned>(k) < cnt) d[k] = x[k];
                            }
                    }
        }
}
}  // namespace

int ion_check_streams(const gsh_ion_layout* layout, const int32_t* streams, int n_streams, int* cplx, int* rate)
{
    GSH_REQUIRE(layout != nullptr && streams != nullptr, "null argument");
    GSH_REQUIRE(n_streams >= 1 && n_streams <= GSH_ION_MAX_SELECTED, "%d streams selected: one call takes 1..%d", n_streams, GSH_ION_MAX_SELECTED);
    const IonLayout& L = layout->l;
    for (int i = 0; i < n_streams; i++)
        {
            GSH_REQUIRE(streams[i] >= 0 && streams[i] < L.n_streams, "stream %d outside 0..%d", streams[i], L.n_streams - 1);
            for (int j = 0; j < i; j++) GSH_REQUIRE(streams[j] != streams[i], "stream %d is named twice", streams[i]);
            const IonStream &s = L.s[streams[i]], &s0 = L.s[streams[0]];
            GSH_REQUIRE(s.cplx == s0.cplx, "streams %d and %d are %s and %s: the streams of one call are all complex or all real (select them in separate calls)",
                streams[0], streams[i], s0.cplx ? "complex" : "real", s.cplx ? "complex" : "real");
            GSH_REQUIRE(s.rate == s0.rate, "streams %d and %d hold %d and %d samples per cycle: the streams of one call must have the same rate (select them in separate calls)",
                streams[0], streams[i], s0.rate, s.rate);
        }
    *cplx = L.s[streams[0]].cplx;
    *rate = L.s[streams[0]].rate;
    return GSH_OK;
}

int ion_unpack(const gsh_ion_layout* layout, const void* d_src, unsigned long long first, unsigned long long n, int conj, const int32_t* streams,
    int n_streams, void* const* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
    const IonLayout& L = layout->l;
    const IonStream& s0 = L.s[streams[0]];
    const unsigned long long rate = static_cast<unsigned long long>(s0.rate), per = s0.cplx ? 2ull : 1ull;
    IonArgs a{};
    a.fields = s0.fields;
    a.magic = register_div_magic(static_cast<int>(s0.fields));
    a.cycle_bytes = L.cycle_bytes;
    a.cplx = s0.cplx;
    a.qsign = conj ? -1.0f : 1.0f;
    a.n_sel = n_streams;
    for (int i = 0; i < n_streams; i++) a.e[i] = L.s[streams[i]].e;
    // g consecutive fields touch (g + fields - 2) / fields + 1 cycles at the most: the largest multiple of 4 whose cycles fit the tile (>= 4)
    const unsigned long long cycles = ION_TILE_BYTES / L.cycle_bytes;
    a.group = static_cast<unsigned>(std::min<unsigned long long>(ION_GROUP_MAX, ((cycles - 1ull) * s0.fields + 1ull) & ~3ull));
    // launches of 2^26 samples: a multiple of 4 floats (the pairing into 16-byte stores carries over), field numbers far inside 32 bits
    const unsigned long long chunk = 1ull << 26;
    for (unsigned long long done = 0; done < n; done += chunk)
        {
            const unsigned long long at = first + done, len = std::min(n - done, chunk), cycle = at / rate;
            a.src = static_cast<const unsigned char*>(d_src) + cycle * L.cycle_bytes;
            a.foff = static_cast<unsigned>((at - cycle * rate) * per);
            a.nf = static_cast<unsigned>(len * per);
            for (int i = 0; i < n_streams; i++) a.dst[i] = static_cast<float*>(d_dst[i]) + done * per;
            const unsigned blocks = (a.nf + a.group - 1u) / a.group;
            unpack_ion_kernel<<<dim3(blocks), dim3(ION_THREADS), 0, s>>>(a);
            GSH_HIP(hipGetLastError());
        }
    return GSH_OK;
}
}  // namespace gsh

extern "C"
{
    int gsh_ion_layout_create(const gsh_ion_chunk* chunks, int n_chunks, const gsh_ion_stream* streams, int n_streams, gsh_ion_layout_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null argument");
        *out = nullptr;
        gsh_ion_layout* l = new (std::nothrow) gsh_ion_layout{};
        GSH_REQUIRE(l != nullptr, "out of memory");
        char why[256] = "";
        const int rc = gsh::ion_reduce(chunks, n_chunks, streams, n_streams, &l->l, why, sizeof(why));
        if (rc != GSH_OK)
            {
                delete l;
                return gsh::set_error(rc, "%s", why);
            }
        *out = l;
        return GSH_OK;
    }

    void gsh_ion_layout_destroy(gsh_ion_layout_t* layout) { delete layout; }

    int gsh_ion_layout_info(const gsh_ion_layout_t* layout, uint32_t* cycle_bytes, int32_t* n_streams)
    {
        GSH_REQUIRE(layout != nullptr, "null layout");
        if (cycle_bytes) *cycle_bytes = layout->l.cycle_bytes;
        if (n_streams) *n_streams = layout->l.n_streams;
        return GSH_OK;
    }

    int gsh_ion_stream_info(const gsh_ion_layout_t* layout, int stream, int32_t* samples_per_cycle, int32_t* is_complex, int32_t* field_bits)
    {
        GSH_REQUIRE(layout != nullptr, "null layout");
        GSH_REQUIRE(stream >= 0 && stream < layout->l.n_streams, "stream %d outside 0..%d", stream, layout->l.n_streams - 1);
        const gsh::IonStream& s = layout->l.s[stream];
        if (samples_per_cycle) *samples_per_cycle = s.rate;
        if (is_complex) *is_complex = s.cplx;
        if (field_bits) *field_bits = s.e.w;
        return GSH_OK;
    }

    int gsh_ion_bytes(const gsh_ion_layout_t* layout, int stream, uint64_t n_samples, uint64_t* bytes)
    {
        GSH_REQUIRE(layout != nullptr && bytes != nullptr, "null argument");
        GSH_REQUIRE(stream >= 0 && stream < layout->l.n_streams, "stream %d outside 0..%d", stream, layout->l.n_streams - 1);
        const uint64_t rate = static_cast<uint64_t>(layout->l.s[stream].rate);
        *bytes = (n_samples / rate + (n_samples % rate ? 1u : 0u)) * layout->l.cycle_bytes;
        return GSH_OK;
    }

    int gsh_ion_decode_host(const gsh_ion_layout_t* layout, int stream, const void* bytes, uint64_t first_sample, uint64_t n_samples, float* out)
    {
        GSH_REQUIRE(layout != nullptr, "null layout");
        GSH_REQUIRE(stream >= 0 && stream < layout->l.n_streams, "stream %d outside 0..%d", stream, layout->l.n_streams - 1);
        GSH_REQUIRE(n_samples == 0 || (bytes != nullptr && out != nullptr), "null argument");
        const uint64_t per = layout->l.s[stream].cplx ? 2u : 1u;
        gsh::ion_decode_fields(layout->l, stream, static_cast<const unsigned char*>(bytes), first_sample * per, n_samples * per, out);
        return GSH_OK;
    }

    int gsh_ion_unpack_device(int device, const gsh_ion_layout_t* layout, const void* d_src, uint64_t first_sample, uint64_t n_samples,
        int inverted_spectrum, const int32_t* streams, int n_streams, void* const* d_dst, void* hip_stream)
    {
        int cplx = 0, rate = 0;
        int rc = gsh::ion_check_streams(layout, streams, n_streams, &cplx, &rate);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(d_dst != nullptr, "null argument");
        GSH_REQUIRE(cplx || !inverted_spectrum, "inverted_spectrum with real streams: IF samples have no spectrum to invert here");
        for (int i = 0; i < n_streams; i++)
            {
                GSH_REQUIRE(d_dst[i] != nullptr, "null destination for stream %d", streams[i]);
                GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_dst[i]) & (cplx ? 7u : 3u)) == 0, "destination must be %d-byte aligned", cplx ? 8 : 4);
            }
        GSH_REQUIRE(n_samples == 0 || d_src != nullptr, "null argument");
        GSH_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % layout->l.align == 0, "d_src: the %u-byte words of the layout must be %u-byte aligned", layout->l.align,
            layout->l.align);
        rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        return gsh::ion_unpack(layout, d_src, first_sample, n_samples, inverted_spectrum ? 1 : 0, streams, n_streams, d_dst, static_cast<hipStream_t>(hip_stream));
    }
}
