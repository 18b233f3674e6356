// gsh_gen_*: the signal generator (Signal_Generator, src/algorithms/signal_generator/gnuradio_blocks/signal_generator_c.cc) on the device: synthetic
// GNSS scenarios written into a caller's buffer or straight into a sample ring.  See include/gnss_sdr_hip.h for the contract and
// signal_generator.h for the integer arithmetic shared with the host.
//
// Table-driven: a satellite is two complex tables of one period (the reference's sampled_code_data_ / sampled_code_pilot_, sg.cc:164-323, built and
// scaled by the host), two periodic sign sequences that advance where the reference may change its data bit (k == delay_samples inside every code
// period, sg.cc:362-383) and a carrier.  The three ways the reference combines its tables (sg.cc:366, :428-448, :518) are one expression:
//     out[n] = sum_sat (sA[p] A[n mod period] + sB[p] B[n mod period]) exp(+j (theta0 + 2 pi f n / fs)) + noise[n],   p = (n + period - delay) / period
// in float32, satellites in ascending order, every operation rounded once (-ffp-contract=off).  n is the ABSOLUTE sample index: table entry, sign
// entry, carrier phase and noise are functions of n alone, so the stream does not depend on how it is cut into calls, on the launch geometry or on
// where a ring wraps.
//
// Carrier.  The reference accumulates a float32 phase per sample (volk_gnsssdr_s32f_sincos_32fc) and a float32 start phase per vector
// (sg.cc:350-354); here the phase of sample n is frac(w n) + phi0 in 64-bit fixed point (signal_generator.h), rounded to float32 once and handed to
// sincospif -- the argument reduction of expmj (mcorr_device.h), without its double multiplication.  A stated deviation: DESIGN.md.
//
// Noise.  Philox4x32-10 keyed by the seed, counter = the absolute sample index; the first two words through Box-Muller give the sample's I and Q,
// unit variance each (the reference: two std::normal_distribution<float> engines, sg.cc:540-546).
//
// Work split.  A lane produces two consecutive samples and stores them as one 16-byte vector; pairs are aligned to the destination's 16 bytes, so
// a destination that starts on an odd sample (a ring position) has a one-sample head.  A work-group covers 512 samples.  Every table entry is read
// once per satellite and sample -- there is no reuse that staging in LDS would serve -- and consecutive lanes read consecutive entries; what IS
// shared by all lanes (the satellite's parameters, the launch's start indices) is wave-uniform and comes through scalar loads.
#include "gsh_internal.h"
#include "sample_stream.h"
#include "signal_generator.h"
#include <cmath>
#include <new>
#include <vector>

namespace
{
using gsh::GenArgs;
using gsh::GenSat;
using gsh::set_error;

// sample n0 + j of the launch
__device__ __forceinline__ float2 gen_sample(const GenArgs& a, unsigned j)
{
    const unsigned long long n = a.n0 + j;
    float re = 0.0f, im = 0.0f;
    for (int s = 0; s < a.n_sats; s++)
        {
            const GenSat& g = a.sats[s];
            const unsigned t = a.u0[s] + j;          // below 2^31: u0 < period <= 2^30, j < 2^30
            const unsigned q = t / g.period;         // sign boundaries passed since n0
            unsigned idx = t - q * g.period + g.delay;
            if (idx >= g.period) idx -= g.period;    // n mod period
            const float sa = static_cast<float>(g.sA[(a.pa0[s] + q) % g.len_a]);
            const float2 A = g.A[idx];
            float x = sa * A.x, y = sa * A.y;
            if (g.B != nullptr)
                {
                    const float sb = static_cast<float>(g.sB[(a.pb0[s] + q) % g.len_b]);
                    const float2 B = g.B[idx];
                    x = x + sb * B.x;
                    y = y + sb * B.y;
                }
            const unsigned long long rev = gsh::gen_phase_rev64(g.w_hi, g.w_lo, g.phi0, n);
            float sn, cs;
            sincospif(static_cast<float>(static_cast<long long>(rev)) * 0x1p-63f, &sn, &cs);  // 2 rev in [-1, 1]
            re = re + (x * cs - y * sn);
            im = im + (x * sn + y * cs);
        }
    if (a.noise)
        {
            uint32_t w[4];
            gsh::gen_noise_words(a.seed, n, w);
            const float u = (static_cast<float>(w[0] >> 9) + 0.5f) * 0x1p-23f;  // (0, 1), exact
            const float r = sqrtf(-2.0f * logf(u));
            float sn, cs;
            sincospif(static_cast<float>(static_cast<int>(w[1])) * 0x1p-31f, &sn, &cs);
            re = re + r * cs;
            im = im + r * sn;
        }
    return make_float2(re, im);
}

__global__ __launch_bounds__(gsh::GEN_THREADS) void gen_kernel(const GenArgs a)
{
    // pairs are aligned to the destination's 16 bytes: with an odd first sample the first pair's lower half lies before out[0]
    const unsigned skew = static_cast<unsigned>(reinterpret_cast<uintptr_t>(a.out) >> 3) & 1u;
    const long long j0 = static_cast<long long>(blockIdx.x) * gsh::GEN_TILE + 2 * static_cast<long long>(threadIdx.x) - skew;
    const bool ok0 = j0 >= 0 && j0 < static_cast<long long>(a.len);
    const bool ok1 = j0 + 1 < static_cast<long long>(a.len);
    if (ok0 && ok1)
        {
            const float2 v0 = gen_sample(a, static_cast<unsigned>(j0));
            const float2 v1 = gen_sample(a, static_cast<unsigned>(j0 + 1));
            *reinterpret_cast<float4*>(a.out + j0) = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    else if (ok0)
        a.out[j0] = gen_sample(a, static_cast<unsigned>(j0));
    else if (ok1)
        a.out[j0 + 1] = gen_sample(a, static_cast<unsigned>(j0 + 1));
}

// floor(frac(|f| / fs) 2^128) by long division, exact: r < fs always, 2 r exact, and fs <= 2 r < 2 fs where the subtraction happens (Sterbenz)
void rev_per_sample(double f, double fs, uint64_t* w_hi, uint64_t* w_lo)
{
    double r = std::fmod(std::fabs(f), fs);
    uint64_t w[2] = {0, 0};
    for (int i = 0; i < 128; i++)
        {
            r = 2.0 * r;
            w[i / 64] <<= 1;
            if (r >= fs)
                {
                    r -= fs;
                    w[i / 64] |= 1u;
                }
        }
    if (f < 0.0)  // two's complement of the 128-bit fraction
        {
            w[1] = ~w[1] + 1u;
            w[0] = ~w[0] + (w[1] == 0 ? 1u : 0u);
        }
    *w_hi = w[0];
    *w_lo = w[1];
}

struct SatHost
{
    bool set{false};
    GenSat d{};               // with device pointers
    void* buf{nullptr};       // one allocation: A, B, sA, sB
};
}  // namespace

struct gsh_gen
{
    int device{0};
    double fs{0.0};
    int n_sats{0};
    SatHost sat[gsh::GEN_MAX_SATS];
    GenSat* d_sats{nullptr};
    bool dirty{true};         // d_sats is behind sat[]
    int noise{0};
    unsigned long long seed{0};
    unsigned long long pos{0};  // next sample to produce
    hipStream_t stream{nullptr};
    hipEvent_t ev0{nullptr}, ev1{nullptr};
};

namespace gsh
{
int gen_launch(const GenArgs& a, void* hip_stream)
{
    const unsigned skew = static_cast<unsigned>(reinterpret_cast<uintptr_t>(a.out) >> 3) & 1u;
    const unsigned long long span = static_cast<unsigned long long>(a.len) + skew;
    const unsigned grid = static_cast<unsigned>((span + GEN_TILE - 1) / GEN_TILE);
    hipLaunchKernelGGL(gen_kernel, dim3(grid), dim3(GEN_THREADS), 0, static_cast<hipStream_t>(hip_stream), a);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace gsh

namespace
{
constexpr unsigned long long GEN_MAX_INDEX = 1ull << 63;

int check_ready(const gsh_gen* g)
{
    GSH_REQUIRE(g != nullptr, "null generator");
    for (int s = 0; s < g->n_sats; s++)
        if (!g->sat[s].set) return set_error(GSH_ERR_STATE, "satellite %d of %d has not been set (gsh_gen_set_satellite)", s, g->n_sats);
    return GSH_OK;
}

// samples [n0, n0 + n) into out on st, in launches of GEN_MAX_LAUNCH at most
int launch_range(gsh_gen* g, unsigned long long n0, unsigned long long n, float2* out, hipStream_t st)
{
    if (g->dirty)
        {
            GenSat h[gsh::GEN_MAX_SATS];
            for (int s = 0; s < g->n_sats; s++) h[s] = g->sat[s].d;
            GSH_HIP(hipMemcpy(g->d_sats, h, sizeof(GenSat) * g->n_sats, hipMemcpyHostToDevice));  // (synchronous: no launch of this handle is in flight)
            g->dirty = false;
        }
    while (n > 0)
        {
            const unsigned long long len = n < gsh::GEN_MAX_LAUNCH ? n : gsh::GEN_MAX_LAUNCH;
            GenArgs a{};
            a.sats = g->d_sats;
            a.out = out;
            a.n0 = n0;
            a.seed = g->seed;
            a.len = static_cast<uint32_t>(len);
            a.n_sats = g->n_sats;
            a.noise = g->noise;
            for (int s = 0; s < g->n_sats; s++)
                {
                    const GenSat& d = g->sat[s].d;
                    const unsigned long long u = n0 + d.period - d.delay;
                    const unsigned long long p = u / d.period;
                    a.u0[s] = static_cast<uint32_t>(u % d.period);
                    a.pa0[s] = static_cast<uint16_t>(p % d.len_a);
                    a.pb0[s] = static_cast<uint16_t>(d.len_b ? p % d.len_b : 0);
                }
            int rc = gsh::gen_launch(a, st);
            if (rc != GSH_OK) return rc;
            n0 += len;
            out += len;
            n -= len;
        }
    return GSH_OK;
}

struct SegmentCtx
{
    gsh_gen* g;
};

// MultiSegmentWriter: samples [first, first + len) of the push into dst[0]
int write_segment(void* ctx, unsigned long long first, unsigned long long len, float2* const* dst, hipStream_t st)
{
    gsh_gen* g = static_cast<SegmentCtx*>(ctx)->g;
    return launch_range(g, g->pos + first, len, dst[0], st);
}

bool signs_ok(const int8_t* s, int len)
{
    for (int i = 0; i < len; i++)
        if (s[i] != 1 && s[i] != -1) return false;
    return true;
}
}  // namespace

extern "C"
{
    void gsh_gen_philox_words(uint64_t seed, uint64_t sample_index, uint32_t out[4])
    {
        gsh::gen_noise_words(seed, sample_index, out);
    }

    int gsh_gen_check_satellite(double fs_sps, const float* table_a, const float* table_b, uint32_t period, uint32_t delay_samples, const int8_t* signs_a,
        int32_t len_a, const int8_t* signs_b, int32_t len_b, double doppler_hz, double start_phase_rad, double carrier_offset_hz)
    {
        GSH_REQUIRE(std::isfinite(fs_sps) && fs_sps > 0.0, "the sample rate must be positive and finite");
        GSH_REQUIRE(table_a != nullptr, "null table A");
        GSH_REQUIRE(period >= 1, "period %u below 1", period);
        GSH_REQUIRE(period <= (1u << 30), "period %u above 2^30", period);
        GSH_REQUIRE(delay_samples < period, "delay_samples %u outside [0, %u)", delay_samples, period);
        GSH_REQUIRE(signs_a != nullptr, "null sign sequence A");
        GSH_REQUIRE(len_a >= 1 && len_a <= gsh::GEN_MAX_SIGNS, "sign sequence A of %d entries outside 1..%d", len_a, gsh::GEN_MAX_SIGNS);
        GSH_REQUIRE(signs_ok(signs_a, len_a), "sign sequence A holds a byte that is neither +1 nor -1");
        if (table_b != nullptr)
            {
                GSH_REQUIRE(signs_b != nullptr, "null sign sequence B with a table B");
                GSH_REQUIRE(len_b >= 1 && len_b <= gsh::GEN_MAX_SIGNS, "sign sequence B of %d entries outside 1..%d", len_b, gsh::GEN_MAX_SIGNS);
                GSH_REQUIRE(signs_ok(signs_b, len_b), "sign sequence B holds a byte that is neither +1 nor -1");
            }
        GSH_REQUIRE(std::isfinite(doppler_hz), "the Doppler is not finite");
        GSH_REQUIRE(std::isfinite(start_phase_rad), "the start phase is not finite");
        GSH_REQUIRE(std::isfinite(carrier_offset_hz) && std::isfinite(doppler_hz + carrier_offset_hz), "the carrier offset is not finite");
        for (uint32_t i = 0; i < 2 * period; i++)
            {
                GSH_REQUIRE(std::isfinite(table_a[i]), "table A holds a value that is not finite (float %u)", i);
                GSH_REQUIRE(table_b == nullptr || std::isfinite(table_b[i]), "table B holds a value that is not finite (float %u)", i);
            }
        return GSH_OK;
    }

    int gsh_gen_create(int device, double fs_sps, int32_t n_sats, gsh_gen_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null out pointer");
        *out = nullptr;
        GSH_REQUIRE(std::isfinite(fs_sps) && fs_sps > 0.0, "the sample rate must be positive and finite");
        GSH_REQUIRE(n_sats >= 1 && n_sats <= gsh::GEN_MAX_SATS, "n_sats %d outside 1..%d", n_sats, gsh::GEN_MAX_SATS);
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_gen* g = new (std::nothrow) gsh_gen();
        GSH_REQUIRE(g != nullptr, "out of host memory");
        g->device = device;
        g->fs = fs_sps;
        g->n_sats = n_sats;
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_gen_destroy(g);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipEventCreate(&g->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipEventCreate(&g->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipMalloc(&g->d_sats, sizeof(GenSat) * n_sats)) != hipSuccess) return fail(e, "hipMalloc(satellites)");
        *out = g;
        return GSH_OK;
    }

    void gsh_gen_destroy(gsh_gen_t* g)
    {
        if (!g) return;
        (void)hipSetDevice(g->device);
        if (g->stream) (void)hipStreamSynchronize(g->stream);
        for (auto& s : g->sat)
            if (s.buf) (void)hipFree(s.buf);
        if (g->d_sats) (void)hipFree(g->d_sats);
        if (g->ev0) (void)hipEventDestroy(g->ev0);
        if (g->ev1) (void)hipEventDestroy(g->ev1);
        if (g->stream) (void)hipStreamDestroy(g->stream);
        delete g;
    }

    int gsh_gen_set_satellite(gsh_gen_t* g, int32_t sat, const float* table_a, const float* table_b, uint32_t period, uint32_t delay_samples,
        const int8_t* signs_a, int32_t len_a, const int8_t* signs_b, int32_t len_b, double doppler_hz, double start_phase_rad, double carrier_offset_hz)
    {
        GSH_REQUIRE(g != nullptr, "null generator");
        GSH_REQUIRE(sat >= 0 && sat < g->n_sats, "satellite %d outside 0..%d", sat, g->n_sats - 1);
        int rc = gsh_gen_check_satellite(g->fs, table_a, table_b, period, delay_samples, signs_a, len_a, signs_b, len_b, doppler_hz, start_phase_rad,
            carrier_offset_hz);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(g->device));
        // one allocation: A | B | sA | sB (the tables first: 8-byte aligned)
        const size_t tab = sizeof(float2) * period;
        const size_t nb = table_b ? 1 : 0;
        const size_t bytes = tab * (1 + nb) + static_cast<size_t>(len_a) + (nb ? static_cast<size_t>(len_b) : 0);
        std::vector<unsigned char> h(bytes);
        std::memcpy(h.data(), table_a, tab);
        if (nb) std::memcpy(h.data() + tab, table_b, tab);
        std::memcpy(h.data() + tab * (1 + nb), signs_a, len_a);
        if (nb) std::memcpy(h.data() + tab * (1 + nb) + len_a, signs_b, len_b);
        void* buf = nullptr;
        GSH_HIP(hipMalloc(&buf, bytes));
        hipError_t e = hipMemcpy(buf, h.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess)
            {
                (void)hipFree(buf);
                return gsh::hip_fail(e, "hipMemcpy(satellite)", __FILE__, __LINE__);
            }
        SatHost& s = g->sat[sat];
        if (s.buf) (void)hipFree(s.buf);  // (every call of the handle that launches also waits: nothing still reads it)
        s.buf = buf;
        unsigned char* d = static_cast<unsigned char*>(buf);
        s.d.A = reinterpret_cast<const float2*>(d);
        s.d.B = nb ? reinterpret_cast<const float2*>(d + tab) : nullptr;
        s.d.sA = reinterpret_cast<const signed char*>(d + tab * (1 + nb));
        s.d.sB = nb ? s.d.sA + len_a : nullptr;
        rev_per_sample(doppler_hz + carrier_offset_hz, g->fs, &s.d.w_hi, &s.d.w_lo);
        double rev = start_phase_rad * 0.15915494309189533576888376337251436;
        rev -= std::floor(rev);
        s.d.phi0 = rev >= 1.0 ? 0u : static_cast<uint64_t>(std::ldexp(rev, 64));
        s.d.period = period;
        s.d.delay = delay_samples;
        s.d.len_a = static_cast<uint32_t>(len_a);
        s.d.len_b = nb ? static_cast<uint32_t>(len_b) : 0u;
        s.set = true;
        g->dirty = true;
        return GSH_OK;
    }

    int gsh_gen_set_noise(gsh_gen_t* g, int32_t enabled, uint64_t seed)
    {
        GSH_REQUIRE(g != nullptr, "null generator");
        g->noise = enabled ? 1 : 0;
        g->seed = seed;
        return GSH_OK;
    }

    int gsh_gen_seek(gsh_gen_t* g, uint64_t sample_index)
    {
        GSH_REQUIRE(g != nullptr, "null generator");
        GSH_REQUIRE(sample_index < GEN_MAX_INDEX, "sample index %llu at or above 2^63", static_cast<unsigned long long>(sample_index));
        g->pos = sample_index;
        return GSH_OK;
    }

    int gsh_gen_position(const gsh_gen_t* g, uint64_t* sample_index)
    {
        GSH_REQUIRE(g != nullptr && sample_index != nullptr, "null argument");
        *sample_index = g->pos;
        return GSH_OK;
    }

    int gsh_gen_generate_device(gsh_gen_t* g, uint64_t n, void* device_out)
    {
        int rc = check_ready(g);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(n == 0 || device_out != nullptr, "null output");
        GSH_REQUIRE(reinterpret_cast<uintptr_t>(device_out) % sizeof(float2) == 0, "the output must be aligned to a complex sample (8 bytes)");
        GSH_REQUIRE(n < GEN_MAX_INDEX - g->pos, "%llu samples from %llu pass 2^63", static_cast<unsigned long long>(n), g->pos);
        if (n == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(g->device));
        rc = launch_range(g, g->pos, n, static_cast<float2*>(device_out), g->stream);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipStreamSynchronize(g->stream));
        g->pos += n;
        return GSH_OK;
    }

    int gsh_gen_push(gsh_gen_t* g, gsh_stream_t* ring, uint64_t n, uint64_t* first_index)
    {
        int rc = check_ready(g);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(ring != nullptr, "null ring");
        GSH_REQUIRE(ring->device == g->device, "the ring lies on device %d, the generator on device %d", ring->device, g->device);
        GSH_REQUIRE(n < GEN_MAX_INDEX - g->pos, "%llu samples from %llu pass 2^63", static_cast<unsigned long long>(n), g->pos);
        rc = gsh::stream_multi_check_rings(&ring, 1, n);
        if (rc != GSH_OK) return rc;
        rc = gsh::stream_multi_check_live(&ring, 1, n);
        if (rc != GSH_OK) return rc;
        if (first_index) *first_index = ring->next;
        if (n == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(g->device));
        SegmentCtx ctx{g};
        rc = gsh::stream_write_device_multi(&ring, 1, n, ring->stream, write_segment, &ctx);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipStreamSynchronize(ring->stream));
        g->pos += n;
        return GSH_OK;
    }

    int gsh_gen_time_generate(gsh_gen_t* g, uint64_t n, int reps, float* avg_ms)
    {
        int rc = check_ready(g);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(avg_ms != nullptr, "null avg_ms");
        GSH_REQUIRE(n >= 1 && n <= gsh::GEN_MAX_LAUNCH && reps >= 1, "%llu samples x %d", static_cast<unsigned long long>(n), reps);
        GSH_REQUIRE(n < GEN_MAX_INDEX - g->pos, "%llu samples from %llu pass 2^63", static_cast<unsigned long long>(n), g->pos);
        GSH_HIP(hipSetDevice(g->device));
        float2* d_out = nullptr;
        GSH_HIP(hipMalloc(&d_out, sizeof(float2) * n));
        hipStream_t st = g->stream;
        hipError_t e = hipSuccess;
        float ms = 0.0f;
        for (int i = 0; i < 3 && rc == GSH_OK; i++) rc = launch_range(g, g->pos, n, d_out, st);  // clocks up
        if (rc == GSH_OK && (e = hipEventRecord(g->ev0, st)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        for (int i = 0; i < reps && rc == GSH_OK; i++) rc = launch_range(g, g->pos, n, d_out, st);
        if (rc == GSH_OK && (e = hipEventRecord(g->ev1, st)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventSynchronize(g->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventSynchronize", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventElapsedTime(&ms, g->ev0, g->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventElapsedTime", __FILE__, __LINE__);
        (void)hipStreamSynchronize(st);
        (void)hipFree(d_out);
        if (rc != GSH_OK) return rc;
        *avg_ms = ms / static_cast<float>(reps);
        return GSH_OK;
    }
}
