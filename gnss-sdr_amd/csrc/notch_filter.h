// The arithmetic of the notch filters that gsh_notch_* (notch_filter.hip) and the conditioner's notch stage (cond_notch.hip) share, as device
// functions: both run this text, so a segment's energy, noise floor, decision and per-sample map have the same bits whichever of the two forms them.
// Restates notch_cc.cc:73-118 and notch_lite_cc.cc:81-136; see the head of notch_filter.hip.
#ifndef GSH_NOTCH_FILTER_H
#define GSH_NOTCH_FILTER_H
#include "gsh_internal.h"

namespace gsh
{
constexpr int NF_THREADS = 256;
constexpr int NF_CHUNK = 128;  // samples one thread chains sequentially

// the blocks' sequential state (device memory)
struct NotchState
{
    float noise_pow_est;
    int n_segments;
    int filter_state;
    int n_segments_coeff;
    float2 last_out;
    float2 z0;
};

// segments a work-group of the segment kernels stages at once, and the LDS it needs: length twiddles, then per staged sample the sample and its dB value
inline int nf_seg_per_wg(int length) { return 2048 / length > 1 ? 2048 / length : 1; }
inline size_t nf_segment_lds(int length) { return sizeof(float2) * length + (sizeof(float2) + sizeof(float)) * static_cast<size_t>(nf_seg_per_wg(length)) * length; }

// thres_ of notch.cc:54-55: quantile(complement(chi_squared(2 * length), pfa)) = 2 * gamma_p_inv(length, 1 - pfa), in float
inline float nf_threshold(float pfa, int length) { return static_cast<float>(2.0 * gamma_p_inv(static_cast<double>(length), 1.0 - static_cast<double>(pfa))); }

__device__ __forceinline__ float2 cmul_ref(float2 a, float2 b)  // std::complex<float> product, one rounding per operation
{
    return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)); }

// z0 = exp(j atan2(Im c, Re c)), c = cur conj(prev)   (notch.cc:95-99; volk_32fc_x2_multiply_conjugate_32fc, volk_32fc_s32f_atan2_32f, std::exp)
__device__ __forceinline__ float2 phase_step(float2 cur, float2 prev)
{
    const float cr = __fadd_rn(__fmul_rn(cur.x, prev.x), __fmul_rn(cur.y, prev.y));
    const float ci = __fsub_rn(__fmul_rn(cur.y, prev.x), __fmul_rn(cur.x, prev.y));
    const float ang = atan2f(ci, cr);
    float s, c;
    sincosf(ang, &s, &c);
    return make_float2(c, s);
}
__device__ __forceinline__ float angle_step(float2 cur, float2 prev)
{
    const float cr = __fadd_rn(__fmul_rn(cur.x, prev.x), __fmul_rn(cur.y, prev.y));
    const float ci = __fsub_rn(__fmul_rn(cur.y, prev.x), __fmul_rn(cur.x, prev.y));
    return atan2f(ci, cr);
}

// The body of a segment kernel's work-group (NF_THREADS threads, nf_segment_lds() bytes at lds): energy and -- with_floor -- the floor value of
// segments seg0 .. seg0 + segs of the launch.  x points at item 0 (the sample in front of the first one processed); segment s covers items
// 1 + s L .. s L + L.  rot0 is the place of the work-group's first segment in the rotation of the energy sum, (its index in the stream the rotation
// is keyed to) % seg_per_wg: a launch whose first segment opens that stream passes 0, since seg0 is a multiple of seg_per_wg.
__device__ __forceinline__ void nf_segment_workgroup(float* lds, const float2* __restrict__ x, int length, unsigned long long seg0, int segs, float* __restrict__ energy,
    float* __restrict__ floor_lin, int with_floor, int seg_per_wg, int rot0)
{
    float2* tw = reinterpret_cast<float2*>(lds);                        // length twiddles
    float2* xs = tw + length;                                           // seg_per_wg * length samples
    float* db = reinterpret_cast<float*>(xs + static_cast<size_t>(seg_per_wg) * length);  // seg_per_wg * length dB values
    const int count = segs * length;
    const float2* __restrict__ cur = x + 1 + seg0 * length;
    for (int i = threadIdx.x; i < count; i += NF_THREADS) xs[i] = cur[i];
    if (with_floor)
        for (int i = threadIdx.x; i < length; i += NF_THREADS)
            {
                float s, c;
                sincospif(2.0f * static_cast<float>(i) / static_cast<float>(length), &s, &c);
                tw[i] = make_float2(c, -s);
            }
    __syncthreads();
    // energy: real part of volk_32fc_x2_conjugate_dot_prod_32fc(in, in) (notch.cc:87-88), float terms, double sum
    for (int s = threadIdx.x; s < segs; s += NF_THREADS)
        {
            const int rot = (rot0 + s) % seg_per_wg;
            double e = 0.0;
            for (int k = 0; k < length; k++)
                {
                    const float2 v = xs[s * length + (k + rot) % length];
                    e += static_cast<double>(__fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)));
                }
            energy[seg0 + s] = static_cast<float>(e);
        }
    if (!with_floor) return;
    // spectrum: bin k of segment s (notch.cc:77-79); 10 log10 through a base-2 logarithm like the VOLK kernel
    for (int i = threadIdx.x; i < count; i += NF_THREADS)
        {
            const int s = i / length, k = i - s * length;
            double ar = 0.0, ai = 0.0;
            int m = 0;
            for (int n = 0; n < length; n++)
                {
                    const float2 v = xs[s * length + n], w = tw[m];
                    ar += static_cast<double>(v.x) * w.x - static_cast<double>(v.y) * w.y;
                    ai += static_cast<double>(v.x) * w.y + static_cast<double>(v.y) * w.x;
                    m += k;
                    if (m >= length) m -= length;
                }
            const float re = static_cast<float>(ar), im = static_cast<float>(ai);
            const float p = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
            db[i] = p > 0.0f ? __fmul_rn(3.01029995663981209120f, log2f(p)) : __fmul_rn(3.01029995663981209120f, -127.0f);
        }
    __syncthreads();
    // volk_32f_s32f_calc_spectral_noise_floor_32f(&sig2dB, power_spect, 15.0, length) and notch.cc:82, sequential float sums as the kernel forms them
    for (int s = threadIdx.x; s < segs; s += NF_THREADS)
        {
            const float* d = db + s * length;
            float sum = 0.0f;
            for (int k = 0; k < length; k++) sum = __fadd_rn(sum, d[k]);
            const float mean_amp = __fadd_rn(__fdiv_rn(sum, static_cast<float>(length)), 15.0f);
            sum = 0.0f;
            int kept = length;
            for (int k = 0; k < length; k++)
                {
                    if (d[k] <= mean_amp)
                        sum = __fadd_rn(sum, d[k]);
                    else
                        kept--;
                }
            const float sig2db = kept == 0 ? mean_amp : __fdiv_rn(sum, static_cast<float>(kept));
            floor_lin[seg0 + s] = __fdiv_rn(powf(10.0f, __fdiv_rn(sig2db, 10.0f)), static_cast<float>(2 * length));
        }
}

// A call can reach an estimating segment (and so needs the floor values) only from a state with the counter below n_segments_est, or when the
// counter can pass n_segments_reset inside the call: it only grows otherwise.
__host__ __device__ __forceinline__ bool nf_needs_floor(int n_segments, unsigned long long n_seg, int n_segments_est, int n_segments_reset)
{
    return (n_segments < n_segments_est) || (static_cast<unsigned long long>(n_segments) + n_seg > static_cast<unsigned long long>(n_segments_reset));
}

// notch.cc:72-118 / lite.cc:81-136, one segment after the other, one thread: mode[i] = 0 estimate + copy, 1 filter, 2 copy; bit 7: the filter engages
// here (last_out = 0); z0_seg[i] (lite) the segment's coefficient.  s goes in and out (last_out and Notch's z0 are not touched); *n_filtered (may be
// null) is advanced by the number of filtered segments.  false: an estimating segment was reached without the floor values (have_floor 0); the
// caller drops s and what was written so far and repeats with them.
__device__ __forceinline__ bool nf_decide_segments(const float2* __restrict__ x, const float* __restrict__ energy, const float* __restrict__ floor_lin, int have_floor,
    unsigned long long n_seg, int length, unsigned char* __restrict__ mode, float2* __restrict__ z0_seg, NotchState& s, int n_segments_est, int n_segments_reset,
    int n_segments_coeff_reset, float thres, unsigned long long* n_filtered)
{
    const bool lite = n_segments_coeff_reset > 0;
    unsigned long long filtered = 0;
    for (unsigned long long i = 0; i < n_seg; i++)
        {
            unsigned char m;
            if ((s.n_segments < n_segments_est) && (s.filter_state == 0))
                {
                    if (!have_floor) return false;
                    s.noise_pow_est = __fdiv_rn(__fadd_rn(__fmul_rn(static_cast<float>(s.n_segments), s.noise_pow_est), floor_lin[i]), static_cast<float>(s.n_segments + 1));
                    m = 0;
                }
            else
                {
                    if (__fdiv_rn(energy[i], s.noise_pow_est) > thres)
                        {
                            m = 1;
                            if (s.filter_state == 0)
                                {
                                    s.filter_state = 1;
                                    m |= 0x80;  // last_out_ = 0
                                    s.n_segments_coeff = 0;
                                }
                            if (lite)
                                {
                                    if (s.n_segments_coeff == 0)
                                        {
                                            const float2* cur = x + 1 + i * length;
                                            const float a1 = angle_step(cur[1], cur[0]);
                                            const float a2 = angle_step(cur[length - 1], cur[length - 2]);
                                            const float ang = __fdiv_rn(__fadd_rn(a1, a2), 2.0f);
                                            float sn, cs;
                                            sincosf(ang, &sn, &cs);
                                            s.z0 = make_float2(cs, sn);
                                        }
                                    z0_seg[i] = s.z0;
                                    s.n_segments_coeff = (s.n_segments_coeff + 1) % n_segments_coeff_reset;
                                }
                            filtered++;
                        }
                    else
                        {
                            if (s.n_segments > n_segments_reset) s.n_segments = 0;
                            s.filter_state = 0;
                            m = 2;
                        }
                }
            mode[i] = m;
            s.n_segments++;
        }
    if (n_filtered != nullptr) *n_filtered += filtered;
    return true;
}

// the affine map of sample n (output index): out = a + b * out_prev
__device__ __forceinline__ void sample_map(const float2* __restrict__ x, unsigned long long n, int length, const unsigned char* __restrict__ mode,
    const float2* __restrict__ z0_seg, bool lite, float p, float2& a, float2& b, float2* z_out = nullptr)
{
    const unsigned long long s = n / length;
    const unsigned char m = mode[s];
    const float2 cur = x[n + 1], prev = x[n];
    if ((m & 0x7f) != 1)
        {
            a = cur;
            b = make_float2(0.0f, 0.0f);
            return;
        }
    const float2 z = lite ? z0_seg[s] : phase_step(cur, prev);
    if (z_out) *z_out = z;
    a = csub(cur, cmul_ref(z, prev));                                 // in[n] - z0 in[n-1]
    b = cmul_ref(make_float2(p, 0.0f), z);                            // p_c_factor_ * z_0_ (complex product as the block forms it)
    if ((m & 0x80) && (n - s * length == 0)) b = make_float2(0.0f, 0.0f);  // the filter engages: last_out_ = 0
}
}  // namespace gsh
#endif
