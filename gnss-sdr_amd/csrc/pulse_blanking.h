// The arithmetic of pulse blanking that gsh_pb_* (pulse_blanking.hip) and the conditioner's blanking stage (cond_blanking.hip) share, as device
// functions: both run this text, so a segment's energy and decision have the same bits whichever of the two forms them.
#ifndef GSH_PULSE_BLANKING_H
#define GSH_PULSE_BLANKING_H
#include "gsh_internal.h"

namespace gsh
{
constexpr int PB_THREADS = 256;
constexpr int PB_MAX_LENGTH = 4096;

// segments a work-group of the energy kernels stages at once: 32 KB of LDS
inline int pb_seg_per_wg(int length) { return length >= 8192 ? 1 : 8192 / length; }

// volk_32fc_magnitude_squared_32f, pulse_blanking_cc.cc:63
__device__ __forceinline__ float pb_mag2(float2 v) { return __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)); }

// energy of the segment whose |x|^2 lie at t[0 .. length): added in double from t[rot] on, rounded to float once.  rot is the segment's place in
// its work-group, (absolute segment index) % pb_seg_per_wg(length): the rotated start spreads the LDS banks
__device__ __forceinline__ float pb_segment_energy(const float* t, int length, int rot)
{
    double e = 0.0;
    for (int k = 0; k < length; k++) e += static_cast<double>(t[(k + rot) % length]);
    return static_cast<float>(e);
}

// pulse_blanking_cc.cc:69-95 over n_seg segments in order, one thread: mask[s] = 1 where segment s is blanked; the state goes in and out through the
// references; *n_blanked (may be null) is advanced by the number of blanked segments
__device__ __forceinline__ void pb_decide_segments(const float* __restrict__ energy, unsigned long long n_seg, unsigned char* __restrict__ mask, float& noise_io,
    int& n_segments_io, bool& last_filtered_io, float n_deg, int n_segments_est, int n_segments_reset, float thres, unsigned long long* n_blanked)
{
    float noise = noise_io;
    int n_segments = n_segments_io;
    bool last_filtered = last_filtered_io;
    unsigned long long blanked = 0;
    for (unsigned long long s = 0; s < n_seg; s++)
        {
            const float segment_energy = energy[s];
            unsigned char blank = 0;
            if ((n_segments < n_segments_est) && (last_filtered == false))
                {
                    noise = __fdiv_rn(__fadd_rn(__fmul_rn(static_cast<float>(n_segments), noise), __fdiv_rn(segment_energy, n_deg)), static_cast<float>(n_segments + 1));
                }
            else
                {
                    if (__fdiv_rn(segment_energy, noise) > thres)
                        {
                            blank = 1;
                            last_filtered = true;
                        }
                    else
                        {
                            last_filtered = false;
                            if (n_segments > n_segments_reset) n_segments = 0;
                        }
                }
            mask[s] = blank;
            n_segments++;
            if (n_blanked != nullptr) blanked += blank;
        }
    noise_io = noise;
    n_segments_io = n_segments;
    last_filtered_io = last_filtered;
    if (n_blanked != nullptr) *n_blanked += blanked;
}

// thres_ of pulse_blanking_cc.cc:48-49: quantile(complement(chi_squared(2 * length), pfa)) = 2 * gamma_p_inv(length, 1 - pfa), in float
inline float pb_threshold(float pfa, int length) { return static_cast<float>(2.0 * gamma_p_inv(static_cast<double>(length), 1.0 - static_cast<double>(pfa))); }
}  // namespace gsh
#endif
