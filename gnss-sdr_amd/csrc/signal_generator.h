// The signal generator's integer arithmetic (gsh_gen_*, include/gnss_sdr_hip.h), shared by the kernel (signal_generator.hip) and the host: the
// Philox4x32-10 word stage of the noise, the carrier's fixed-point revolution count, and the launch arguments.  Plain C++ as kalman_step.h and
// exact_division.h are: the same text runs on a lane and -- for tests/test_siggen_abi.py, through gsh_gen_philox_words -- on the host.
#ifndef GSH_SIGNAL_GENERATOR_H
#define GSH_SIGNAL_GENERATOR_H
#include <stdint.h>

#ifdef __HIPCC__
#define GSH_GEN_FN __device__ __host__ inline __attribute__((always_inline))
#else
#define GSH_GEN_FN inline
#endif

namespace gsh
{
constexpr int GEN_MAX_SATS = 32;       // GSH_GEN_MAX_SATS
constexpr int GEN_MAX_SIGNS = 1024;    // entries of a sign sequence
constexpr int GEN_THREADS = 256;       // lanes of a work-group, two consecutive samples each
constexpr int GEN_TILE = 2 * GEN_THREADS;
constexpr unsigned long long GEN_MAX_LAUNCH = 1ull << 30;  // samples per launch: offset + period and the boundary count stay below 2^32

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   k0 += W0, k1 += W1 after each but the last
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

GSH_GEN_FN void philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; r++)
        {
            const uint64_t p0 = static_cast<uint64_t>(PHILOX_M0) * c0;
            const uint64_t p1 = static_cast<uint64_t>(PHILOX_M1) * c2;
            const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
            const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
            c1 = static_cast<uint32_t>(p1);
            c3 = static_cast<uint32_t>(p0);
            c0 = n0;
            c2 = n2;
            k0 += PHILOX_W0;
            k1 += PHILOX_W1;
        }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the four words of absolute sample n under `seed`: counter (n low, n high, 0, 0), key (seed low, seed high).  Nothing else enters.
GSH_GEN_FN void gen_noise_words(uint64_t seed, uint64_t n, uint32_t out[4])
{
    const uint32_t ctr[4] = {static_cast<uint32_t>(n), static_cast<uint32_t>(n >> 32), 0u, 0u};
    philox4x32_10(ctr, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), out);
}

// ---- carrier.  The frequency is kept as revolutions per sample in 0.128 fixed point (w_hi : w_lo, two's complement for a negative frequency), the
// start phase as revolutions in 0.64; the phase of absolute sample n is the top 64 bits of frac(w n) + phi0 -- integer arithmetic modulo one
// revolution, a function of n alone, exact to 2^-64 revolutions for any 64-bit n.
GSH_GEN_FN uint64_t gen_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}
GSH_GEN_FN uint64_t gen_phase_rev64(uint64_t w_hi, uint64_t w_lo, uint64_t phi0, uint64_t n)
{
    return w_hi * n + gen_mulhi64(w_lo, n) + phi0;
}

#ifdef __HIPCC__
// what a satellite is, resident in device memory between launches (gsh_gen_set_satellite)
struct GenSat
{
    const float2* A;         // `period` samples
    const float2* B;         // or nullptr
    const signed char* sA;   // len_a entries of +-1
    const signed char* sB;   // len_b entries
    uint64_t w_hi, w_lo;     // revolutions per sample, 0.128
    uint64_t phi0;           // start phase, revolutions, 0.64
    uint32_t period, delay;
    uint32_t len_a, len_b;
};

// One launch: samples [n0, n0 + len) into out.  Passed by value.  With u = (n + period - delay), sample n reads table entry n mod period =
// (u mod period + delay) mod period and sign entry (u / period) mod len; the host gives u mod period and the sign indices at n0, the kernel adds
// the offset (below 2^30) in 32 bits.
struct GenArgs
{
    const GenSat* sats;
    float2* out;
    uint64_t n0;
    uint64_t seed;
    uint32_t len;
    int32_t n_sats;
    int32_t noise;
    uint32_t u0[GEN_MAX_SATS];
    uint16_t pa0[GEN_MAX_SATS], pb0[GEN_MAX_SATS];
};

int gen_launch(const GenArgs& a, void* hip_stream);
#endif
}  // namespace gsh
#endif
