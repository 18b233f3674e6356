// Wide correlator bank for MI355X (gfx950, wave64): up to GSH_MAX_WIDE_TAPS (64) taps per job in one pass over the window.
//
// A tap of a wide job is one output of one reference Carrier_wipeoff_multicorrelator_resampler call in standard mode (the standard
// resampler K/volk_gnsssdr_32f_xn_resampler_32f_xn.h:63-80 and the standard rotator, what high_dyn = 0 means in gsh_corr_job); the
// chip of sample n at tap t is code[wrap(floor(fl(fl(fl(step * n) + shift_t) - rem)))], one IEEE rounding per operation (this file is
// compiled with -ffp-contract=off like the rest of the library), for ANY ascending shifts: spans wider than a code period, duplicates,
// negative raw indices.
//
// What a work-group (256 threads, four waves) does: one BLOCK of TB taps (4, 8 or 16) over one SEGMENT of one job's window.
//   * shared by the taps of the block: the 16-byte load of a lane's two samples, their rotation by the lane's own two phasors, the
//     conversion of n and fl(step * n) -- the first operation of every tap's index chain is the same float for all taps.  Per tap and
//     sample that leaves two adds, one floor conversion, one address, one LDS look-up and the complex multiply-accumulate;
//   * one accumulator set: TB complex sums per lane (32 registers at TB = 16), every sample rotated by its own phasor as the
//     closed-loop kernel does it, so that nothing has to be folded afterwards;
//   * the carrier is evaluated, not recurred: the work-group's factor table (mcorr_device.h fac_table_fill) seeds every lane exactly
//     and the phasors are stepped by exp(-j 512 step) for at most MC_RESEED (32) strides before the next exact seed;
//   * the code table holds exactly the raw chip indices [lo, hi] this block's taps can touch over this segment, wrapped while it is
//     staged: the chain is monotone in n and in the shift, so the four corners bound it, and the look-ups need neither a wrap nor a
//     guard band however wide the bank is (a +-1 100-chip span on a 1 023-chip code is a table of ~3 000 entries).  Only a range
//     that does not fit the LDS (more than 16 384 entries) stages the whole code and wraps every index;
//   * taps beyond the job's n_taps inside a block repeat the last real shift (same index range) and are not stored; tap blocks
//     beyond n_taps write zeros and end.
// Spreading a job over tap blocks changes no sum.  Spreading it over sample segments does, so the number of segments is a function
// of the job alone (multicorrelator_wide.h mcorr_wide_splits) and the partial sums are added in segment order: a job's output bits
// do not depend on the launch it shares.
#include "multicorrelator_wide.h"
#include "mcorr_device.h"

namespace gsh
{
namespace
{
using namespace mcdev;
constexpr int WT = GSH_MAX_WIDE_TAPS;
constexpr int WIDE_MAX_BLOCK = MCORR_WIDE_MAX_BLOCK;    // largest tap block
constexpr int WIDE_RED = MC_WAVES * WIDE_MAX_BLOCK;     // float2 entries of the wave-sum area
constexpr int WIDE_TABLE_CAP = 16384;                   // code-table entries: 64 KiB
constexpr int WIDE_RESEED = packed_reseed_trips(1);     // chunks of 512 samples between exact seeds: what fac_table_fill<1> spaces its A entries by

typedef const __attribute__((address_space(3))) float* lds_cfloat_ptr;

// the TB taps of one pair of samples.  a0 / a1: fl(step * n) of the two samples; y0 / y1: the rotated samples; tab_at: byte address of the
// table entry of raw index 0 (modulo 2^32: the raw indices of a windowed table may be anywhere in the int range); WRAP: the table is the whole code
template <int TB, bool WRAP>
__device__ __forceinline__ void wide_taps_pair(unsigned tab_at, int code_len, const float (&sh)[TB], float rem_code, float a0, float a1, float2 y0, float2 y1,
    float2 (&acc)[TB])
{
    // eight taps at a time: sixteen look-ups in flight, then their thirty-two multiply-accumulates (all TB at once want 2 TB registers for the code values alone)
    constexpr int G = TB < 8 ? TB : 8;
    static_assert(TB % G == 0, "tap block: whole groups");
#pragma unroll
    for (int g = 0; g < TB; g += G)
        {
            float c0[G], c1[G];
#pragma unroll
            for (int i = 0; i < G; i++)
                {
                    int k0 = raw_chip_std(a0, sh[g + i], rem_code);
                    int k1 = raw_chip_std(a1, sh[g + i], rem_code);
                    if constexpr (WRAP)
                        {
                            k0 = wrap_chip(k0, code_len);
                            k1 = wrap_chip(k1, code_len);
                        }
                    c0[i] = *reinterpret_cast<lds_cfloat_ptr>((static_cast<unsigned>(k0) << 2) + tab_at);
                    c1[i] = *reinterpret_cast<lds_cfloat_ptr>((static_cast<unsigned>(k1) << 2) + tab_at);
                }
#pragma unroll
            for (int i = 0; i < G; i++)
                {
                    acc[g + i].x = fmaf(y0.x, c0[i], acc[g + i].x);
                    acc[g + i].y = fmaf(y0.y, c0[i], acc[g + i].y);
                }
#pragma unroll
            for (int i = 0; i < G; i++)
                {
                    acc[g + i].x = fmaf(y1.x, c1[i], acc[g + i].x);
                    acc[g + i].y = fmaf(y1.y, c1[i], acc[g + i].y);
                }
        }
}

template <int TB>
__global__ __launch_bounds__(MC_THREADS, (TB <= 8 ? 4 : 3)) void wide_taps_kernel(McorrWideArgs a)  // (waves per SIMD the register count leaves: 134 registers at 16 taps)
{
    static_assert(TB <= WIDE_MAX_BLOCK && WT % TB == 0, "tap block");
    extern __shared__ __align__(16) float lds[];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    // tap block fastest, then segment, then job: the work-groups that read the same samples are neighbours (one XCD, one L2)
    const int block = static_cast<int>(lb % static_cast<unsigned>(a.n_blocks));
    const unsigned rest = lb / static_cast<unsigned>(a.n_blocks);
    const int split = static_cast<int>(rest % static_cast<unsigned>(a.max_splits));
    const int job = static_cast<int>(rest / static_cast<unsigned>(a.max_splits));
    const gsh_corr_job_wide& J = a.jobs[job];
    const int tid = threadIdx.x;
    const int n_taps = J.n_taps, n_total = J.n_samples;
    const int splits = mcorr_wide_splits(n_total, a.splits_user);
    if (split >= splits) return;  // (the grid is sized for the batch's longest job; nobody reads this job's partials beyond its own count)

    // ---- this work-group's taps [t0, t0 + TB) and its slice [n_begin, n_end) of the window
    const int t0 = block * TB;
    const int t_end = (block == a.n_blocks - 1) ? WT : t0 + TB;  // the last block launched also writes the zeros of the taps no block owns
    float2* const dst = (a.max_splits == 1 ? a.out + static_cast<size_t>(job) * WT : a.partials + (static_cast<size_t>(job) * a.max_splits + split) * WT) + t0;
    int seg = (n_total + splits - 1) / splits;
    seg = (seg + 1) & ~1;
    const int n_begin = min(split * seg, n_total);
    const int n_end = min(n_total, n_begin + seg);
    if (t0 >= n_taps || n_end <= n_begin)
        {
            if (tid < t_end - t0) dst[tid] = make_float2(0.0f, 0.0f);
            return;
        }
    const unsigned long long abs0 = J.sample_offset + static_cast<unsigned long long>(n_begin);
    const int odd = static_cast<int>(abs0 & 1ULL);
    const int n_first = n_begin - odd;                                                          // sample index of pair 0's first element
    const float2* __restrict__ base = a.stream + (abs0 - static_cast<unsigned long long>(odd));  // 16-byte aligned

    const float rem_code = J.rem_code_phase_chips, code_step = J.code_phase_step_chips;
    float sh[TB];
#pragma unroll
    for (int i = 0; i < TB; i++) sh[i] = J.shifts_chips[min(t0 + i, n_taps - 1)];

    // ---- the raw chip indices of this block over this segment: every rounding of the chain is monotone in n (either sign of the step)
    // and in the shift (ascending), so the four corners bound them -- evaluated with the very expressions the samples use
    int lo, hi;
    {
        const float aL = __fmul_rn(code_step, static_cast<float>(n_begin)), aH = __fmul_rn(code_step, static_cast<float>(n_end - 1));
        const int k00 = raw_chip_std(aL, sh[0], rem_code), k01 = raw_chip_std(aL, sh[TB - 1], rem_code);
        const int k10 = raw_chip_std(aH, sh[0], rem_code), k11 = raw_chip_std(aH, sh[TB - 1], rem_code);
        lo = min(min(k00, k01), min(k10, k11));
        hi = max(max(k00, k01), max(k10, k11));
    }
    const long long span = static_cast<long long>(hi) - lo + 1;

    // ---- stage the code table: entry i is code[wrap(lo + i)], i < span -- or, for a range the LDS cannot hold, the whole code
    const int code_len = a.code_lens[J.code_slot];
    const float* __restrict__ gcode = a.codes + static_cast<size_t>(J.code_slot) * a.code_stride;
    const unsigned tab_base = static_cast<unsigned>(reinterpret_cast<size_t>((lds_cfloat_ptr)lds));
    const bool windowed = span <= a.table_floats;
    const bool misfit = !windowed && code_len > a.table_floats;  // cannot happen for a batch the host sized (tracking_api.hip); reported as NaN if it does
    unsigned tab_at = tab_base;
    if (windowed)
        {
            int k = wrap_chip(wrap_chip(lo, code_len) + tid, code_len);
            for (int i = tid; i < static_cast<int>(span); i += MC_THREADS)
                {
                    lds[i] = gcode[k];
                    k += MC_THREADS;
                    if (code_len >= MC_THREADS)
                        k = k >= code_len ? k - code_len : k;
                    else
                        k = wrap_chip(k, code_len);
                }
            tab_at = tab_base - (static_cast<unsigned>(lo) << 2);
        }
    else if (!misfit)
        for (int j = tid; j < code_len; j += MC_THREADS) lds[j] = gcode[j];

    float2* const red = reinterpret_cast<float2*>(lds + ((a.table_floats + 3) & ~3));
    float2* const fac = red + WIDE_RED;
    const float phase_step = J.phase_step_rad, rem_carr = J.rem_carr_phase_rad;
    if ((tid >> 6) == 0) fac_table_fill<1>(fac, phase_step, rem_carr, n_first, tid);

    float2 acc[TB];
#pragma unroll
    for (int i = 0; i < TB; i++) acc[i] = make_float2(0.0f, 0.0f);

    __syncthreads();  // code table and factor table visible

    if (misfit)
        {
#pragma unroll
            for (int i = 0; i < TB; i++) acc[i] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        }
    else
        {
            const int n_pairs = (n_end - n_first + 1) >> 1;
            const int n_chunks = (n_pairs + MC_THREADS - 1) / MC_THREADS;
            const float2 lane_fac = cmul(fac[FAC_WH + (tid >> 5)], fac[FAC_B + (tid & 31)]);  // exp(-j 2 tid step)
            const float2 inc1 = fac[FAC_INC], inc_chunk = fac[FAC_INC + 1];                  // exp(-j step), exp(-j 512 step)
            const float4* __restrict__ const pairs = reinterpret_cast<const float4*>(base) + tid;
            // a chunk whose 512 samples all lie inside the segment: plain loads, no masks
            auto interior = [&](int c) { return (c > 0 || odd == 0) && (n_first + 2 * (c + 1) * MC_THREADS <= n_end); };
            // the lane's pair of chunk c; a sample outside the segment is not read and counts as zero
            auto load = [&](int c) -> float4 {
                if (interior(c)) return pairs[static_cast<size_t>(c) * MC_THREADS];
                const int n0 = n_first + 2 * (c * MC_THREADS + tid);
                const bool in0 = n0 >= n_begin && n0 < n_end, in1 = n0 + 1 < n_end;  // (n0 + 1 >= n_begin always)
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (in0 && in1)
                    v = pairs[static_cast<size_t>(c) * MC_THREADS];
                else if (in0 || in1)
                    {
                        const float2 s = base[2 * (static_cast<size_t>(c) * MC_THREADS + tid) + (in0 ? 0 : 1)];
                        v = in0 ? make_float4(s.x, s.y, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, s.x, s.y);
                    }
                return v;
            };
            // the whole walk, once per kind of table (the kind is the work-group's: no branch inside a trip)
            auto walk = [&](auto wrap) {
            float2 p0 = make_float2(1.0f, 0.0f), p1 = p0;
            float4 x = load(0);
            for (int c = 0; c < n_chunks; c++)
                {
                    const int n0 = n_first + 2 * (c * MC_THREADS + tid);
                    if (c % WIDE_RESEED == 0)
                        {
                            const int r = c / WIDE_RESEED;
                            if (r < FAC_NA)
                                p0 = cmul(fac[FAC_A + r], lane_fac);
                            else  // beyond the table (segments of more than 327 680 samples): the lane's own evaluation
                                p0 = expmj(carrier_phase<false>(rem_carr, phase_step, 0.0f, n0));
                            p1 = cmul(p0, inc1);
                        }
                    float4 x_next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (c + 1 < n_chunks) x_next = load(c + 1);
                    const float2 y0 = cmul(make_float2(x.x, x.y), p0), y1 = cmul(make_float2(x.z, x.w), p1);
                    // a sample outside the segment (zero above) looks up the nearest index inside it: the table holds the segment's range only
                    int m0 = n0, m1 = n0 + 1;
                    if (!interior(c))
                        {
                            m0 = min(max(m0, n_begin), n_end - 1);
                            m1 = min(max(m1, n_begin), n_end - 1);
                        }
                    const float a0 = __fmul_rn(code_step, static_cast<float>(m0)), a1 = __fmul_rn(code_step, static_cast<float>(m1));
                    wide_taps_pair<TB, decltype(wrap)::value>(tab_at, code_len, sh, rem_code, a0, a1, y0, y1, acc);
                    p0 = cmul(p0, inc_chunk);
                    p1 = cmul(p1, inc_chunk);
                    x = x_next;
                }
            };
            if (windowed)
                walk(std::false_type());
            else
                walk(std::true_type());
        }

    // ---- integrate-and-dump: wave64 prefix sums in DPP steps (the last lane holds the wave's sum), then one LDS step over the four waves in wave order
    {
        float sums[2 * TB];
#pragma unroll
        for (int i = 0; i < TB; i++)
            {
                sums[2 * i] = acc[i].x;
                sums[2 * i + 1] = acc[i].y;
            }
        wave_scan_incl_n(sums);
        if ((tid & 63) == 63)
            {
#pragma unroll
                for (int i = 0; i < TB; i++) red[(tid >> 6) * TB + i] = make_float2(sums[2 * i], sums[2 * i + 1]);
            }
    }
    __syncthreads();
    if (tid < t_end - t0)
        {
            float2 s = make_float2(0.0f, 0.0f);
            if (tid < TB && t0 + tid < n_taps)
                {
#pragma unroll
                    for (int w = 0; w < MC_WAVES; w++)
                        {
                            s.x += red[w * TB + tid].x;
                            s.y += red[w * TB + tid].y;
                        }
                }
            dst[tid] = s;
        }
}

// adds each job's per-segment partial sums in segment order (deterministic); the first partial is taken as it is
__global__ __launch_bounds__(256) void wide_taps_reduce(const float2* __restrict__ partials, const gsh_corr_job_wide* __restrict__ jobs, float2* __restrict__ out,
    int n_jobs, int max_splits, int splits_user)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // job * WT + tap
    if (i >= n_jobs * WT) return;
    const int job = i / WT, tap = i - job * WT;
    const int splits = mcorr_wide_splits(jobs[job].n_samples, splits_user);
    const float2* p = partials + static_cast<size_t>(job) * max_splits * WT + tap;
    float2 s = p[0];
    for (int k = 1; k < splits; k++)
        {
            s.x += p[static_cast<size_t>(k) * WT].x;
            s.y += p[static_cast<size_t>(k) * WT].y;
        }
    out[i] = s;
}

template <int TB>
int launch_block(const McorrWideArgs& a, size_t lds, hipStream_t stream)
{
    if (lds > 64 * 1024)
        GSH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_taps_kernel<TB>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    const unsigned long long grid = static_cast<unsigned long long>(a.n_jobs) * static_cast<unsigned>(a.n_blocks) * static_cast<unsigned>(a.max_splits);
    GSH_REQUIRE(grid <= 0x7fffffffULL, "%d wide jobs x %d tap blocks x %d segments exceed one launch", a.n_jobs, a.n_blocks, a.max_splits);
    hipLaunchKernelGGL((wide_taps_kernel<TB>), dim3(static_cast<unsigned>(grid)), dim3(MC_THREADS), lds, stream, a);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace

int mcorr_wide_table_cap() { return WIDE_TABLE_CAP; }

size_t mcorr_wide_lds_bytes(int table_floats)
{
    const size_t tab = (static_cast<size_t>(table_floats) + 3) & ~static_cast<size_t>(3);
    return tab * sizeof(float) + (WIDE_RED + FAC_ENTRIES) * sizeof(float2);
}

// Taps per work-group.  It changes no sum, so it may follow the launch: the largest block that still leaves four work-groups per compute unit (a block's
// samples are loaded and rotated once per work-group; 32 channels x 64 taps in blocks of 16 would be 128 work-groups on 256 compute units).
int mcorr_wide_tap_block(int n_jobs, int max_taps, int max_splits)
{
    const long long segments = static_cast<long long>(n_jobs) * max_splits;
    for (int tb = WIDE_MAX_BLOCK; tb > 4; tb /= 2)
        if (segments * ((max_taps + tb - 1) / tb) >= 4 * 256) return tb;
    return 4;
}

int mcorr_wide_launch(const McorrWideArgs& args, hipStream_t stream)
{
    if (args.n_jobs <= 0) return GSH_OK;
    McorrWideArgs a = args;
    GSH_REQUIRE(a.max_splits >= 1 && a.max_splits <= 64, "segments %d outside 1..64", a.max_splits);
    GSH_REQUIRE(a.table_floats >= 1 && a.table_floats <= WIDE_TABLE_CAP, "code table of %d entries outside 1..%d", a.table_floats, WIDE_TABLE_CAP);
    GSH_REQUIRE(a.max_splits == 1 || a.partials != nullptr, "no room for the partial sums");
    GSH_REQUIRE(a.max_taps >= 1 && a.max_taps <= WT, "n_taps %d outside 1..%d", a.max_taps, WT);
    a.tap_block = mcorr_wide_tap_block(a.n_jobs, a.max_taps, a.max_splits);
    a.n_blocks = (a.max_taps + a.tap_block - 1) / a.tap_block;
    const size_t lds = mcorr_wide_lds_bytes(a.table_floats);
    int rc;
    if (a.tap_block == 4)
        rc = launch_block<4>(a, lds, stream);
    else if (a.tap_block == 8)
        rc = launch_block<8>(a, lds, stream);
    else
        rc = launch_block<16>(a, lds, stream);
    if (rc != GSH_OK) return rc;
    if (a.max_splits > 1)
        {
            const int total = a.n_jobs * WT;
            hipLaunchKernelGGL(wide_taps_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, a.partials, a.jobs, a.out, a.n_jobs, a.max_splits, a.splits_user);
            GSH_HIP(hipGetLastError());
        }
    return GSH_OK;
}
}  // namespace gsh
