// Batched Early/Prompt/Late (VE/E/P/L/VL) multicorrelator for MI355X (gfx950, wave64).
//
// One launch evaluates many "jobs"; a job is one call of the reference's
//   Cpu_Multicorrelator_Real_Codes::Carrier_wipeoff_multicorrelator_resampler
//   (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.cc:103-126)
// i.e. code resampling
//   (K/volk_gnsssdr_32f_xn_resampler_32f_xn.h:63-80, K/..high_dynamics_resampler..:67-91)
// fused with carrier wipe-off and multiply-accumulate
//   (K/volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn.h:66-98, K/..high_dynamic_rotator..:68-109),
// K/ = src/algorithms/libs/volk_gnsssdr_module/volk_gnsssdr/kernels/volk_gnsssdr/ in the gnss-sdr tree.
//
// Design (not a translation of the reference's CPU kernels or of its CUDA block):
//   * no resampled-code buffers and no wiped-off signal buffer ever exist: the chip of
//     sample n is looked up on the fly from an LDS-resident copy of the +-1 code;
//   * the chip index uses the reference's float32 expression operation for operation
//     ((step*(float)n + shift) - rem, one IEEE rounding each; this file is compiled with
//     -ffp-contract=off), so chip selection is BIT-EXACT with the _generic protokernel;
//   * the carrier NCO is evaluated, not recurred from n=0: every thread seeds
//     exp(-j(rem + n*step)) exactly (double-precision phase, reduced mod 2pi) and steps it
//     by exp(-j*512*step) for at most MC_RESEED (32) strides before re-seeding, which keeps the
//     rotator within ~1e-6 of the exact value instead of the reference's O(1e-5) drift;
//   * each work-group (256 threads = 4 waves) streams its window with 16-byte loads
//     (two complex64 per lane, 1 KiB per wave-instruction), accumulates T complex sums per
//     lane in registers, reduces them with wave64 shuffles and one 4-way LDS step, and stores
//     T complex results: algorithmic traffic 8*N + 8*T bytes per job;
//   * blockIdx is remapped so that consecutive jobs (host order: epoch-major, channel-minor,
//     i.e. jobs that read the same samples) run on the same XCD and share its L2.
//
// This header is the kernel text, and only that.  A translation unit defines GSH_MC_THREADS (mcorr_device.h: 256 unless told otherwise), includes it ONCE and
// instantiates the flavours it launches: multicorrelator.hip every flavour at 256 threads (four waves per job), multicorrelator_t128.hip the E/P/L whole-code
// flavours and the walk at 128 (two waves per job; it names the template mcorr_kernel_t128 so that a profile tells the two sizes apart, and defines
// GSH_MC_VARIANT_128, which the walk kernel below exists under).  The kernels have internal linkage: what a unit does not launch it does not build.
#ifndef GSH_MCORR_KERNELS_H
#define GSH_MCORR_KERNELS_H

#include "multicorrelator.h"
#include "mcorr_device.h"
#include <cmath>

namespace gsh
{
namespace
{
using namespace mcdev;
static_assert(FAC_ENTRIES == MCORR_FAC_ENTRIES, "the host's LDS sizes (mcorr_lds_bytes*) and the kernel's factor table");
#ifndef GSH_MC_MIN_WAVES
#define GSH_MC_MIN_WAVES 5  // E/P/L: the packed body holds four accumulator sets; <= 96 VGPRs (5 waves per SIMD), the kernel is VALU-issue bound
#endif

#ifndef GSH_MC_RUN_LEN
#define GSH_MC_RUN_LEN 8
#endif
constexpr int MC_RUN_LEN = GSH_MC_RUN_LEN;  // samples per lane run of the run-based path (mcorr_device.h)

// WIN: the launch stages per-segment windows of the codes (a.window_floats > 0); otherwise every work-group stages its whole code at the start of the
// LDS and the look-ups use a constant offset
// PAIR: every job of the launch is pair_eligible (the host checked, a.pair): the early tap is read next to the late one
// HALF: and its shifts are exactly -0.5 / 0 / +0.5 chip, its code at most MC_HALF_MAX_CODE_LEN long (a.half): all three taps from the prompt's index chain
//       and a doubled code table at the start of the LDS, the plain table behind it (mcorr_device.h packed_trip)
template <int NT, int MODE, bool AUX, bool RUNS = false, bool WIN = false, bool PAIR = false, bool HALF = false>
__global__ __launch_bounds__(MC_THREADS, ((NT <= 3 && !AUX) ? GSH_MC_MIN_WAVES : 1)) void mcorr_kernel(McorrArgs a)
{
    static_assert(!PAIR || (NT == 3 && MODE == 0 && !AUX && !RUNS), "paired taps: the plain E/P/L launch");
    static_assert(!HALF || (PAIR && !WIN), "half-chip taps: a paired-tap launch with whole-code tables");
    static_assert(!RUNS || (MODE == 0 && !AUX), "the run-based path exists for the standard mode without a fused tap");
    extern __shared__ __align__(16) float lds[];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int slot = static_cast<int>(lb) / a.splits;
    const int split = static_cast<int>(lb) - slot * a.splits;
    const int job = a.job_list ? a.job_list[slot] : slot;
    const gsh_corr_job& J = a.jobs[job];
    const int tid = threadIdx.x;
    const int aux_job = AUX ? a.aux[job] : -1;
    if (AUX && aux_job == -2) return;  // computed (and its output row written) by the job in front of it

    JobCtx c;
    c.n_total = J.n_samples;
    c.code_len = a.code_lens[J.code_slot];
    c.rem_carr = J.rem_carr_phase_rad;
    c.phase_step = J.phase_step_rad;
    c.phase_rate = J.phase_rate_step_rad;
    c.rem_code = J.rem_code_phase_chips;
    c.code_step = J.code_phase_step_chips;
    c.code_rate = J.code_phase_rate_step_chips;
    c.packed = a.packed != 0;
    c.runs = RUNS && a.packed == 2;

    // ---- this work-group's slice of the window
    int seg = (c.n_total + a.splits - 1) / a.splits;
    seg = (seg + 1) & ~1;
    c.n_begin = min(split * seg, c.n_total);
    c.n_end = min(c.n_total, c.n_begin + seg);
    unsigned long long win0 = J.sample_offset + a.sample_base;
    if (a.ring_capacity) win0 %= a.ring_capacity;
    const unsigned long long abs0 = win0 + static_cast<unsigned long long>(c.n_begin);
    const int odd = static_cast<int>(abs0 & 1ULL);
    c.n_first = c.n_begin - odd;
    const float2* __restrict__ base = a.stream + (abs0 - static_cast<unsigned long long>(odd));  // 16-byte aligned

    float sh[NT];
    int rot[NT];
#pragma unroll
    // unused slots (jobs with fewer taps than the kernel flavour) repeat the last real shift: the index range [lo, hi] below then equals the
    // one the host sized the code window for (bank_window_floats spans the real taps only); their sums are never stored
    for (int t = 0; t < NT; t++) sh[t] = J.shifts_chips[min(t, max(J.n_taps, 1) - 1)];
    rot[0] = 0;
    if (mode_hd_code(MODE))
        {
            // K/..high_dynamics_resampler..:82-85: shift_samples += (int)round((shift[t]-shift[t-1])/step)
            unsigned accum = 0;
#pragma unroll
            for (int t = 1; t < NT; t++)
                {
                    if (t < J.n_taps) accum += static_cast<unsigned>(static_cast<int>(roundf(__fdiv_rn(__fsub_rn(sh[t], sh[t - 1]), c.code_step))));
                    rot[t] = static_cast<int>(accum);
                }
        }
    else
        {
#pragma unroll
            for (int t = 1; t < NT; t++) rot[t] = 0;
        }

    // the raw chip index is monotone in n and in the shift (every rounding is monotone) when step >= 0: its range over this
    // segment is [lo, hi], evaluated with the very expressions the samples use
    int lo = 0, hi = -1;
    if (!mode_hd_code(MODE) && c.n_end > c.n_begin)
        {
            float smin = sh[0], smax = sh[0];
#pragma unroll
            for (int t = 1; t < NT; t++)
                {
                    smin = fminf(smin, sh[t]);
                    smax = fmaxf(smax, sh[t]);
                }
            lo = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_begin)), smin, c.rem_code);
            hi = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_end - 1)), smax, c.rem_code);
        }

    // ---- stage the local code in LDS: the whole code (+ guard bands holding the wrapped neighbours), or -- when the host found that
    // every segment of this launch touches only a short run of it (long codes, split windows) -- just the samples lo..hi, so that a
    // 10 230-chip code does not cost 41 KB of LDS per work-group and with it most of the compute unit's occupancy
    float* tab = lds + (HALF ? MC_HALF_WORDS : 0);
    const float* __restrict__ gcode = a.codes + static_cast<size_t>(J.code_slot) * a.code_stride;
    bool windowed = false, misfit = false, aux_fast = true;
    int lds_floats;
    typedef const __attribute__((address_space(3))) float* lds_float_ptr;
    const bool pair_ok = (!PAIR || gsh::mcorr_pair_eligible(J.n_taps, J.shifts_chips, J.code_phase_step_chips, J.high_dyn))
                         && (!HALF || gsh::mcorr_half_chip_eligible(J.n_taps, J.shifts_chips, J.code_phase_step_chips, J.high_dyn, c.code_len));
    if (WIN != (a.window_floats > 0) || !pair_ok || (!WIN && reinterpret_cast<size_t>((lds_float_ptr)lds) != 0))  // (this kernel has no static LDS: the dynamic array starts at 0)
        {
            misfit = (c.n_end > c.n_begin);  // cannot happen: the launcher picks the flavour from the same field; reported as NaN if it does
            lds_floats = a.window_floats > 0 ? a.window_floats : c.code_len + 2 * MC_MARGIN;
        }
    else if (a.window_floats > 0)
        {
            const long long span = static_cast<long long>(hi) - lo + 1;
            if (!mode_hd_code(MODE) && c.code_step >= 0.0f && span >= 1 && span <= a.window_floats)
                {
                    windowed = true;
                    for (int i = tid; i < static_cast<int>(span); i += MC_THREADS) tab[i] = gcode[wrap_chip(lo + i, c.code_len)];
                    c.k_lo = lo;
                    c.k_hi = hi;
                    c.k_off = -lo;
                }
            else
                misfit = (c.n_end > c.n_begin);  // cannot happen for a batch the host admitted (bank_window_floats); reported as NaN if it does
            lds_floats = a.window_floats;
        }
    else if constexpr (HALF)
        {
            // both tables are a copy of the image the host built when the code was set (multicorrelator.h mcorr_build_half_image: doubled table, plain table, guard bands
            // and all, laid out as the LDS is): 16-byte rows, first those the doubled table fills, then those of the plain one.  (Built here, element by element, the two
            // tables cost every thread 8 loads, 16 LDS stores and their addresses -- in each of a launch's 12 800 work-groups, for a content that changes with the satellite.)
            // The last row of either table may reach up to three words beyond it: zeros of the image, into the padding in front of MC_HALF_WORDS / of `red`.
            static_assert(MC_MARGIN == MCORR_MARGIN && MC_HALF_WORDS == MCORR_HALF_WORDS, "the host's image and the kernel's LDS layout");
            const int tab_len = c.code_len + 2 * MC_MARGIN;
            const int rows_dbl = (2 * tab_len + 3) >> 2, rows = rows_dbl + ((tab_len + 3) >> 2);
            // every load goes out before the first store waits for one (a loop of load, wait, store pays the L2 round trip once per row); a thread with fewer rows than
            // the others copies the last row again -- no branch, the same value to the same place.  A row's byte offset is the same in the image and in the LDS.
            const char* const image = reinterpret_cast<const char*>(a.code_images + static_cast<size_t>(J.code_slot) * MCORR_HALF_IMAGE_WORDS);
            constexpr int PER_THREAD = (MCORR_HALF_IMAGE_WORDS / 4 + MC_THREADS - 1) / MC_THREADS;
            const unsigned last = 16u * static_cast<unsigned>(rows - 1), end_dbl = 16u * static_cast<unsigned>(rows_dbl);
            const unsigned skip = 4u * MC_HALF_WORDS - end_dbl;  // from the doubled table's last row to the plain table's first
            unsigned at[PER_THREAD];
            float4 row[PER_THREAD];
            typedef float row_t __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) row_t* lds_row_ptr;
#pragma unroll
            for (int i = 0; i < PER_THREAD; i++)
                {
                    const unsigned r = min(16u * static_cast<unsigned>(tid + i * MC_THREADS), last);
                    at[i] = r < end_dbl ? r : r + skip;
                    row[i] = *reinterpret_cast<const float4*>(image + at[i]);
                }
#pragma unroll
            for (int i = 0; i < PER_THREAD; i++)  // (the dynamic LDS starts at address 0, checked above: the byte offset IS the address, one ds_write_b128)
                *reinterpret_cast<lds_row_ptr>(at[i]) = (row_t){row[i].x, row[i].y, row[i].z, row[i].w};
            lds_floats = tab_len + MC_HALF_WORDS;
        }
    else
        {
            // the code itself: straight copies (no wrap arithmetic); then the two guard bands, one element per thread of the first wave
            // (the single loop with a wrap per element cost ~150 VALU instructions per wave -- 7 % of everything a wave executes for a 25 000-sample window)
            const int tab_len = c.code_len + 2 * MC_MARGIN;
            for (int j = tid; j < c.code_len; j += MC_THREADS) tab[MC_MARGIN + j] = gcode[j];
            if (tid < 2 * MC_MARGIN)
                {
                    const int k = tid < MC_MARGIN ? tid - MC_MARGIN : c.code_len + (tid - MC_MARGIN);  // -MARGIN .. -1, len .. len + MARGIN - 1
                    tab[MC_MARGIN + k] = gcode[wrap_margin(k, c.code_len)];
                }
            lds_floats = AUX ? a.code_stride + 2 * MC_MARGIN : tab_len;
        }
    // ---- the fused correlator's code (AUX): a second table behind the first
    if (AUX && aux_job >= 0 && !misfit)
        {
            const gsh_corr_job& J2 = a.jobs[aux_job];
            const float* __restrict__ gcode2 = a.codes + static_cast<size_t>(J2.code_slot) * a.code_stride;
            c.aux_on = true;
            c.aux_shift = J2.shifts_chips[0];
            c.aux_zero = (c.aux_shift == 0.0f);
            c.aux_code_len = a.code_lens[J2.code_slot];
            const int aux_base = (lds_floats + 3) & ~3;
            int lo2 = 0, hi2 = -1;
            if (c.n_end > c.n_begin)
                {
                    lo2 = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_begin)), c.aux_shift, c.rem_code);
                    hi2 = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_end - 1)), c.aux_shift, c.rem_code);
                }
            if (a.window_floats > 0)
                {
                    const long long span2 = static_cast<long long>(hi2) - lo2 + 1;
                    if (windowed && span2 >= 1 && span2 <= a.window_floats)
                        {
                            for (int i = tid; i < static_cast<int>(span2); i += MC_THREADS) tab[aux_base + i] = gcode2[wrap_chip(lo2 + i, c.aux_code_len)];
                            c.aux_k_lo = lo2;
                            c.aux_k_hi = hi2;
                            c.aux_k_off = aux_base - lo2;
                        }
                    else
                        misfit = (c.n_end > c.n_begin);
                }
            else
                {
                    const int tab_len2 = c.aux_code_len + 2 * MC_MARGIN;
                    for (int i = tid; i < tab_len2; i += MC_THREADS) tab[aux_base + i] = gcode2[wrap_margin(i - MC_MARGIN, c.aux_code_len)];
                    c.aux_k_off = aux_base + MC_MARGIN;
                    aux_fast = (lo2 >= -MC_MARGIN) && (hi2 < c.aux_code_len + MC_MARGIN) && (c.aux_code_len >= MC_MARGIN);
                }
            lds_floats = aux_base + (a.window_floats > 0 ? a.window_floats : a.code_stride + 2 * MC_MARGIN);
        }
    else if (AUX)
        lds_floats = ((lds_floats + 3) & ~3) + (a.window_floats > 0 ? a.window_floats : a.code_stride + 2 * MC_MARGIN);  // same `red` place for every work-group
    float2* red = reinterpret_cast<float2*>(lds + ((lds_floats + 3) & ~3));
    // ---- the factors of every lane's carrier seeds for this job (mcorr_device.h fac_table_fill): one evaluation per lane of the first wave, beside the staging
    float2* const fac = red + MC_WAVES * GSH_MAX_TAPS;
    if constexpr (MODE == 0 && MC_THREADS <= 256)
        {
            if (a.packed != 0 && a.fac != 0)
                {
                    if ((tid >> 6) == 0) fac_table_fill<2>(fac, c.phase_step, c.rem_carr, c.n_first, tid);
                    c.fac_tab = fac;
                }
        }

    float2 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = make_float2(0.0f, 0.0f);
    float2 acc_aux = make_float2(0.0f, 0.0f);

    __syncthreads();  // code table(s) visible

    if (misfit)
        {
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
            acc_aux = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        }
    else if (c.n_end > c.n_begin)
        {
            // skip the per-sample wrap when the indices stay inside what is staged
            const bool fast = windowed || (!mode_hd_code(MODE) && (c.code_step >= 0.0f) && (lo >= -MC_MARGIN) && (hi < c.code_len + MC_MARGIN) && (c.code_len >= MC_MARGIN) && aux_fast);
            // centre tap at exactly 0 (E/P/L, VE/E/P/L/VL): its (a + 0.0f) is skipped; needs sample indices exact in float
            const bool zp = (NT & 1) && (NT == J.n_taps) && (sh[NT / 2] == 0.0f) && !mode_hd_code(MODE) && (c.n_total < (1 << 24));
            if (RUNS && fast && c.runs && c.code_step > 1.0e-6f && c.n_total < (1 << 24))
                {
                    if constexpr (RUNS)
                        {
                            float* const runs_lds = reinterpret_cast<float*>(fac + FAC_ENTRIES) + (tid >> 6) * RunsLayout<MC_RUN_LEN>::FLOATS;
                            run_segment_runs<NT, MC_RUN_LEN>(c, base, tab, sh, acc, runs_lds);
                        }
                }
            else if (fast && zp)
                run_segment<NT, MODE, false, true, AUX, !WIN, PAIR, HALF>(c, base, tab, sh, rot, acc, &acc_aux);
            else if (fast)
                run_segment<NT, MODE, false, false, AUX, !WIN && !HALF>(c, base, tab, sh, rot, acc, &acc_aux);  // (constant look-up offsets: the table at LDS address 0)
            else
                run_segment<NT, MODE, true, false, AUX>(c, base, tab, sh, rot, acc, &acc_aux);
        }

    // ---- integrate-and-dump: wave64 prefix sum in DPP steps (the last lane holds the wave's sum; six v_add_f32_dpp per value instead of the
    // ds_bpermute + address + add of a shuffle tree), then one LDS step over the 4 waves
    {
        float sums[2 * NT + (AUX ? 2 : 0)];
#pragma unroll
        for (int t = 0; t < NT; t++)
            {
                sums[2 * t] = acc[t].x;
                sums[2 * t + 1] = acc[t].y;
            }
        if (AUX)
            {
                sums[2 * NT] = acc_aux.x;
                sums[2 * NT + 1] = acc_aux.y;
            }
        wave_scan_incl_n(sums);
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t] = make_float2(sums[2 * t], sums[2 * t + 1]);
        if (AUX) acc_aux = make_float2(sums[2 * NT], sums[2 * NT + 1]);
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 63)
        {
#pragma unroll
            for (int t = 0; t < NT; t++) red[wave * GSH_MAX_TAPS + t] = acc[t];
            if (AUX) red[wave * GSH_MAX_TAPS + NT] = acc_aux;  // NT < GSH_MAX_TAPS in the AUX kernels
        }
    __syncthreads();
    if (AUX && aux_job >= 0 && tid >= GSH_MAX_TAPS && tid < 2 * GSH_MAX_TAPS)
        {
            // the fused job's whole output row: its one tap, zeros behind it
            const int tap = tid - GSH_MAX_TAPS;
            float2 s = make_float2(0.0f, 0.0f);
            if (tap == 0)
                {
#pragma unroll
                    for (int w = 0; w < MC_WAVES; w++)
                        {
                            s.x += red[w * GSH_MAX_TAPS + NT].x;
                            s.y += red[w * GSH_MAX_TAPS + NT].y;
                        }
                }
            if (a.splits == 1)
                a.out[static_cast<size_t>(aux_job) * GSH_MAX_TAPS + tap] = s;
            else
                a.partials[(static_cast<size_t>(aux_job) * a.splits + split) * GSH_MAX_TAPS + tap] = s;
        }
    if (tid < GSH_MAX_TAPS)
        {
            float2 s = make_float2(0.0f, 0.0f);
            if (tid < NT && tid < J.n_taps)
                {
#pragma unroll
                    for (int w = 0; w < MC_WAVES; w++)
                        {
                            s.x += red[w * GSH_MAX_TAPS + tid].x;
                            s.y += red[w * GSH_MAX_TAPS + tid].y;
                        }
                }
            if (a.splits == 1)
                a.out[static_cast<size_t>(job) * GSH_MAX_TAPS + tid] = s;
            else
                a.partials[(static_cast<size_t>(job) * a.splits + split) * GSH_MAX_TAPS + tid] = s;
        }
}

#ifdef GSH_MC_VARIANT_128
// The walk (round 11): mcorr_kernel_t128<3, 0, false, false, false, true, true> -- E/P/L, standard mode, whole-code tables, paired taps, half-chip shifts, one
// work-group per job, no splits -- with its body inside a loop over job slots.  The grid is ONE resident round of work-groups (walk_grid, its unit: G = what the chip
// holds); work-group lb takes the slots lb, lb + G, lb + 2 G, ... of the launch.  A launch of 12 800 such jobs is otherwise five lock-step rounds of 2 560
// work-groups, and at the end of each round every wave slot stands empty while its successor is dispatched and goes through the dependent set-up (job record, code
// length, 13 KB of code image into LDS, barrier, first samples) before its first trip.  Along a walk
//   * a wave slot is handed over once per launch, not once per job;
//   * the code image is staged when the job's code slot differs from the one the LDS holds (the job table is epoch-major, channel-minor: with G a multiple of the
//     channel count a work-group meets the same code slot every time), which does not depend on G: any grid is CORRECT;
//   * everything else -- factor table, judgement, accumulators, JobCtx, fold, wave sums, the job's own output row -- is the parent's, per job: the same lanes take
//     the same samples, the same products enter the same sums in the same order, and the outputs are the parent's bit for bit (tests/test_tracking_walk_gpu.py).
// What keeps the loop at the parent's registers (profiles/ab/r06/chain_kernel.patch learned both):
//   * the arguments are read per job THROUGH A POINTER into the kernarg segment that is made opaque at the head of every job, not from the by-value parameter: what
//     the compiler knows to be invariant it keeps in SGPRs across the whole loop, thirty-odd registers the trip loops do not need;
//   * the job table, the launch list and the code lengths are read through the constant address space (nothing writes them while the kernel runs): scalar loads,
//     although the loop's own output stores lie between one job's reads and the next one's.
// Barriers: two per job, as in the parent -- B1 "tables visible", B2 "red written".  No third one between job k's reduction and job k + 1's writes while the code
// slot stays:
//   * after B2 only the first wave reads `red` of job k (tid < GSH_MAX_TAPS).  Before B1 of job k + 1 the first wave writes `fac` (the same wave, behind its own
//     reads, at another address: the layout depends on the code length only, and the slot is the same), and nobody writes the code tables; `red` of job k + 1 is
//     written after B1 of job k + 1, which the first wave enters only with its reads of job k complete (the barrier's fence waits for them);
//   * `fac` of job k is read by both waves inside the trips, i.e. before B2 of job k; it is rewritten after B2;
//   * the code tables are read before B2 of job k and not written at all.
// When the slot CHANGES the other wave may start to overwrite the tables -- with another code length, at the place of job k's `red` -- while the first wave still
// sums job k: that path, and only that path, begins with a barrier of its own.
// The register budget is the parent's, 96 (five waves per SIMD), and tests/test_tracking_walk_resources.py holds the kernel to it.  The bound ASKED of the compiler is
// four waves: inside the loop over jobs it hoists the constants of every inlined carrier-seed evaluation (four registers) and one constant pair of the half-chip
// set-up in front of the loop, and held to 96 from the outset it parks that pair in scratch (12 bytes: one store per wave, one load per job -- and a kernel that uses
// scratch at all); free to take 128 it allocates exactly 96 and spills nothing.
#ifndef GSH_MC_WALK_MIN_WAVES
#define GSH_MC_WALK_MIN_WAVES 4
#endif
#ifndef GSH_MC_WALK_PRIO
#define GSH_MC_WALK_PRIO 1  // a walk's issue priority falls with the jobs it has left (below); 0: every wave at the default priority (A/B: profiles/r11_summary.txt)
#endif
__global__ __launch_bounds__(MC_THREADS, GSH_MC_WALK_MIN_WAVES) void mcorr_walk_kernel_t128(McorrArgs args_in_kernarg_segment)
{
    constexpr int NT = 3;
    (void)args_in_kernarg_segment;
    typedef const __attribute__((address_space(4))) McorrArgs* kernarg_ptr;
    typedef const __attribute__((address_space(4))) gsh_corr_job* job_ptr;
    typedef const __attribute__((address_space(4))) int* const_int_ptr;
    typedef const __attribute__((address_space(3))) float* lds_float_ptr;
    extern __shared__ __align__(16) float lds[];
    int staged = -1;  // the code slot whose image the LDS holds
    int tid = threadIdx.x;
    for (unsigned slot = xcd_remap(blockIdx.x, gridDim.x);; slot += gridDim.x)
        {
            kernarg_ptr ap = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ap));
#define a (*ap)
            if (slot >= static_cast<unsigned>(a.n_launch)) break;
#if GSH_MC_WALK_PRIO
            {
                // A SIMD issues by priority, then by age: among five resident waves of equal priority the oldest wins every tie, for the whole launch, and finishes its
                // walk long before the youngest -- the slots it leaves stay empty (one resident round: nothing is waiting for them) and the stragglers run on a
                // half-empty SIMD.  The jobs a walk still has in front of it are its priority: a wave that is ahead yields to those behind it.
                const unsigned left = (static_cast<unsigned>(a.n_launch) - 1u - slot) / gridDim.x;
                if (left >= 3u)
                    __builtin_amdgcn_s_setprio(3);
                else if (left == 2u)
                    __builtin_amdgcn_s_setprio(2);
                else if (left == 1u)
                    __builtin_amdgcn_s_setprio(1);
                else
                    __builtin_amdgcn_s_setprio(0);
            }
#endif
            asm volatile("" : "+v"(tid));  // (opaque, in place: no lane arithmetic derived from it is hoisted out of the loop and kept across all of it)
            const int job = a.job_list ? ((const_int_ptr)a.job_list)[slot] : static_cast<int>(slot);
            const job_ptr Jp = (job_ptr)a.jobs + job;
            const int code_slot = Jp->code_slot, n_taps = Jp->n_taps;
            const float jsh[NT] = {Jp->shifts_chips[0], Jp->shifts_chips[1], Jp->shifts_chips[2]};

            JobCtxLooped c;
            c.n_total = Jp->n_samples;
            c.code_len = ((const_int_ptr)a.code_lens)[code_slot];
            c.rem_carr = Jp->rem_carr_phase_rad;
            c.phase_step = Jp->phase_step_rad;
            c.phase_rate = Jp->phase_rate_step_rad;
            c.rem_code = Jp->rem_code_phase_chips;
            c.code_step = Jp->code_phase_step_chips;
            c.code_rate = Jp->code_phase_rate_step_chips;
            c.packed = a.packed != 0;
            c.runs = false;
            c.tid = tid;

            // ---- the window (splits == 1: the whole of it)
            c.n_begin = 0;
            c.n_end = c.n_total;
            unsigned long long win0 = Jp->sample_offset + a.sample_base;
            if (a.ring_capacity) win0 %= a.ring_capacity;
            const int odd = static_cast<int>(win0 & 1ULL);
            c.n_first = -odd;
            const float2* __restrict__ base = a.stream + (win0 - static_cast<unsigned long long>(odd));  // 16-byte aligned

            // unused slots repeat the last real shift, as in mcorr_kernel (a job with fewer than three taps is a misfit here: its shifts are never used)
            const int last_tap = max(n_taps, 1) - 1;
            float sh[NT];
            int rot[NT];
            sh[0] = jsh[0];
            sh[1] = last_tap >= 1 ? jsh[1] : jsh[0];
            sh[2] = last_tap >= 2 ? jsh[2] : sh[1];
#pragma unroll
            for (int t = 0; t < NT; t++) rot[t] = 0;

            int lo = 0, hi = -1;
            if (c.n_end > c.n_begin)
                {
                    const float smin = fminf(fminf(sh[0], sh[1]), sh[2]), smax = fmaxf(fmaxf(sh[0], sh[1]), sh[2]);
                    lo = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_begin)), smin, c.rem_code);
                    hi = raw_chip_std(__fmul_rn(c.code_step, static_cast<float>(c.n_end - 1)), smax, c.rem_code);
                }

            // ---- the code image, when the LDS does not hold it already (mcorr_kernel, HALF, explains the copy)
            float* const tab = lds + MC_HALF_WORDS;
            bool misfit = false;
            int lds_floats;
            const bool pair_ok = gsh::mcorr_half_chip_eligible(n_taps, jsh, c.code_step, Jp->high_dyn, c.code_len);
            if (a.window_floats > 0 || !pair_ok || reinterpret_cast<size_t>((lds_float_ptr)lds) != 0)
                {
                    misfit = (c.n_end > c.n_begin);  // cannot happen: the launcher picks this kernel from the same fields; reported as NaN if it does
                    lds_floats = a.window_floats > 0 ? a.window_floats : c.code_len + 2 * MC_MARGIN;
                    if (staged >= 0) __syncthreads();  // `red` of this job lies inside the tables: the first wave may still sum the job before
                    staged = -1;
                }
            else
                {
                    const int tab_len = c.code_len + 2 * MC_MARGIN;
                    if (code_slot != staged)  // uniform over the work-group
                        {
                            if (staged >= 0) __syncthreads();  // (see above: the first wave may still read `red` of the job before, where this table will lie)
                            const int rows_dbl = (2 * tab_len + 3) >> 2, rows = rows_dbl + ((tab_len + 3) >> 2);
                            const char* const image = reinterpret_cast<const char*>(a.code_images + static_cast<size_t>(code_slot) * MCORR_HALF_IMAGE_WORDS);
                            constexpr int PER_THREAD = (MCORR_HALF_IMAGE_WORDS / 4 + MC_THREADS - 1) / MC_THREADS;
                            const unsigned last = 16u * static_cast<unsigned>(rows - 1), end_dbl = 16u * static_cast<unsigned>(rows_dbl);
                            const unsigned skip = 4u * MC_HALF_WORDS - end_dbl;  // from the doubled table's last row to the plain table's first
                            unsigned at[PER_THREAD];
                            float4 row[PER_THREAD];
                            typedef float row_t __attribute__((ext_vector_type(4)));
                            typedef __attribute__((address_space(3))) row_t* lds_row_ptr;
#pragma unroll
                            for (int i = 0; i < PER_THREAD; i++)
                                {
                                    const unsigned r = min(16u * static_cast<unsigned>(tid + i * MC_THREADS), last);
                                    at[i] = r < end_dbl ? r : r + skip;
                                    row[i] = *reinterpret_cast<const float4*>(image + at[i]);
                                }
#pragma unroll
                            for (int i = 0; i < PER_THREAD; i++) *reinterpret_cast<lds_row_ptr>(at[i]) = (row_t){row[i].x, row[i].y, row[i].z, row[i].w};
                            staged = code_slot;
                        }
                    lds_floats = tab_len + MC_HALF_WORDS;
                }
            float2* red = reinterpret_cast<float2*>(lds + ((lds_floats + 3) & ~3));
            float2* const fac = red + MC_WAVES * GSH_MAX_TAPS;
            if (a.packed != 0 && a.fac != 0)
                {
                    if ((tid >> 6) == 0) fac_table_fill<2>(fac, c.phase_step, c.rem_carr, c.n_first, tid);
                    c.fac_tab = fac;
                }

            float2 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t] = make_float2(0.0f, 0.0f);
            float2 acc_aux = make_float2(0.0f, 0.0f);

            __syncthreads();  // B1: code tables and factor table visible

            if (misfit)
                {
#pragma unroll
                    for (int t = 0; t < NT; t++) acc[t] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
                }
            else if (c.n_end > c.n_begin)
                {
                    const bool fast = (c.code_step >= 0.0f) && (lo >= -MC_MARGIN) && (hi < c.code_len + MC_MARGIN) && (c.code_len >= MC_MARGIN);
                    const bool zp = (NT == n_taps) && (sh[NT / 2] == 0.0f) && (c.n_total < (1 << 24));
                    if (fast && zp)
                        run_segment<NT, 0, false, true, false, true, true, true>(c, base, tab, sh, rot, acc, &acc_aux);
                    else if (fast)
                        run_segment<NT, 0, false, false, false, false>(c, base, tab, sh, rot, acc, &acc_aux);
                    else
                        run_segment<NT, 0, true, false, false>(c, base, tab, sh, rot, acc, &acc_aux);
                }

            // ---- integrate-and-dump, as in mcorr_kernel
            {
                float sums[2 * NT];
#pragma unroll
                for (int t = 0; t < NT; t++)
                    {
                        sums[2 * t] = acc[t].x;
                        sums[2 * t + 1] = acc[t].y;
                    }
                wave_scan_incl_n(sums);
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = make_float2(sums[2 * t], sums[2 * t + 1]);
            }
            const int wave = tid >> 6;
            if ((tid & 63) == 63)
                {
#pragma unroll
                    for (int t = 0; t < NT; t++) red[wave * GSH_MAX_TAPS + t] = acc[t];
                }
            __syncthreads();  // B2: `red` written
            if (tid < GSH_MAX_TAPS)
                {
                    float2 s = make_float2(0.0f, 0.0f);
                    if (tid < NT && tid < n_taps)
                        {
#pragma unroll
                            for (int w = 0; w < MC_WAVES; w++)
                                {
                                    s.x += red[w * GSH_MAX_TAPS + tid].x;
                                    s.y += red[w * GSH_MAX_TAPS + tid].y;
                                }
                        }
                    a.out[static_cast<size_t>(job) * GSH_MAX_TAPS + tid] = s;
                }
#undef a
        }
}
#endif  // GSH_MC_VARIANT_128
}  // namespace
}  // namespace gsh

#endif
