// The batched E/P/L multicorrelator's launcher, and its kernels at 256 threads (four waves per job: every flavour).  The kernel text and the design notes are
// csrc/mcorr_kernels.h.
//
// Two work-group sizes of one kernel text (round 6): multicorrelator_t128.hip includes the same header with GSH_MC_THREADS = 128 and builds the E/P/L whole-code
// flavours with TWO waves per job, behind one entry (mcorr_launch_epl_t128).  What a job costs besides its trips -- set-up, edge trips, fold, wave sums: ~330
// vector instructions per WAVE (profiles/ab/r06/session5.txt) -- is then paid twice, not four times: 5 928 instead of 6 689 vector instructions per 25 000-sample
// job, 173 us instead of 184 per launch of 12 800 jobs.  With few jobs in flight (closed-loop batches, split windows) four waves per job finish a job sooner and
// keep the chip fuller: launch_class picks per launch (use_128).  Every launch of the bank goes through launch_class, whichever entry it came by, and the
// partials of a split launch are summed once, behind the last class (reduce_if_split).
#include "mcorr_kernels.h"
#include <cstdlib>

namespace gsh
{
namespace
{
// sums the per-split partials of each job in split order (deterministic)
__global__ __launch_bounds__(256) void mcorr_reduce_partials(const float2* __restrict__ partials, float2* __restrict__ out, int n_jobs, int splits)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // job*GSH_MAX_TAPS + tap
    if (i >= n_jobs * GSH_MAX_TAPS) return;
    const int job = i / GSH_MAX_TAPS, tap = i - job * GSH_MAX_TAPS;
    float2 s = make_float2(0.0f, 0.0f);
    for (int k = 0; k < splits; k++)
        {
            const float2 p = partials[(static_cast<size_t>(job) * splits + k) * GSH_MAX_TAPS + tap];
            s.x += p.x;
            s.y += p.y;
        }
    out[i] = s;
}

// lds_half: the LDS bytes of the half-chip flavour for this launch's codes (mcorr_lds_bytes_half), 0 when they are too long for it
template <int NT>
int launch_nt(const McorrArgs& a, int mode, size_t lds, size_t lds_half, hipStream_t stream)
{
    const dim3 grid(static_cast<unsigned>(a.n_launch) * static_cast<unsigned>(a.splits));
    const dim3 block(MC_THREADS);
    if (a.aux != nullptr)
        {
            if constexpr (NT == 3 || NT == 5)
                {
                    GSH_REQUIRE(mode == 0, "fused jobs need the standard mode");
                    if (a.window_floats > 0)
                        hipLaunchKernelGGL((mcorr_kernel<NT, 0, true, false, true>), grid, block, lds, stream, a);
                    else
                        hipLaunchKernelGGL((mcorr_kernel<NT, 0, true>), grid, block, lds, stream, a);
                    GSH_HIP(hipGetLastError());
                    return GSH_OK;
                }
            else
                return set_error(GSH_ERR_INVALID, "fused jobs exist only for the 3- and 5-tap kernels");
        }
    switch (mode)
        {
        case 0:
#ifdef GSH_MC_RUNS_EXPERIMENT  // the run-based body (round 2, slower, 16 - 32 B of scratch per thread): only in a library built with this macro (profiles/ab/build_variant.py)
            if constexpr (NT <= 5)
                {
                    if (a.packed == 2 && a.window_floats == 0)
                        {
                            const size_t lds_runs = lds + static_cast<size_t>(MC_WAVES) * RunsLayout<MC_RUN_LEN>::FLOATS * sizeof(float);
                            if (lds_runs <= 64 * 1024)  // beyond that the scratch costs more occupancy than the path gains
                                {
                                    hipLaunchKernelGGL((mcorr_kernel<NT, 0, false, true>), grid, block, lds_runs, stream, a);
                                    break;
                                }
                        }
                }
#endif
            if constexpr (NT == 3)
                {
                    if (a.pair && a.packed == 1)
                        {
                            if (a.window_floats > 0)
                                hipLaunchKernelGGL((mcorr_kernel<NT, 0, false, false, true, true>), grid, block, lds, stream, a);
                            else if (a.half && lds_half > 0 && a.code_images != nullptr)
                                hipLaunchKernelGGL((mcorr_kernel<NT, 0, false, false, false, true, true>), grid, block, lds_half, stream, a);
                            else
                                hipLaunchKernelGGL((mcorr_kernel<NT, 0, false, false, false, true>), grid, block, lds, stream, a);
                            break;
                        }
                }
            if (a.window_floats > 0)
                hipLaunchKernelGGL((mcorr_kernel<NT, 0, false, false, true>), grid, block, lds, stream, a);
            else
                hipLaunchKernelGGL((mcorr_kernel<NT, 0, false>), grid, block, lds, stream, a);
            break;
        case 1:
            hipLaunchKernelGGL((mcorr_kernel<NT, 1, false>), grid, block, lds, stream, a);
            break;
        case 2:
            hipLaunchKernelGGL((mcorr_kernel<NT, 2, false>), grid, block, lds, stream, a);
            break;
        default:
            return set_error(GSH_ERR_INVALID, "unknown correlator mode %d", mode);
        }
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

// what every work-group keeps behind its code table(s): a row of sums per wave, the factor table of the carrier seeds
size_t lds_tail_bytes(int waves) { return (static_cast<size_t>(waves) * GSH_MAX_TAPS + MCORR_FAC_ENTRIES) * sizeof(float2); }

// work-group size of a launch: 128 threads (two waves per job) for the E/P/L whole-code flavours once the launch holds at least two rounds of them (2 x 2 560
// work-groups: a job then takes twice as long, and a chip that is not full wants the shorter jobs); GSH_MC_WG=128 / 256 forces one (A/B runs)
bool use_128(const McorrArgs& a, int class_taps, int mode)
{
    static const int forced = [] {
        const char* e = std::getenv("GSH_MC_WG");
        return e != nullptr ? std::atoi(e) : 0;
    }();
    // (packed == 3, the A/B switch that turns the paired and half-chip trips off, keeps the work-group size of the launch it is compared with: the order of summation
    //  depends on it, and tests/test_tracking_half_chip_taps_gpu.py holds the two-wave kernels' fast trips bit-identical to their per-tap trips that way)
    const bool possible = mode == 0 && a.aux == nullptr && a.window_floats == 0 && class_taps == 3 && (a.packed == 1 || a.packed == 3);
    if (!possible || forced == 256) return false;
    if (forced == 128) return true;
    return static_cast<long long>(a.n_launch) * a.splits >= 2 * 2560;
}

// tap class of a job (or of a launch's largest job): the kernel flavours hold 1, 3, 5 or GSH_MAX_TAPS accumulator sets
int tap_class(int n_taps) { return n_taps <= 1 ? 1 : (n_taps <= 3 ? 3 : (n_taps <= 5 ? 5 : GSH_MAX_TAPS)); }

// One launch: the jobs a.job_list / a.n_launch names, through the kernels of `class_taps` taps, at the work-group size use_128 picks.  The partials of a split
// launch stay where they are (reduce_if_split).
int launch_class(const McorrArgs& a, int class_taps, int mode, int max_code_len, hipStream_t stream)
{
    const bool two_waves = use_128(a, class_taps, mode);
    const int waves = two_waves ? 2 : MCORR_WAVES;
    const size_t lds = a.aux != nullptr ? mcorr_lds_bytes_fused(max_code_len, a.window_floats, waves)
                                        : (a.window_floats > 0 ? mcorr_lds_bytes_window(a.window_floats, waves) : mcorr_lds_bytes(max_code_len, waves));
    GSH_REQUIRE(lds <= 160 * 1024, "local code of %d samples does not fit the 160 KiB LDS", max_code_len);
    const size_t lds_half = mcorr_lds_bytes_half(max_code_len, waves);
    if (two_waves) return mcorr_launch_epl_t128(a, lds, lds_half, stream);
    switch (class_taps)
        {
        case 1:
            return launch_nt<1>(a, mode, lds, lds_half, stream);
        case 3:
            return launch_nt<3>(a, mode, lds, lds_half, stream);
        case 5:
            return launch_nt<5>(a, mode, lds, lds_half, stream);
        default:
            return launch_nt<GSH_MAX_TAPS>(a, mode, lds, lds_half, stream);
        }
}

// the partials of every job summed into its output row: one launch, after every class of the batch has written its own
int reduce_if_split(const McorrArgs& a, hipStream_t stream)
{
    if (a.splits <= 1) return GSH_OK;
    const int total = a.n_jobs * GSH_MAX_TAPS;
    hipLaunchKernelGGL(mcorr_reduce_partials, dim3((total + 255) / 256), dim3(256), 0, stream, a.partials, a.out, a.n_jobs, a.splits);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace

int mcorr_packed_default()
{
    // GSH_MC_PACKED_BODY: 0 the round-1 body, 1 the packed trips, 2 the run-based path where a job qualifies, 3 the packed trips with the derived
    // early / late taps switched off (A/B switch, read once)
    static const int v = [] {
        const char* e = std::getenv("GSH_MC_PACKED_BODY");
        if (e != nullptr && e[0] == '0') return 0;
#ifdef GSH_MC_RUNS_EXPERIMENT
        if (e != nullptr && e[0] == '2') return 2;
#endif
        if (e != nullptr && e[0] == '3') return 3;  // packed trips without the derived early / late taps
        return 1;
    }();
    return v;
}

int mcorr_fac_default()
{
    static const int v = [] {
        const char* e = std::getenv("GSH_MC_FAC");
        return (e != nullptr && e[0] == '0') ? 0 : 1;
    }();
    return v;
}

size_t mcorr_lds_bytes_window(int window_floats, int waves)
{
    const size_t tab = (static_cast<size_t>(window_floats) + 3) & ~static_cast<size_t>(3);
    return tab * sizeof(float) + lds_tail_bytes(waves);
}

size_t mcorr_lds_bytes_fused(int max_code_len, int window_floats, int waves)
{
    const size_t one = window_floats > 0 ? static_cast<size_t>(window_floats) : static_cast<size_t>(max_code_len) + 2 * MCORR_MARGIN;
    const size_t tab = ((one + 3) & ~static_cast<size_t>(3)) + ((one + 3) & ~static_cast<size_t>(3));
    return tab * sizeof(float) + lds_tail_bytes(waves);
}

size_t mcorr_lds_bytes(int max_code_len, int waves)
{
    const size_t tab = (static_cast<size_t>(max_code_len) + 2 * MCORR_MARGIN + 3) & ~static_cast<size_t>(3);
    return tab * sizeof(float) + lds_tail_bytes(waves);
}

// the half-chip flavour: the doubled table in front of everything else; 0: the codes are too long for it
size_t mcorr_lds_bytes_half(int max_code_len, int waves)
{
    if (max_code_len > MCORR_HALF_MAX_CODE_LEN) return 0;
    static_assert(MC_HALF_MAX_CODE_LEN == MCORR_HALF_MAX_CODE_LEN, "the host's eligibility rule and the kernel's table size");
    return static_cast<size_t>(MCORR_HALF_WORDS) * sizeof(float) + mcorr_lds_bytes(max_code_len, waves);
}

int mcorr_launch(const McorrArgs& a, int max_taps, int mode, int max_code_len, hipStream_t stream)
{
    if (a.n_jobs <= 0) return GSH_OK;
    GSH_REQUIRE(max_taps >= 1 && max_taps <= GSH_MAX_TAPS, "n_taps %d outside 1..%d", max_taps, GSH_MAX_TAPS);
    GSH_REQUIRE(a.splits >= 1, "splits must be >= 1");
    const int rc = launch_class(a, tap_class(max_taps), mode, max_code_len, stream);
    return rc != GSH_OK ? rc : reduce_if_split(a, stream);
}

int mcorr_launch_classes(const McorrArgs& args, const McorrClassPlan& plan, int mode, int max_code_len, hipStream_t stream)
{
    if (args.n_jobs <= 0) return GSH_OK;
    GSH_REQUIRE(args.splits >= 1, "splits must be >= 1");
    static const int class_taps[4] = {1, 3, 5, GSH_MAX_TAPS};
    for (int c = 0; c < 4; c++)
        {
            if (plan.count[c] <= 0) continue;
            McorrArgs a = args;
            a.job_list = plan.list + plan.offset[c];
            a.n_launch = plan.count[c];
            if (!plan.aux[c]) a.aux = nullptr;
            // (a class that use_128 sends to the two-wave kernels is one launch among the others: its partials, if any, are summed with theirs below)
            const int rc = launch_class(a, class_taps[c], mode, max_code_len, stream);
            if (rc != GSH_OK) return rc;
        }
    return reduce_if_split(args, stream);
}
}  // namespace gsh
