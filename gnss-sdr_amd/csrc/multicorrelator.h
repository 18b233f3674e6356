// Internal C++ interface between the C-ABI layer (gsh_api.hip) and the correlator kernels
// (multicorrelator.hip).  Not part of the ABI.
#ifndef GSH_MULTICORRELATOR_H
#define GSH_MULTICORRELATOR_H

#include "gsh_internal.h"

namespace gsh
{
// a job whose early tap may be read next to its late tap (mcorr_device.h packed_trip): E/P/L, prompt at exactly 0, late - early exactly 1 chip,
// standard mode, the code running forward
__host__ __device__ inline bool mcorr_pair_eligible(int n_taps, const float* shifts, float code_step, int mode)
{
    return n_taps == 3 && mode == 0 && shifts[1] == 0.0f && (static_cast<double>(shifts[2]) - static_cast<double>(shifts[0]) == 1.0) && code_step > 0.0f;
}

// a pair-eligible job whose three taps may all be taken from the prompt tap's index chain (mcorr_device.h packed_trip, half-chip taps): early and late exactly half a
// chip either side of the prompt, and a code short enough that every index of its doubled table, floor(2 w), is a half-precision bit pattern (below 2048)
constexpr int MCORR_HALF_MAX_CODE_LEN = 1024;
__host__ __device__ inline bool mcorr_half_chip_eligible(int n_taps, const float* shifts, float code_step, int mode, int code_len)
{
    return mcorr_pair_eligible(n_taps, shifts, code_step, mode) && shifts[0] == -0.5f && shifts[2] == 0.5f && code_len <= MCORR_HALF_MAX_CODE_LEN;
}

// The LDS image of a code as the half-chip flavour stages it (mcorr_device.h packed_trip), built once per gsh_bank_set_code and copied by every work-group:
// the doubled guard-banded table D[2 i] = D[2 i + 1] = table[i] at word 0 (sized for the longest code the flavour takes), the plain guard-banded table
// table[i] = code[(i - MARGIN) mod len], i in [0, len + 2 MARGIN), at word MCORR_HALF_WORDS; what lies behind either table is zero.
constexpr int MCORR_MARGIN = 32;                                                                  // guard entries on each side of a code table
constexpr int MCORR_HALF_WORDS = 2 * (MCORR_HALF_MAX_CODE_LEN + 2 * MCORR_MARGIN);                // the doubled table's room
constexpr int MCORR_HALF_IMAGE_WORDS = MCORR_HALF_WORDS + MCORR_HALF_MAX_CODE_LEN + 2 * MCORR_MARGIN;  // 3 264 words, a whole number of 16-byte rows
static_assert(MCORR_HALF_WORDS % 4 == 0 && MCORR_HALF_IMAGE_WORDS % 4 == 0, "the image is copied in 16-byte rows");
constexpr int MCORR_FAC_ENTRIES = 64;  // float2 entries of a work-group's carrier-seed factor table, behind its wave sums in the LDS (mcorr_device.h fac_table_fill)
inline void mcorr_build_half_image(const float* code, int code_len, float* image)
{
    for (int i = 0; i < MCORR_HALF_IMAGE_WORDS; i++) image[i] = 0.0f;
    for (int i = 0; i < code_len + 2 * MCORR_MARGIN; i++)
        {
            const int k = ((i - MCORR_MARGIN) % code_len + code_len) % code_len;
            image[2 * i] = image[2 * i + 1] = image[MCORR_HALF_WORDS + i] = code[k];
        }
}

struct McorrArgs
{
    const float2* stream;            // device, complex64 IF samples
    unsigned long long stream_len;   // samples
    const gsh_corr_job* jobs;        // device, n_jobs entries
    const float* codes;              // device, n_slots * code_stride floats
    const int* code_lens;            // device, n_slots
    int code_stride;
    const float* code_images;        // device, n_slots * MCORR_HALF_IMAGE_WORDS floats (mcorr_build_half_image), or nullptr: no launch of this bank takes the half-chip flavour
    float2* out;                     // device, n_jobs * GSH_MAX_TAPS
    float2* partials;                // device, n_jobs * splits * GSH_MAX_TAPS (splits > 1 only)
    int n_jobs;
    int splits;
    int window_floats;               // > 0: LDS holds only a window of the code per work-group (all jobs: mode 0, code_step >= 0); 0: the whole code
    const int* job_list;             // device, n_launch job indices this launch works on (order kept), or nullptr: jobs 0..n_launch-1
    int n_launch;                    // jobs in this launch (n_jobs stays the size of the whole table: outputs / partials are indexed by job)
    unsigned long long sample_base;  // added to every job's sample_offset at launch (gsh_bank_set_sample_base): the same resident job table serves block after block
    unsigned long long ring_capacity;// > 0: the stream is a gsh_stream ring, positions are taken modulo its capacity (windows stay contiguous: mirror)
    int packed;                      // 1: the packed four-samples-per-lane body may be used (default); 0: the round-1 body (A/B runs)
    int fac;                         // 1: the carrier seeds come from the work-group's factor table (default); 0: two evaluations per lane (A/B runs, GSH_MC_FAC=0)
    int pair;                        // 1: every job with two or three taps in this batch is an E/P/L set with a zero-shift prompt, early and late exactly one chip
                                     // apart and the code running forward (the host checked): the 3-tap launch reads early next to late (mcorr_device.h)
    int half;                        // 1: and every one of them is mcorr_half_chip_eligible: the whole-code 3-tap launch takes its three taps from one index chain
    const int* aux;                  // device, n_jobs, or nullptr.  aux[j] >= 0: job j also computes the single tap of job aux[j] (same window and
                                     // NCO, another code) and writes its output row; -2: job j is computed by its leader; -1: plain job
};

// Largest n_taps over the jobs and which mode combinations occur decide the template
// instance; all jobs of one launch must share `mode` (gsh_corr_job::high_dyn).
// 1 unless the environment says GSH_MC_PACKED_BODY=0 (read once; A/B switch for profiles/ab/mcorr_ab.py)
int mcorr_packed_default();
// 1 unless the environment says GSH_MC_FAC=0 (read once; A/B switch)
int mcorr_fac_default();

int mcorr_launch(const McorrArgs& args, int max_taps, int mode, int max_code_len, hipStream_t stream);

// A batch whose jobs differ in tap count is launched per kernel flavour (1, <= 3, <= 5, <= 8 taps) so that a 3-tap job does not pay for
// five: `list` holds the job indices grouped by class (device), offset / count per class, aux[c] whether class c contains fused leaders.
struct McorrClassPlan
{
    const int* list;
    int offset[4];
    int count[4];
    bool aux[4];
};
int mcorr_launch_classes(const McorrArgs& args, const McorrClassPlan& plan, int mode, int max_code_len, hipStream_t stream);
// The two-wave kernels' only entry (csrc/multicorrelator_t128.hip): one E/P/L launch in the standard mode with whole-code tables and no fused jobs, i.e. what
// use_128() of csrc/multicorrelator.hip admits -- mcorr_launch / mcorr_launch_classes choose, callers do not.  lds / lds_half: mcorr_lds_bytes /
// mcorr_lds_bytes_half of the launch's longest code at two waves.  It launches the kernel and nothing else: the partials are summed by its caller.
int mcorr_launch_epl_t128(const McorrArgs& args, size_t lds, size_t lds_half, hipStream_t stream);

// dynamic LDS bytes a work-group of `waves` waves needs for a code of max_code_len samples (every caller but the launcher means the four-wave kernels)
constexpr int MCORR_WAVES = 4;
size_t mcorr_lds_bytes(int max_code_len, int waves = MCORR_WAVES);
// the same for the half-chip flavour of the E/P/L kernels (a doubled table in front); 0: the code is too long for that flavour
size_t mcorr_lds_bytes_half(int max_code_len, int waves = MCORR_WAVES);
// the same when only `window_floats` code samples are staged per work-group
size_t mcorr_lds_bytes_window(int window_floats, int waves = MCORR_WAVES);
// LDS bytes with room for the fused correlator's second code table (aux != nullptr)
size_t mcorr_lds_bytes_fused(int max_code_len, int window_floats, int waves = MCORR_WAVES);
}  // namespace gsh

#endif
