// Internal C++ interface between the C-ABI layer (tracking_api.hip) and the wide correlator bank (multicorrelator_wide.hip):
// jobs of up to GSH_MAX_WIDE_TAPS taps, standard resampler and rotator.  Not part of the ABI.
#ifndef GSH_MULTICORRELATOR_WIDE_H
#define GSH_MULTICORRELATOR_WIDE_H

#include "gsh_internal.h"

namespace gsh
{
// Work-groups a wide job's window is cut into.  A function of the job's own length and of the explicit gsh_bank_set_splits value ALONE
// (user = 0: the rule below), never of the batch: the cut decides the order of a job's float32 sums, and a job's output bits must not
// depend on which other jobs share its launch.  A segment keeps at least 1 024 samples (two trips of a work-group).
constexpr int MCORR_WIDE_AUTO_SEGMENT = 32768;
__host__ __device__ inline int mcorr_wide_splits(int n_samples, int user)
{
    int s = user > 0 ? user : n_samples / MCORR_WIDE_AUTO_SEGMENT;
    const int by_len = n_samples / 1024;
    if (s > by_len) s = by_len;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

struct McorrWideArgs
{
    const float2* stream;            // device, complex64 IF samples
    const gsh_corr_job_wide* jobs;   // device, n_jobs entries; sample_offset is a position in `stream` (sample base and ring position already applied)
    const float* codes;              // device, n_slots * code_stride floats
    const int* code_lens;            // device, n_slots
    int code_stride;
    float2* out;                     // device, n_jobs * GSH_MAX_WIDE_TAPS
    float2* partials;                // device, n_jobs * max_splits * GSH_MAX_WIDE_TAPS (max_splits > 1 only)
    int n_jobs;
    int splits_user;                 // gsh_bank_set_splits (0: per job, mcorr_wide_splits)
    int max_splits;                  // largest mcorr_wide_splits of the batch: the grid's extent; a job's work-groups beyond its own count end at once
    int table_floats;                // code-table entries of the LDS (mcorr_wide_table_floats)
    int max_taps;                    // largest n_taps of the batch
    // filled in by mcorr_wide_launch:
    int tap_block;                   // taps per work-group: 4, 8 or 16 (changes no sum: a tap's products and their order are those of its lane and wave)
    int n_blocks;                    // tap blocks launched per job: ceil(max_taps / tap_block)
};

// most code-table entries a work-group can stage; a tap block whose chip indices span more takes the whole code and wraps every index
int mcorr_wide_table_cap();
// taps a work-group may take at most (the tap block follows the launch: the host sizes the table for the largest)
constexpr int MCORR_WIDE_MAX_BLOCK = 16;
size_t mcorr_wide_lds_bytes(int table_floats);
int mcorr_wide_launch(const McorrWideArgs& args, hipStream_t stream);
}  // namespace gsh

#endif
