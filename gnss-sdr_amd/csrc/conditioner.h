// The signal conditioner's one-pass kernels (gsh_cond_*, include/gnss_sdr_hip.h): adapter, FIR and resampler per ring sample.  The kernels live in
// fir_filter.hip, beside fir_kernel, because they call its device functions (fetch_translated: the loose chain's arithmetic by construction); the
// handle, its bookkeeping and the C ABI are conditioner.hip.
#ifndef GSH_CONDITIONER_H
#define GSH_CONDITIONER_H
#include "gsh_internal.h"
#include "notch_filter.h"
#include "packed_unpack.h"

namespace gsh
{
// what the block's items are (CondArgs::kind): 0 .. 4 are the input kinds of the FIR handle (fir_filter.hip), 5 and 6 the ring's integer item types
enum
{
    COND_CPX_FLOAT = 0,
    COND_REAL_FLOAT = 1,
    COND_REAL_SHORT = 2,
    COND_REAL_BYTE = 3,
    COND_PACKED = 4,
    COND_CPX_SHORT = 5,
    COND_CPX_BYTE = 6
};
enum
{
    COND_RS_NONE = 0,
    COND_RS_DECIMATE = 1,
    COND_RS_INTERPOLATE = 2
};
constexpr int COND_TILE = 1024;      // ring samples per work-group at most
constexpr int COND_MAX_SPAN = 4096;  // staged inputs per work-group: 32 KiB of LDS as float2, four work-groups and more per compute unit

// One launch: ring samples [out0, out0 + n_out) of the conditioner's output stream into `out`.  Passed by value.
struct CondArgs
{
    const void* in;              // the raw block: n_in samples of `kind`, sample 0 at its first byte
    const float2* hist;          // the n_taps - 1 samples before the block, converted (and conjugated), untranslated
    float2* hist_out;            // cond_launch_history: receives the new tail
    const float* taps;
    float2* out;
    unsigned long long in0;      // absolute index of the block's first sample
    unsigned long long n_in;
    unsigned long long out0;     // absolute output index of out[0]
    unsigned long long n_out;    // below 2^32
    unsigned long long q0, r0;   // the resampler's plan for out0: ResampleArgs of resampler.hip (cond_plan_resampler fills them)
    double rev_per_sample;       // f_c / f_s
    unsigned step;
    int rs_mode;                 // COND_RS_*
    int n_taps;                  // 0: no filter (the sample itself; `hist`, `taps` unused)
    int decimation;
    int kind;
    int conj;                    // inverted_spectrum: conjugate the decoded sample, before the filter
    int tile, max_span;          // cond_tile(): ring samples per work-group and the inputs they span at most
    PackedCode packed;           // kind COND_PACKED
};

// filter output that feeds output d of the launch: resample_gather_kernel's index (resampler.hip), d below 2^32
__device__ __forceinline__ unsigned long long cond_filter_index(const CondArgs& a, unsigned long long d)
{
    if (a.rs_mode == COND_RS_DECIMATE) return a.q0 + (a.r0 + (d << 32)) / a.step;
    if (a.rs_mode == COND_RS_INTERPOLATE) return a.q0 + ((a.r0 + d * a.step) >> 32);
    return a.out0 + d;
}

// ---- the blanking stage (cond_blanking.hip): pulse_blanking_cc between the filter and the resampler.  A push forms its new filter outputs behind
// the carry of the open segment in a stage buffer (cond_launch without a resampler), then: one energy per completed segment, the decision over
// them, and the masked gather into the ring.
struct CondBlankState          // device memory, carried from push to push
{
    float noise_power_estimation;
    int n_segments;
    int last_filtered;
    int reserved;
    unsigned long long n_decided, n_blanked;  // segments decided since the handle was created, and those of them that were blanked
};
struct CondBlankArgs
{
    const float2* stage;       // filter outputs base, base + 1, ...: the carry, then the push's new ones
    float* energy;             // n_seg
    unsigned char* mask;       // n_seg
    const CondBlankState* state_in;
    CondBlankState* state_out; // (gsh_cond_time_push: a copy)
    unsigned long long base;   // absolute filter-output index of stage[0]: a multiple of length
    unsigned long long n_seg;  // segments this push completes: stage[0 .. n_seg * length)
    int length, n_segments_est, n_segments_reset;
    float thres;
};
// queue the energies and the decision of b.n_seg > 0 segments
int cond_blank_launch_decide(const CondBlankArgs& b, hipStream_t st);
// queue the gather: ring samples [a.out0, a.out0 + a.n_out) into a.out, each mask ? 0 : stage[m(j) - base] (a: q0, r0 planned; every m(j) within
// the decided segments)
int cond_blank_launch_gather(const CondArgs& a, const CondBlankArgs& b, hipStream_t st);

// ---- the notch stage (cond_notch.hip): notch_cc / notch_lite_cc between the filter and the resampler.  Notch output w[k] is the mitigated filter
// output y[k + 1] with y[k] in front of it; w is cut into segments of `length` from w[0] on and into chunks of NF_CHUNK from w[0] on.  A push forms
// its new filter outputs behind the carried ones (y from the start of the open chunk on) in a stage buffer x, whose item 0 is filter output
// `origin`: the first sample of the segment the open chunk starts in, so that index k - origin of x, mode and z0_seg addresses w[k] the way
// sample_map (notch_filter.h) addresses a call's sample.  Then: energy and floor of the segments the push completes, their decision, the
// composites of the chunks from the open one on, the carry chain, the replay that writes the push's new outputs, and the gather into the ring.
struct CondNotchState          // device memory, carried from push to push
{
    NotchState s;              // (last_out and Notch's per-sample z0 are not kept: they depend on where a call ends)
    unsigned long long n_decided, n_filtered;  // segments decided since the handle was created, and those of them that went through the recurrence
    float2 carry;              // the recurrence's value in front of the open chunk: a chain of chunk composites, never a replayed output
};
struct CondNotchArgs
{
    float2* x;                 // filter outputs origin, origin + 1, ...; those below y0 are never formed nor read
    float* energy;             // n_seg
    float* floor_lin;          // n_seg
    unsigned char* mode;       // per segment from seg_base on: the carried ones, then the n_seg new ones
    float2* z0_seg;            // (NotchLite) likewise
    float2* comp;              // per chunk from c0 on: (B, A) composites, then the carries
    float2* w;                 // notch outputs W0 .. W1
    const float2* y_in;        // carried filter outputs y0 .. y0 + n_y_in, modes and coefficients of segments seg_base .. S0
    const unsigned char* mode_in;
    const float2* z0_in;
    float2* y_out;             // what the push leaves: filter outputs y1 .. y1 + n_y_out, modes and coefficients of segments seg_base1 .. S0 + n_seg
    unsigned char* mode_out;
    float2* z0_out;
    const CondNotchState* state_in;
    CondNotchState* state_out; // (gsh_cond_time_push: a copy)
    unsigned long long origin, seg_base;  // origin = seg_base * length
    unsigned long long y0, n_y_in;        // y0 = c0 * NF_CHUNK
    unsigned long long y1, n_y_out, seg_base1;
    unsigned long long S0, n_seg;         // first segment the push completes, and how many
    unsigned long long W0, W1;            // = S0 * length, (S0 + n_seg) * length
    unsigned long long c0, n_chunks;      // chunks c0 .. c0 + n_chunks cover [y0, W1); the first n_full of them are whole
    unsigned long long n_full;
    int length, n_segments_est, n_segments_reset, n_segments_coeff;
    float thres, p_c_factor;
};
// queue the copy of the carried filter outputs, modes and coefficients into x, mode, z0_seg (before the push's filter outputs are formed behind them)
int cond_notch_launch_load(const CondNotchArgs& n, hipStream_t st);
// queue segment kernel, decision, compose, carry and replay of n.n_seg > 0 segments
int cond_notch_launch_filter(const CondNotchArgs& n, hipStream_t st);
// queue the copy of what the next push needs into y_out, mode_out, z0_out
int cond_notch_launch_save(const CondNotchArgs& n, hipStream_t st);
// queue the gather: ring samples [a.out0, a.out0 + a.n_out) into a.out, each w[m(j) - W0] (a: q0, r0 planned; every m(j) within [W0, W1))
int cond_notch_launch_gather(const CondArgs& a, const CondNotchArgs& n, hipStream_t st);

// q0, r0 of a launch whose first output is a.out0 (a.step, a.rs_mode set)
void cond_plan_resampler(CondArgs* a);
// a.tile, a.max_span for the handle's filter and ratio: the largest power of two of outputs whose inputs fit COND_MAX_SPAN
void cond_tile(CondArgs* a);
// queue the launch on st (a.n_out > 0)
int cond_launch(const CondArgs& a, hipStream_t st);
// queue the history update: a.hist_out = the last n_taps - 1 converted samples of (a.hist, the block)
int cond_launch_history(const CondArgs& a, hipStream_t st);
}  // namespace gsh
#endif
