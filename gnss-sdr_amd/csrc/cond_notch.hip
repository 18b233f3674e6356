// The notch stage of the signal conditioner (gsh_cond_set_notch, include/gnss_sdr_hip.h): notch_cc / notch_lite_cc
// (src/algorithms/input_filter/gnuradio_blocks/notch_cc.cc:72-118, notch_lite_cc.cc:81-136) between the conditioner's filter and its resampler, on the
// push's stream.  The arithmetic is notch_filter.h, the text gsh_notch_process_device runs.
//
// Indices.  y is the filter-output stream, w[k] the mitigated y[k + 1] with y[k] in front of it.  Segments tile w from w[0] on, and so do the chunks
// of NF_CHUNK outputs the recurrence is chained over: both are absolute, so which composite a sample belongs to, and with it every bit of the
// output, does not depend on where the stream is cut into pushes.  The stage buffer x holds y from `origin` on (CondNotchArgs, conditioner.h):
// origin is a multiple of the length, so sample_map's n / length and n - s * length mean the same relative to it.
//
// Launches of a push: load (the carried filter outputs, modes and coefficients in front of the new ones), the chain's own launch for the new
// filter outputs (conditioner.hip), then for the segments the push completes: energy and floor, the one-thread decision, one composite per chunk
// from the open chunk on, the one-thread carry chain, the replay that writes the new outputs; save (what the next push needs), and the gather
// w[m(j)] into the ring with the resampler's integer m(j).  Every loop is bounded by a count the host computed; nothing is read back.
//
// The floor values (a length-point DFT per segment) are formed when the state at the start of the push says an estimating segment can be reached:
// nf_needs_floor, the condition gsh_notch_process_device evaluates on its shadow state.  It is exact, not a guess: from a counter at or above
// n_segments_est that cannot pass n_segments_reset within the push, the counter only grows, and an estimating segment needs it below n_segments_est.
#include "conditioner.h"

namespace gsh
{
namespace
{
constexpr int CN_THREADS = 256;

__global__ __launch_bounds__(CN_THREADS) void cond_notch_load_kernel(CondNotchArgs n, int lite)
{
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x;
    if (i < n.n_y_in) n.x[n.y0 - n.origin + i] = n.y_in[i];
    const unsigned long long n_modes = n.S0 - n.seg_base;
    if (i < n_modes)
        {
            n.mode[i] = n.mode_in[i];
            if (lite) n.z0_seg[i] = n.z0_in[i];
        }
}

__global__ __launch_bounds__(CN_THREADS) void cond_notch_save_kernel(CondNotchArgs n, int lite)
{
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x;
    if (i < n.n_y_out) n.y_out[i] = n.x[n.y1 - n.origin + i];
    const unsigned long long n_modes = n.S0 + n.n_seg - n.seg_base1;
    if (i < n_modes)
        {
            const unsigned long long s = n.seg_base1 - n.seg_base + i;
            n.mode_out[i] = n.mode[s];
            if (lite) n.z0_out[i] = n.z0_seg[s];
        }
}

// notch_segment_kernel over the stage buffer; the energy's rotation keyed to the segment's absolute index
__global__ __launch_bounds__(NF_THREADS) void cond_notch_segment_kernel(CondNotchArgs n, int seg_per_wg)
{
    extern __shared__ float lds[];
    const unsigned long long seg0 = static_cast<unsigned long long>(blockIdx.x) * seg_per_wg;
    const int segs = static_cast<int>(min(static_cast<unsigned long long>(seg_per_wg), n.n_seg - seg0));
    const int with_floor = nf_needs_floor(n.state_in->s.n_segments, n.n_seg, n.n_segments_est, n.n_segments_reset) ? 1 : 0;
    nf_segment_workgroup(lds, n.x + (n.W0 - n.origin), n.length, seg0, segs, n.energy, n.floor_lin, with_floor, seg_per_wg,
        static_cast<int>((n.S0 + seg0) % static_cast<unsigned long long>(seg_per_wg)));
}

// notch_decide_kernel with the state handed from push to push and the two counters
__global__ void cond_notch_decide_kernel(CondNotchArgs n)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    CondNotchState st = *n.state_in;
    const int have_floor = nf_needs_floor(st.s.n_segments, n.n_seg, n.n_segments_est, n.n_segments_reset) ? 1 : 0;  // as the segment kernel: see the head of the file
    const unsigned long long first = n.S0 - n.seg_base;
    (void)nf_decide_segments(n.x + (n.W0 - n.origin), n.energy, n.floor_lin, have_floor, n.n_seg, n.length, n.mode + first, n.z0_seg + first, st.s, n.n_segments_est,
        n.n_segments_reset, n.n_segments_coeff, n.thres, &st.n_filtered);
    st.n_decided += n.n_seg;
    *n.state_out = st;
}

// one thread per chunk c0 + t: the composite of its samples up to W1 (notch_compose_kernel)
__global__ __launch_bounds__(CN_THREADS) void cond_notch_compose_kernel(CondNotchArgs n, int lite)
{
    const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x;
    if (t >= n.n_chunks) return;
    const unsigned long long k0 = (n.c0 + t) * NF_CHUNK;
    const unsigned long long k1 = min(n.W1, k0 + NF_CHUNK);
    float2 B = make_float2(1.0f, 0.0f), A = make_float2(0.0f, 0.0f);
    for (unsigned long long k = k0; k < k1; k++)
        {
            float2 a, b;
            sample_map(n.x, k - n.origin, n.length, n.mode, n.z0_seg, lite != 0, n.p_c_factor, a, b);
            A = cadd(a, cmul_ref(b, A));
            B = cmul_ref(b, B);
        }
    n.comp[2 * t] = B;
    n.comp[2 * t + 1] = A;
}

// carries: comp[2 t] = value of the recurrence just before chunk c0 + t (notch_carry_kernel); the chain runs over the whole chunks only, and what
// it arrives at -- the carry of the chunk the next push opens with -- goes into the state
__global__ void cond_notch_carry_kernel(CondNotchArgs n)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float2 carry = n.state_out->carry;  // (the decision copied it from state_in)
    for (unsigned long long t = 0; t < n.n_chunks; t++)
        {
            const float2 B = n.comp[2 * t], A = n.comp[2 * t + 1];
            n.comp[2 * t] = carry;
            if (t < n.n_full) carry = cadd(A, cmul_ref(B, carry));
        }
    n.state_out->carry = carry;
}

// one thread per chunk: replay from the carry (notch_apply_kernel), writing the outputs the push adds: those from W0 on
__global__ __launch_bounds__(CN_THREADS) void cond_notch_replay_kernel(CondNotchArgs n, int lite)
{
    const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x;
    if (t >= n.n_chunks) return;
    const unsigned long long k0 = (n.c0 + t) * NF_CHUNK;
    const unsigned long long k1 = min(n.W1, k0 + NF_CHUNK);
    float2 out = n.comp[2 * t];
    for (unsigned long long k = k0; k < k1; k++)
        {
            float2 a, b;
            sample_map(n.x, k - n.origin, n.length, n.mode, n.z0_seg, lite != 0, n.p_c_factor, a, b);
            const bool filt = (n.mode[(k - n.origin) / n.length] & 0x7f) == 1;
            if (filt) out = cadd(a, cmul_ref(b, out));
            if (k >= n.W0) n.w[k - n.W0] = filt ? out : a;
        }
}

// one thread per ring sample, the source picked by the resampler's index
__global__ __launch_bounds__(CN_THREADS) void cond_notch_gather_kernel(CondArgs a, const float2* __restrict__ w, unsigned long long W0)
{
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * CN_THREADS;
    for (unsigned long long d = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x; d < a.n_out; d += stride)
        a.out[d] = w[cond_filter_index(a, d) - W0];
}

// no resampler: ring sample d is w[a.out0 + d - W0]; two per thread in one 16-byte store from a.out + head on (head 0 or 1 makes that address a
// multiple of 16), the head and an odd last sample by two threads of the first work-group
__global__ __launch_bounds__(CN_THREADS) void cond_notch_gather_pairs_kernel(CondArgs a, const float2* __restrict__ w, unsigned long long W0, unsigned head)
{
    const unsigned long long n_pairs = (a.n_out - head) >> 1;
    const float2* __restrict__ src = w + (a.out0 - W0);
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * CN_THREADS;
    for (unsigned long long p = static_cast<unsigned long long>(blockIdx.x) * CN_THREADS + threadIdx.x; p < n_pairs; p += stride)
        {
            const unsigned long long d = head + 2 * p;
            const float2 v0 = src[d], v1 = src[d + 1];
            *reinterpret_cast<float4*>(a.out + d) = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    if (blockIdx.x == 0)
        {
            if (threadIdx.x == 0 && head != 0u) a.out[0] = src[0];
            const unsigned long long last = head + 2 * n_pairs;
            if (threadIdx.x == 1 && last < a.n_out) a.out[last] = src[last];
        }
}

unsigned blocks_for(unsigned long long items)
{
    const unsigned long long blocks = (items + CN_THREADS - 1) / CN_THREADS;
    return static_cast<unsigned>(blocks == 0 ? 1 : blocks);
}
}  // namespace

int cond_notch_launch_load(const CondNotchArgs& n, hipStream_t st)
{
    const unsigned long long items = n.n_y_in > n.S0 - n.seg_base ? n.n_y_in : n.S0 - n.seg_base;
    if (items == 0) return GSH_OK;
    cond_notch_load_kernel<<<dim3(blocks_for(items)), dim3(CN_THREADS), 0, st>>>(n, n.n_segments_coeff > 0 ? 1 : 0);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

int cond_notch_launch_save(const CondNotchArgs& n, hipStream_t st)
{
    const unsigned long long modes = n.S0 + n.n_seg - n.seg_base1;
    const unsigned long long items = n.n_y_out > modes ? n.n_y_out : modes;
    if (items == 0) return GSH_OK;
    cond_notch_save_kernel<<<dim3(blocks_for(items)), dim3(CN_THREADS), 0, st>>>(n, n.n_segments_coeff > 0 ? 1 : 0);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

int cond_notch_launch_filter(const CondNotchArgs& n, hipStream_t st)
{
    const int lite = n.n_segments_coeff > 0 ? 1 : 0;
    const int seg_per_wg = nf_seg_per_wg(n.length);
    const unsigned long long blocks_s = (n.n_seg + seg_per_wg - 1) / seg_per_wg;
    cond_notch_segment_kernel<<<dim3(static_cast<unsigned>(blocks_s)), dim3(NF_THREADS), nf_segment_lds(n.length), st>>>(n, seg_per_wg);
    GSH_HIP(hipGetLastError());
    cond_notch_decide_kernel<<<dim3(1), dim3(64), 0, st>>>(n);
    GSH_HIP(hipGetLastError());
    cond_notch_compose_kernel<<<dim3(blocks_for(n.n_chunks)), dim3(CN_THREADS), 0, st>>>(n, lite);
    GSH_HIP(hipGetLastError());
    cond_notch_carry_kernel<<<dim3(1), dim3(64), 0, st>>>(n);
    GSH_HIP(hipGetLastError());
    cond_notch_replay_kernel<<<dim3(blocks_for(n.n_chunks)), dim3(CN_THREADS), 0, st>>>(n, lite);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

int cond_notch_launch_gather(const CondArgs& a, const CondNotchArgs& n, hipStream_t st)
{
    if (a.rs_mode == COND_RS_NONE)
        {
            const unsigned head = static_cast<unsigned>((reinterpret_cast<uintptr_t>(a.out) >> 3) & 1u);
            unsigned long long blocks = ((a.n_out >> 1) + CN_THREADS) / CN_THREADS;
            if (blocks > 4096ull) blocks = 4096ull;
            cond_notch_gather_pairs_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(CN_THREADS), 0, st>>>(a, n.w, n.W0, head);
            GSH_HIP(hipGetLastError());
            return GSH_OK;
        }
    unsigned long long blocks = (a.n_out + CN_THREADS - 1) / CN_THREADS;
    if (blocks > 4096ull) blocks = 4096ull;
    cond_notch_gather_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(CN_THREADS), 0, st>>>(a, n.w, n.W0);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace gsh
