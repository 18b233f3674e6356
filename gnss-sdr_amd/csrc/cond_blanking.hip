// The blanking stage of the signal conditioner (gsh_cond_set_blanking, include/gnss_sdr_hip.h): pulse_blanking_cc
// (src/algorithms/input_filter/gnuradio_blocks/pulse_blanking_cc.cc:57-106) between the conditioner's filter and its resampler, on the push's stream.
//
// The filter outputs of a push lie in the handle's stage buffer behind the carry of the open segment, so stage[0] is the first sample of a segment
// (absolute filter output `base`, a multiple of length).  Three launches: one energy per completed segment (pb_segment_energy, the rotation keyed
// to the segment's absolute index, so the bits are those of pb_energy_kernel over the whole stream), the one-thread decision (pb_decide_segments) that
// leaves mask, state and counters in device memory, and the gather that writes ring sample j = mask ? 0 : stage[m(j) - base] with the resampler's
// integer m(j).  Every loop is bounded by a count the host computed; nothing is read back.
#include "conditioner.h"
#include "pulse_blanking.h"

namespace gsh
{
namespace
{
constexpr int CB_THREADS = 256;

// pb_energy_kernel over the stage buffer: a work-group stages |y|^2 of seg_per_wg segments in LDS, every thread then sums whole segments
__global__ __launch_bounds__(PB_THREADS) void cond_blank_energy_kernel(CondBlankArgs b, int seg_per_wg)
{
    extern __shared__ float tile[];
    const unsigned long long seg0 = static_cast<unsigned long long>(blockIdx.x) * seg_per_wg;
    const unsigned long long segs = min(static_cast<unsigned long long>(seg_per_wg), b.n_seg - seg0);
    const unsigned long long first = seg0 * b.length;
    const unsigned long long count = segs * b.length;
    for (unsigned long long i = threadIdx.x; i < count; i += PB_THREADS) tile[i] = pb_mag2(b.stage[first + i]);
    __syncthreads();
    const unsigned long long abs0 = b.base / b.length + seg0;  // absolute index of the work-group's first segment
    for (unsigned long long s = threadIdx.x; s < segs; s += PB_THREADS)
        b.energy[seg0 + s] = pb_segment_energy(tile + s * b.length, b.length, static_cast<int>((abs0 + s) % seg_per_wg));
}

// pb_decide_kernel with the state handed from push to push and the two counters
__global__ void cond_blank_decide_kernel(CondBlankArgs b)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float noise = b.state_in->noise_power_estimation;
    int n_segments = b.state_in->n_segments;
    bool last_filtered = b.state_in->last_filtered != 0;
    const unsigned long long decided = b.state_in->n_decided;
    unsigned long long blanked = b.state_in->n_blanked;
    const float n_deg = static_cast<float>(2 * b.length);  // n_deg_fred, :43
    pb_decide_segments(b.energy, b.n_seg, b.mask, noise, n_segments, last_filtered, n_deg, b.n_segments_est, b.n_segments_reset, b.thres, &blanked);
    b.state_out->noise_power_estimation = noise;
    b.state_out->n_segments = n_segments;
    b.state_out->last_filtered = last_filtered ? 1 : 0;
    b.state_out->reserved = 0;
    b.state_out->n_decided = decided + b.n_seg;
    b.state_out->n_blanked = blanked;
}

// mitigated filter output with stage index i (below 2^32: the host bounds the stage buffer)
__device__ __forceinline__ float2 cond_blank_sample(const CondBlankArgs& b, unsigned i)
{
    return b.mask[i / static_cast<unsigned>(b.length)] ? make_float2(0.0f, 0.0f) : b.stage[i];
}

// one thread per ring sample (pb_apply_kernel's 8-byte pattern), the source picked by the resampler's index
__global__ __launch_bounds__(CB_THREADS) void cond_blank_gather_kernel(CondArgs a, CondBlankArgs b)
{
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * CB_THREADS;
    for (unsigned long long d = static_cast<unsigned long long>(blockIdx.x) * CB_THREADS + threadIdx.x; d < a.n_out; d += stride)
        a.out[d] = cond_blank_sample(b, static_cast<unsigned>(cond_filter_index(a, d) - b.base));
}

// no resampler: ring sample d is stage[a.out0 + d - base]; two per thread in one 16-byte store from a.out + head on (head 0 or 1 makes that address a
// multiple of 16), the head and an odd last sample by two threads of the first work-group
__global__ __launch_bounds__(CB_THREADS) void cond_blank_gather_pairs_kernel(CondArgs a, CondBlankArgs b, unsigned head)
{
    const unsigned long long n_pairs = (a.n_out - head) >> 1;
    const unsigned off = static_cast<unsigned>(a.out0 - b.base);
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * CB_THREADS;
    for (unsigned long long p = static_cast<unsigned long long>(blockIdx.x) * CB_THREADS + threadIdx.x; p < n_pairs; p += stride)
        {
            const unsigned long long d = head + 2 * p;
            const float2 v0 = cond_blank_sample(b, off + static_cast<unsigned>(d));
            const float2 v1 = cond_blank_sample(b, off + static_cast<unsigned>(d) + 1u);
            *reinterpret_cast<float4*>(a.out + d) = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    if (blockIdx.x == 0)
        {
            if (threadIdx.x == 0 && head != 0u) a.out[0] = cond_blank_sample(b, off);
            const unsigned long long last = head + 2 * n_pairs;
            if (threadIdx.x == 1 && last < a.n_out) a.out[last] = cond_blank_sample(b, off + static_cast<unsigned>(last));
        }
}
}  // namespace

int cond_blank_launch_decide(const CondBlankArgs& b, hipStream_t st)
{
    const int seg_per_wg = pb_seg_per_wg(b.length);
    const unsigned long long blocks = (b.n_seg + seg_per_wg - 1) / seg_per_wg;
    cond_blank_energy_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(PB_THREADS), sizeof(float) * static_cast<size_t>(seg_per_wg) * b.length, st>>>(b, seg_per_wg);
    GSH_HIP(hipGetLastError());
    cond_blank_decide_kernel<<<dim3(1), dim3(64), 0, st>>>(b);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

int cond_blank_launch_gather(const CondArgs& a, const CondBlankArgs& b, hipStream_t st)
{
    if (a.rs_mode == COND_RS_NONE)
        {
            const unsigned head = static_cast<unsigned>((reinterpret_cast<uintptr_t>(a.out) >> 3) & 1u);
            unsigned long long blocks = ((a.n_out >> 1) + CB_THREADS) / CB_THREADS;
            if (blocks > 4096ull) blocks = 4096ull;
            cond_blank_gather_pairs_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(CB_THREADS), 0, st>>>(a, b, head);
            GSH_HIP(hipGetLastError());
            return GSH_OK;
        }
    unsigned long long blocks = (a.n_out + CB_THREADS - 1) / CB_THREADS;
    if (blocks > 4096ull) blocks = 4096ull;
    cond_blank_gather_kernel<<<dim3(static_cast<unsigned>(blocks)), dim3(CB_THREADS), 0, st>>>(a, b);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace gsh
