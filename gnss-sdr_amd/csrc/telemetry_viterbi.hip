// Galileo telemetry pages on the device: the page decoder of galileo_telemetry_decoder_gs (deinterleaver, K = 7 rate 1/2 Viterbi decoder, CRC-24Q;
// src/algorithms/telemetry_decoder/gnuradio_blocks/galileo_telemetry_decoder_gs.cc:352-560, libs/viterbi_decoder.cc) and the clipped preamble correlation
// of its frame synchroniser (:962-972).  The arithmetic is viterbi_acs.h, shared with the host.
//
// tlm_pages_kernel: one wave64 per channel that has jobs, one lane per trellis state.  The wave walks its channel's jobs in table order (the reference-mode
// metric carry-over and the I/NAV CRC chain need that order).  Per page the lanes stage the deinterleaved, signed soft values in LDS; each of the
// symbols / 2 trellis steps then
//   - fetches the metrics of the lane's two predecessors, lanes 2 * (s & 31) and 2 * (s & 31) + 1: two ds_bpermute (__shfl).  The pattern gathers from
//     all four rows of the wave into each row, which no DPP control expresses (DPP moves within a row of 16, or broadcasts one lane of a row), and a
//     round trip through LDS memory would cost a write, a wait and two reads where bpermute uses the LDS crossbar alone;
//   - adds, compares and selects (tlm_acs);
//   - takes the wave maximum in six __shfl_xor butterflies and subtracts it (the reference normalises every step and the subtraction rounds, so the
//     maximum is on the dependent chain: the kernel is latency-bound on it by construction, a few hundred cycles per step);
//   - ballots the decision into the step's 64-bit word, kept in LDS (at most 492 x 8 B).
// Lane 0 then traces back from state 0 through the words and runs the bit-serial CRC.  All loops have trip counts fixed by the frame type, so non-finite
// symbols cannot hang the kernel (their result is unspecified).  No scratch: nothing per thread is indexed at run time.
//
// tlm_preamble_kernel: one thread per position, corr[i] = sum_k pre[k] * (sym[i + k] < 0 ? -1 : +1).
#include "gsh_internal.h"
#include "viterbi_acs.h"
#include <algorithm>
#include <new>
#include <vector>

struct gsh_tlm
{
    int device{0};
    int n_channels{0};
    int metric_mode{0};
    hipStream_t stream{nullptr};
    float* d_metrics{nullptr};    // [n_channels][64], reference mode's d_prev_section between pages and launches
    uint32_t* d_chain{nullptr};   // [n_channels], the CRC register each channel's last job ended with
    float* d_symbols{nullptr};    // staging of host symbols
    size_t symbols_capacity{0};
    int8_t* d_corr{nullptr};
    size_t corr_capacity{0};
    gsh_tlm_page_job* d_jobs{nullptr};
    gsh_tlm_page_result* d_results{nullptr};
    int32_t* d_order{nullptr};    // job indices grouped by channel, table order within a channel
    size_t jobs_capacity{0};
    int32_t* d_first{nullptr};    // [n_channels + 1], where each active channel's group starts in d_order
};

namespace gsh
{
namespace
{
constexpr int TLM_SCAN_THREADS = 256;

__global__ __launch_bounds__(TLM_STATES) void tlm_pages_kernel(const float* __restrict__ symbols, const gsh_tlm_page_job* __restrict__ jobs,
    const int32_t* __restrict__ order, const int32_t* __restrict__ first, gsh_tlm_page_result* __restrict__ results, float* __restrict__ metrics,
    uint32_t* __restrict__ chain, int metric_mode)
{
    __shared__ float soft[TLM_MAX_SYMBOLS];
    __shared__ uint64_t words[TLM_MAX_STEPS];
    __shared__ uint32_t bits[TLM_BIT_WORDS];
    __shared__ uint32_t crc_out[2];  // register, verdict
    const int lane = threadIdx.x;
    const int begin = first[blockIdx.x];
    const int end = first[blockIdx.x + 1];
    if (begin >= end) return;
    const int channel = jobs[order[begin]].channel;
    const int pred = 2 * (lane & 31);
    const int sym_lo = tlm_out_symbol(lane >> 5, pred);
    const int sym_hi = tlm_out_symbol(lane >> 5, pred + 1);
    const bool reference = metric_mode == TLM_METRIC_REFERENCE;
    float metric = reference ? metrics[static_cast<size_t>(channel) * TLM_STATES + lane] : -TLM_MAXLOG;
    uint32_t chain_reg = chain[channel];  // used by lane 0

    for (int k = begin; k < end; k++)
        {
            const int j = order[k];
            const gsh_tlm_page_job job = jobs[j];
            TlmGeometry g;
            tlm_geometry(job.frame_type, g);
            const float* in = symbols + job.symbol_offset;
            const bool invert = (job.flags & TLM_JOB_INVERT) != 0;
            for (int i = lane; i < g.symbols; i += TLM_STATES) soft[i] = tlm_soft(in, i, g.rows, g.cols, invert);
            __syncthreads();

            if (!reference) metric = -TLM_MAXLOG;
            if (lane == 0) metric = 0.0f;  // viterbi_decoder.cc:56
            for (int t = 0; t < g.steps; t++)
                {
                    const float rec0 = soft[2 * t];
                    const float rec1 = reference ? 0.0f : soft[2 * t + 1];
                    const float prev_lo = __shfl(metric, pred);
                    const float prev_hi = __shfl(metric, pred + 1);
                    int dec;
                    const float next = tlm_acs(sym_lo, sym_hi, prev_lo, prev_hi, rec0, rec1, dec);
                    float max_val = next;
#pragma unroll
                    for (int off = TLM_STATES / 2; off >= 1; off >>= 1) max_val = fmaxf(max_val, __shfl_xor(max_val, off));
                    metric = next - max_val;
                    const unsigned long long word = __ballot(dec);
                    if (lane == 0) words[t] = word;
                }
            __syncthreads();

            if (lane == 0)
                {
                    tlm_traceback(words, g.steps, g.info_bits, bits);
                    bool cont, check;
                    int n_bits, ok;
                    tlm_crc_plan(job.flags, job.crc_bits, job.crc_check, bits, cont, n_bits, check);
                    chain_reg = tlm_crc_run(cont ? chain_reg : 0u, bits, n_bits, check, ok);
                    crc_out[0] = chain_reg;
                    crc_out[1] = static_cast<uint32_t>(ok);
                }
            __syncthreads();
            if (lane < TLM_BIT_WORDS) results[j].bits[lane] = bits[lane];
            if (lane == TLM_BIT_WORDS) results[j].crc_register = crc_out[0];
            if (lane == TLM_BIT_WORDS + 1) results[j].crc_ok = static_cast<int32_t>(crc_out[1]);
            __syncthreads();  // bits and soft are rewritten by the next page
        }
    if (reference) metrics[static_cast<size_t>(channel) * TLM_STATES + lane] = metric;
    if (lane == 0) chain[channel] = chain_reg;
}

__global__ __launch_bounds__(TLM_SCAN_THREADS) void tlm_preamble_kernel(const float* __restrict__ symbols, unsigned long long n, int frame_type, int len,
    int8_t* __restrict__ corr)
{
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * TLM_SCAN_THREADS + threadIdx.x;
    if (i >= n) return;
    int acc = 0;
    if (i + len <= n)
        {
            for (int k = 0; k < len; k++)
                {
                    const int chip = tlm_preamble_chip(frame_type, k);
                    acc += symbols[i + k] < 0.0f ? -chip : chip;  // galileo_telemetry_decoder_gs.cc:964-971: a zero counts as positive
                }
        }
    corr[i] = static_cast<int8_t>(acc);
}

__global__ void tlm_reset_kernel(float* metrics, uint32_t* chain, int first_channel, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * TLM_STATES) metrics[static_cast<size_t>(first_channel) * TLM_STATES + i] = -TLM_MAXLOG;
    if (i < n) chain[first_channel + i] = 0u;
}

int reset_channels(gsh_tlm* h, int first_channel, int n)
{
    const int threads = 256;
    const int blocks = (n * TLM_STATES + threads - 1) / threads;
    hipLaunchKernelGGL(tlm_reset_kernel, dim3(blocks), dim3(threads), 0, h->stream, h->d_metrics, h->d_chain, first_channel, n);
    GSH_HIP(hipGetLastError());
    GSH_HIP(hipStreamSynchronize(h->stream));
    return GSH_OK;
}

// every range check of a job table, before anything touches the device
int check_jobs(int n_channels, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs)
{
    for (int j = 0; j < n_jobs; j++)
        {
            const gsh_tlm_page_job& job = jobs[j];
            TlmGeometry g;
            GSH_REQUIRE(tlm_geometry(job.frame_type, g), "job %d: unknown frame type %d", j, job.frame_type);
            GSH_REQUIRE(job.channel >= 0 && job.channel < n_channels, "job %d: channel %d outside 0..%d", j, job.channel, n_channels - 1);
            GSH_REQUIRE(job.symbol_offset <= n_symbols && n_symbols - job.symbol_offset >= static_cast<uint64_t>(g.symbols),
                "job %d: symbols %llu..+%d leave the buffer of %llu", j, static_cast<unsigned long long>(job.symbol_offset), g.symbols,
                static_cast<unsigned long long>(n_symbols));
            GSH_REQUIRE((job.flags & ~(TLM_JOB_INVERT | TLM_JOB_CRC_CONTINUE | TLM_JOB_INAV_AUTO)) == 0, "job %d: unknown flags 0x%x", j, job.flags);
            GSH_REQUIRE(!(job.flags & TLM_JOB_INAV_AUTO) || job.frame_type == 1, "job %d: GSH_TLM_JOB_INAV_AUTO on frame type %d", j, job.frame_type);
            GSH_REQUIRE(job.crc_bits >= 0 && job.crc_bits + (job.crc_check ? 24 : 0) <= g.info_bits, "job %d: crc_bits %d%s beyond the page's %d bits", j,
                job.crc_bits, job.crc_check ? " + 24" : "", g.info_bits);
        }
    return GSH_OK;
}

int reserve_jobs(gsh_tlm* h, size_t n_jobs)
{
    if (h->jobs_capacity >= n_jobs) return GSH_OK;
    if (h->d_jobs) (void)hipFree(h->d_jobs);
    if (h->d_results) (void)hipFree(h->d_results);
    if (h->d_order) (void)hipFree(h->d_order);
    h->d_jobs = nullptr;
    h->d_results = nullptr;
    h->d_order = nullptr;
    h->jobs_capacity = 0;
    GSH_HIP(hipMalloc(&h->d_jobs, sizeof(gsh_tlm_page_job) * n_jobs));
    GSH_HIP(hipMalloc(&h->d_results, sizeof(gsh_tlm_page_result) * n_jobs));
    GSH_HIP(hipMalloc(&h->d_order, sizeof(int32_t) * n_jobs));
    h->jobs_capacity = n_jobs;
    return GSH_OK;
}

// groups the table by channel (table order within a channel) and uploads it; *n_groups = channels that have jobs
int upload_jobs(gsh_tlm* h, const gsh_tlm_page_job* jobs, int n_jobs, int* n_groups)
{
    std::vector<int32_t> count(static_cast<size_t>(h->n_channels) + 1, 0);
    for (int j = 0; j < n_jobs; j++) count[jobs[j].channel + 1]++;
    std::vector<int32_t> first, slot(h->n_channels, 0);
    int32_t at = 0;
    for (int c = 0; c < h->n_channels; c++)
        {
            if (count[c + 1] == 0) continue;
            slot[c] = at;
            first.push_back(at);
            at += count[c + 1];
        }
    first.push_back(at);
    std::vector<int32_t> order(n_jobs);
    for (int j = 0; j < n_jobs; j++) order[slot[jobs[j].channel]++] = j;
    int rc = reserve_jobs(h, static_cast<size_t>(n_jobs));
    if (rc != GSH_OK) return rc;
    GSH_HIP(hipMemcpy(h->d_jobs, jobs, sizeof(gsh_tlm_page_job) * n_jobs, hipMemcpyHostToDevice));
    GSH_HIP(hipMemcpy(h->d_order, order.data(), sizeof(int32_t) * n_jobs, hipMemcpyHostToDevice));
    GSH_HIP(hipMemcpy(h->d_first, first.data(), sizeof(int32_t) * first.size(), hipMemcpyHostToDevice));
    *n_groups = static_cast<int>(first.size()) - 1;
    return GSH_OK;
}

void launch_pages(gsh_tlm* h, const float* device_symbols, int n_groups)
{
    hipLaunchKernelGGL(tlm_pages_kernel, dim3(n_groups), dim3(TLM_STATES), 0, h->stream, device_symbols, h->d_jobs, h->d_order, h->d_first, h->d_results,
        h->d_metrics, h->d_chain, h->metric_mode);
}

int stage_symbols(gsh_tlm* h, const float* symbols, uint64_t n)
{
    if (h->symbols_capacity < n)
        {
            if (h->d_symbols) (void)hipFree(h->d_symbols);
            h->d_symbols = nullptr;
            h->symbols_capacity = 0;
            GSH_HIP(hipMalloc(&h->d_symbols, sizeof(float) * n));
            h->symbols_capacity = n;
        }
    GSH_HIP(hipMemcpy(h->d_symbols, symbols, sizeof(float) * n, hipMemcpyHostToDevice));
    return GSH_OK;
}
}  // namespace
}  // namespace gsh

extern "C"
{
    int gsh_tlm_create(int device, int n_channels, int metric_mode, gsh_tlm_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null argument");
        *out = nullptr;
        GSH_REQUIRE(n_channels >= 1 && n_channels <= GSH_TLM_MAX_CHANNELS, "n_channels %d outside 1..%d", n_channels, GSH_TLM_MAX_CHANNELS);
        GSH_REQUIRE(metric_mode == GSH_TLM_METRIC_FULL || metric_mode == GSH_TLM_METRIC_REFERENCE, "unknown metric mode %d", metric_mode);
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_tlm* h = new (std::nothrow) gsh_tlm();
        GSH_REQUIRE(h != nullptr, "out of host memory");
        h->device = device;
        h->n_channels = n_channels;
        h->metric_mode = metric_mode;
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_tlm_destroy(h);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipMalloc(&h->d_metrics, sizeof(float) * gsh::TLM_STATES * n_channels)) != hipSuccess) return fail(e, "hipMalloc(metrics)");
        if ((e = hipMalloc(&h->d_chain, sizeof(uint32_t) * n_channels)) != hipSuccess) return fail(e, "hipMalloc(chain)");
        if ((e = hipMalloc(&h->d_first, sizeof(int32_t) * (static_cast<size_t>(n_channels) + 1))) != hipSuccess) return fail(e, "hipMalloc(first)");
        rc = gsh::reset_channels(h, 0, n_channels);
        if (rc != GSH_OK)
            {
                gsh_tlm_destroy(h);
                return rc;
            }
        *out = h;
        return GSH_OK;
    }

    void gsh_tlm_destroy(gsh_tlm_t* h)
    {
        if (!h) return;
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void* p : {static_cast<void*>(h->d_metrics), static_cast<void*>(h->d_chain), static_cast<void*>(h->d_symbols), static_cast<void*>(h->d_corr),
                 static_cast<void*>(h->d_jobs), static_cast<void*>(h->d_results), static_cast<void*>(h->d_order), static_cast<void*>(h->d_first)})
            if (p) (void)hipFree(p);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
    }

    int gsh_tlm_channel_reset(gsh_tlm_t* h, int channel)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        GSH_REQUIRE(channel >= 0 && channel < h->n_channels, "channel %d outside 0..%d", channel, h->n_channels - 1);
        GSH_HIP(hipSetDevice(h->device));
        return gsh::reset_channels(h, channel, 1);
    }

    int gsh_tlm_check_jobs(int n_channels, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs)
    {
        GSH_REQUIRE(n_channels >= 1 && n_channels <= GSH_TLM_MAX_CHANNELS, "n_channels %d outside 1..%d", n_channels, GSH_TLM_MAX_CHANNELS);
        GSH_REQUIRE(n_jobs >= 0 && (n_jobs == 0 || jobs != nullptr), "no job table");
        return gsh::check_jobs(n_channels, n_symbols, jobs, n_jobs);
    }

    int gsh_tlm_preamble_scan(gsh_tlm_t* h, int frame_type, const float* symbols, uint64_t n, int8_t* corr_out)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        gsh::TlmGeometry g;
        GSH_REQUIRE(gsh::tlm_geometry(frame_type, g), "unknown frame type %d", frame_type);
        if (n == 0) return GSH_OK;
        GSH_REQUIRE(symbols != nullptr && corr_out != nullptr, "null buffer");
        GSH_REQUIRE(n <= (1ull << 31), "block of %llu symbols is too long", static_cast<unsigned long long>(n));
        GSH_HIP(hipSetDevice(h->device));
        int rc = gsh::stage_symbols(h, symbols, n);
        if (rc != GSH_OK) return rc;
        if (h->corr_capacity < n)
            {
                if (h->d_corr) (void)hipFree(h->d_corr);
                h->d_corr = nullptr;
                h->corr_capacity = 0;
                GSH_HIP(hipMalloc(&h->d_corr, n));
                h->corr_capacity = n;
            }
        const unsigned blocks = static_cast<unsigned>((n + gsh::TLM_SCAN_THREADS - 1) / gsh::TLM_SCAN_THREADS);
        hipLaunchKernelGGL(gsh::tlm_preamble_kernel, dim3(blocks), dim3(gsh::TLM_SCAN_THREADS), 0, h->stream, h->d_symbols, static_cast<unsigned long long>(n),
            frame_type, g.preamble_len, h->d_corr);
        GSH_HIP(hipGetLastError());
        GSH_HIP(hipMemcpyAsync(corr_out, h->d_corr, n, hipMemcpyDeviceToHost, h->stream));
        GSH_HIP(hipStreamSynchronize(h->stream));
        return GSH_OK;
    }

    int gsh_tlm_decode_pages_device(gsh_tlm_t* h, const void* device_symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs,
        gsh_tlm_page_result* results)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        GSH_REQUIRE(n_jobs >= 0, "negative job count");
        if (n_jobs == 0) return GSH_OK;
        GSH_REQUIRE(jobs != nullptr && results != nullptr, "null job table");
        int rc = gsh::check_jobs(h->n_channels, n_symbols, jobs, n_jobs);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(device_symbols != nullptr, "null buffer");
        GSH_HIP(hipSetDevice(h->device));
        int n_groups = 0;
        rc = gsh::upload_jobs(h, jobs, n_jobs, &n_groups);
        if (rc != GSH_OK) return rc;
        gsh::launch_pages(h, static_cast<const float*>(device_symbols), n_groups);
        GSH_HIP(hipGetLastError());
        GSH_HIP(hipMemcpyAsync(results, h->d_results, sizeof(gsh_tlm_page_result) * n_jobs, hipMemcpyDeviceToHost, h->stream));
        GSH_HIP(hipStreamSynchronize(h->stream));
        return GSH_OK;
    }

    int gsh_tlm_decode_pages(gsh_tlm_t* h, const float* symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs, gsh_tlm_page_result* results)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        GSH_REQUIRE(n_jobs >= 0, "negative job count");
        if (n_jobs == 0) return GSH_OK;
        GSH_REQUIRE(jobs != nullptr && results != nullptr, "null job table");
        int rc = gsh::check_jobs(h->n_channels, n_symbols, jobs, n_jobs);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(symbols != nullptr, "null buffer");
        GSH_HIP(hipSetDevice(h->device));
        rc = gsh::stage_symbols(h, symbols, n_symbols);
        if (rc != GSH_OK) return rc;
        return gsh_tlm_decode_pages_device(h, h->d_symbols, n_symbols, jobs, n_jobs, results);
    }

    int gsh_tlm_time_decode_pages(gsh_tlm_t* h, const float* symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs, int reps, float* avg_ms)
    {
        GSH_REQUIRE(h != nullptr && avg_ms != nullptr, "null argument");
        GSH_REQUIRE(n_jobs >= 1 && reps >= 1, "nothing to time");
        GSH_REQUIRE(jobs != nullptr && symbols != nullptr, "null buffer");
        int rc = gsh::check_jobs(h->n_channels, n_symbols, jobs, n_jobs);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(h->device));
        rc = gsh::stage_symbols(h, symbols, n_symbols);
        if (rc != GSH_OK) return rc;
        int n_groups = 0;
        rc = gsh::upload_jobs(h, jobs, n_jobs, &n_groups);
        if (rc != GSH_OK) return rc;
        hipEvent_t t0, t1;
        GSH_HIP(hipEventCreate(&t0));
        GSH_HIP(hipEventCreate(&t1));
        gsh::launch_pages(h, h->d_symbols, n_groups);  // warm-up
        GSH_HIP(hipEventRecord(t0, h->stream));
        for (int r = 0; r < reps; r++) gsh::launch_pages(h, h->d_symbols, n_groups);
        GSH_HIP(hipEventRecord(t1, h->stream));
        GSH_HIP(hipEventSynchronize(t1));
        GSH_HIP(hipGetLastError());
        float ms = 0.0f;
        GSH_HIP(hipEventElapsedTime(&ms, t0, t1));
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
        *avg_ms = ms / static_cast<float>(reps);
        return GSH_OK;
    }
}
