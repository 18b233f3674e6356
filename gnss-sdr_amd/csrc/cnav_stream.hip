// GPS CNAV messages (L2C, L5) on the device: libswiftcnav's streaming decoder (src/algorithms/telemetry_decoder/libs/libswiftcnav/cnav_msg.c,
// viterbi27.c, bits.c, edc.c) as gps_l2c_telemetry_decoder_gs and gps_l5_telemetry_decoder_gs drive it.  The arithmetic is cnav_stream.h, shared with
// the host.
//
// cnav_stream_kernel: one wave64 per job (= per channel: a call's jobs have distinct channels), one lane per trellis state.  The wave walks the job's
// symbols in the reference's order, both parts per symbol: the part that holds the lock empties the other one's counts on every symbol, so the two
// parts of a channel cannot run as independent waves.  The channel's state is loaded at the start of the job and stored at its end: the two metric
// arrays of each part live in the lanes (lane n holds old_metrics[n] and new_metrics[n]), the decision ring (64 x 8 B per part), the symbol buffer and
// the 512-bit decode buffer in LDS, and everything a branch depends on (CnavRegs) in wave-uniform registers.  The job's symbols are staged in LDS in
// pieces of CNAV_CHUNK, float symbols through the quantiser on the way.  A symbol that does not complete a decode block costs one LDS byte and a few
// scalar operations per part.  A decode block (64 steps the first time, then 32) then
//   - fetches, per step, the metrics of the lane's two predecessors, lanes n >> 1 and (n >> 1) + 32: two ds_bpermute (__shfl); the gather crosses all
//     four rows of the wave, which no DPP control expresses (see telemetry_viterbi.hip);
//   - adds, compares and selects in integers (cnav_acs) and ballots the decision into the step's word of the ring;
//   - checks lane 0's new metric against 2^30 and, only then, takes the wave minimum in six __shfl_xor butterflies and subtracts it;
//   - ranks the metrics of the step before the last one (the reference's quirk, cnav_stream.h), takes the lowest lane that holds the minimum from a
//     ballot, and chases the 64 decisions back through the ring: a dependent chain of 64 LDS reads, the same on every lane;
//   - appends the 32 older bits to the decode buffer and runs the message-lock machine: the preamble rescan is one ballot per 64 buffer positions, the
//     buffer shifts are one word per lane, the CRC over 276 bits stays bit-serial (every lane computes the same value).
// All loop bounds come from the job's symbol count and the constants of cnav_stream.h, so no input can hang the kernel; a job never writes past its
// result capacity; its count goes on, so an overflow is seen.  No scratch: nothing per thread is indexed at run time.
#include "cnav_stream.h"
#include "gsh_internal.h"
#include <algorithm>
#include <new>
#include <vector>

struct gsh_cnav
{
    int device{0};
    int n_channels{0};
    int quantiser_mode{0};
    float soft_scale{1.0f};
    hipStream_t stream{nullptr};
    gsh_cnav_channel_state* d_states{nullptr};  // [n_channels]
    gsh_cnav_channel_state* d_saved{nullptr};   // [n_channels], gsh_cnav_time_push's copy
    void* d_symbols{nullptr};                   // staging of host symbols
    size_t symbols_capacity{0};                 // bytes
    gsh_cnav_job* d_jobs{nullptr};
    int32_t* d_counts{nullptr};
    size_t jobs_capacity{0};
    gsh_cnav_message* d_results{nullptr};
    size_t results_capacity{0};
};

namespace gsh
{
namespace
{
constexpr int CNAV_CHUNK = 1024;  // symbols staged in LDS at a time

__device__ inline uint32_t wave_uniform(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

// one part on the wave: the metrics in the lanes, the arrays in LDS
struct CnavLaneOps
{
    uint32_t& cur;   // old_metrics[lane]
    uint32_t& prev;  // new_metrics[lane]
    uint64_t* ring;
    uint8_t* sym;
    uint32_t* dec;
    const uint32_t lane;

    __device__ static bool uniform(bool v) { return wave_uniform(v ? 1u : 0u) != 0u; }
    __device__ static uint32_t uniform(uint32_t v) { return wave_uniform(v); }
    __device__ uint32_t word(uint32_t j) const { return dec[j]; }
    __device__ void put_symbol(uint32_t i, uint32_t symbol)
    {
        if (lane == 0) sym[i] = static_cast<uint8_t>(symbol);
    }
    __device__ void append(uint32_t n, uint32_t v)
    {
        if (lane == 0) cnav_append_words(dec, n, v);
        __syncthreads();
    }
    __device__ void shift(uint32_t k)
    {
        uint32_t w = 0;
        if (lane < static_cast<uint32_t>(CNAV_DECODED_WORDS)) w = cnav_shifted_word(dec, lane, k);
        __syncthreads();
        if (lane < static_cast<uint32_t>(CNAV_DECODED_WORDS)) dec[lane] = w;
        __syncthreads();
    }
    // the first i in 1 .. end - 1 at which a preamble sits, or 0: one ballot per 64 positions
    __device__ uint32_t find_preamble(uint32_t end, bool& inv) const
    {
        for (uint32_t base = 0; base < CNAV_DECODED_BITS; base += CNAV_STATES)
            {
                if (base >= end) break;
                const uint32_t i = base + lane;
                bool mine = false;
                const bool hit = i >= 1u && i < end && i + CNAV_PREAMBLE_BITS <= CNAV_DECODED_BITS && cnav_preamble_at(dec, i, mine);
                const unsigned long long mask = __ballot(hit);
                if (mask)
                    {
                        const uint32_t first = static_cast<uint32_t>(__ffsll(static_cast<long long>(mask))) - 1u;
                        inv = ((__ballot(hit && mine) >> first) & 1ull) != 0ull;
                        return base + first;
                    }
            }
        return 0;
    }
    __device__ void write_message(uint32_t* out, bool inv) const
    {
        if (lane < static_cast<uint32_t>(CNAV_MSG_WORDS))
            {
                const uint32_t mask = lane == static_cast<uint32_t>(CNAV_MSG_WORDS) - 1u ? ~(0xFFFFFFFFu >> (CNAV_MSG_BITS & 31u)) : 0xFFFFFFFFu;
                out[lane] = (dec[lane] ^ (inv ? 0xFFFFFFFFu : 0u)) & mask;
            }
    }
    __device__ uint32_t decode_block(uint32_t steps, uint32_t& index)
    {
        __syncthreads();  // lane 0's symbols
        uint32_t idx = index & (CNAV_HISTORY - 1u);
        const uint32_t lo_lane = lane >> 1, hi_lane = (lane >> 1) + 32u;
        for (uint32_t t = 0; t < steps && t < CNAV_FIRST_SYMBOLS / 2u; t++)
            {
                const uint32_t sym0 = sym[2u * t], sym1 = sym[2u * t + 1u];
                const uint32_t old_lo = static_cast<uint32_t>(__shfl(static_cast<int>(cur), static_cast<int>(lo_lane)));
                const uint32_t old_hi = static_cast<uint32_t>(__shfl(static_cast<int>(cur), static_cast<int>(hi_lane)));
                uint32_t decision;
                uint32_t next = cnav_acs(lane, old_lo, old_hi, sym0, sym1, decision);
                const unsigned long long word = __ballot(decision != 0u);
                if (lane == 0) ring[idx] = word;
                if (cnav_norm_due(wave_uniform(next)))  // lane 0 holds new metric 0
                    {
                        uint32_t lowest = next;
#pragma unroll
                        for (int off = CNAV_STATES / 2; off >= 1; off >>= 1)
                            {
                                const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(lowest), off));
                                lowest = other < lowest ? other : lowest;
                            }
                        next -= cnav_norm_floor(lowest);
                    }
                prev = cur;  // the reference's pointer swap
                cur = next;
                idx = (idx + 1u) & (CNAV_HISTORY - 1u);
            }
        index = idx;
        __syncthreads();  // the ring
        uint32_t lowest = prev;  // new_metrics: the step before the last one (the quirk)
#pragma unroll
        for (int off = CNAV_STATES / 2; off >= 1; off >>= 1)
            {
                const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(lowest), off));
                lowest = other < lowest ? other : lowest;
            }
        const unsigned long long holders = __ballot(prev == lowest);  // never empty; the reference keeps the first state that holds the minimum
        const uint32_t best = static_cast<uint32_t>(__ffsll(static_cast<long long>(holders))) - 1u;
        return wave_uniform(cnav_traceback(ring, idx, best));
    }
};

template <bool FLOAT_INPUT>
__global__ __launch_bounds__(CNAV_STATES) void cnav_stream_kernel(const void* __restrict__ symbols, const gsh_cnav_job* __restrict__ jobs,
    gsh_cnav_channel_state* __restrict__ states, gsh_cnav_message* __restrict__ results, int32_t* __restrict__ counts, int quantiser_mode, float soft_scale)
{
    __shared__ uint64_t ring[2][CNAV_HISTORY];
    __shared__ uint32_t decoded[2][CNAV_DECODED_WORDS];
    __shared__ uint8_t part_symbols[2][CNAV_FIRST_SYMBOLS];
    __shared__ uint8_t chunk[CNAV_CHUNK];
    const uint32_t lane = threadIdx.x;
    const gsh_cnav_job job = jobs[blockIdx.x];
    gsh_cnav_channel_state& st = states[job.channel];
    const uint32_t n = static_cast<uint32_t>(job.n_symbols);
    const uint32_t capacity = job.result_capacity;
    gsh_cnav_message* out = results + job.result_offset;

    uint32_t cur1 = st.part[0].old_metrics[lane], prev1 = st.part[0].new_metrics[lane];
    uint32_t cur2 = st.part[1].old_metrics[lane], prev2 = st.part[1].new_metrics[lane];
    CnavRegs r1, r2;
    r1 = CnavRegs{wave_uniform(st.part[0].n_symbols), wave_uniform(st.part[0].n_decoded), wave_uniform(st.part[0].flags), wave_uniform(st.part[0].n_crc_fail),
        wave_uniform(st.part[0].decisions_index)};
    r2 = CnavRegs{wave_uniform(st.part[1].n_symbols), wave_uniform(st.part[1].n_decoded), wave_uniform(st.part[1].flags), wave_uniform(st.part[1].n_crc_fail),
        wave_uniform(st.part[1].decisions_index)};
#pragma unroll
    for (int p = 0; p < 2; p++)
        {
            ring[p][lane] = st.part[p].decisions[lane];
            part_symbols[p][lane] = st.part[p].symbols[lane];
            part_symbols[p][lane + CNAV_STATES] = st.part[p].symbols[lane + CNAV_STATES];
            if (lane < static_cast<uint32_t>(CNAV_DECODED_WORDS)) decoded[p][lane] = st.part[p].decoded[lane];
        }
    __syncthreads();
    CnavLaneOps o1{cur1, prev1, ring[0], part_symbols[0], decoded[0], lane};
    CnavLaneOps o2{cur2, prev2, ring[1], part_symbols[1], decoded[1], lane};

    uint32_t count = 0;
    for (uint32_t base = 0; base < n; base += CNAV_CHUNK)
        {
            const uint32_t len = n - base < static_cast<uint32_t>(CNAV_CHUNK) ? n - base : static_cast<uint32_t>(CNAV_CHUNK);
            for (uint32_t i = lane; i < len; i += CNAV_STATES)
                {
                    const uint64_t at = job.symbol_offset + base + i;
                    if (FLOAT_INPUT)
                        chunk[i] = static_cast<uint8_t>(cnav_quantise(static_cast<const float*>(symbols)[at], quantiser_mode, soft_scale));
                    else
                        chunk[i] = static_cast<const uint8_t*>(symbols)[at];
                }
            __syncthreads();
            for (uint32_t k = 0; k < len; k++)
                {
                    const uint32_t symbol = wave_uniform(chunk[k]);
                    CnavDelivery d{};
                    gsh_cnav_message* slot = count < capacity ? out + count : nullptr;
                    const int part = cnav_channel_add_symbol(r1, o1, r2, o2, symbol, d, slot ? slot->bits : nullptr);
                    if (part != 0 && slot != nullptr)
                        {
                            if (lane == 10) slot->symbol_index = base + k;
                            if (lane == 11) slot->delay = d.delay;
                            if (lane == 12) slot->tow = d.tow;
                            if (lane == 13)
                                {
                                    slot->prn = static_cast<uint8_t>(d.prn);
                                    slot->msg_id = static_cast<uint8_t>(d.msg_id);
                                    slot->alert = static_cast<uint8_t>(d.alert);
                                    slot->part = static_cast<uint8_t>(part);
                                }
                            if (lane == 14)
                                {
                                    slot->invert = static_cast<uint8_t>(d.invert);
                                    slot->invert_or = ((r1.flags | r2.flags) & CNAV_FLAG_INVERT) ? 1 : 0;
                                    slot->reserved[0] = slot->reserved[1] = 0;
                                }
                        }
                    if (part != 0) count++;  // past the capacity nothing is written, but the count says how many there were
                }
            __syncthreads();  // the next piece overwrites chunk
        }

    st.part[0].old_metrics[lane] = cur1;
    st.part[0].new_metrics[lane] = prev1;
    st.part[1].old_metrics[lane] = cur2;
    st.part[1].new_metrics[lane] = prev2;
#pragma unroll
    for (int p = 0; p < 2; p++)
        {
            const CnavRegs& r = p == 0 ? r1 : r2;
            st.part[p].decisions[lane] = ring[p][lane];
            st.part[p].symbols[lane] = part_symbols[p][lane];
            st.part[p].symbols[lane + CNAV_STATES] = part_symbols[p][lane + CNAV_STATES];
            if (lane < static_cast<uint32_t>(CNAV_DECODED_WORDS)) st.part[p].decoded[lane] = decoded[p][lane];
            if (lane == 0) st.part[p].decisions_index = r.decisions_index;
            if (lane == 1) st.part[p].n_symbols = r.n_symbols;
            if (lane == 2) st.part[p].n_decoded = r.n_decoded;
            if (lane == 3) st.part[p].flags = r.flags;
            if (lane == 4) st.part[p].n_crc_fail = r.n_crc_fail;
        }
    if (lane == 0) counts[blockIdx.x] = static_cast<int32_t>(count);
}

static_assert(sizeof(gsh_cnav_part_state) == 1240 && sizeof(gsh_cnav_channel_state) == 2480 && sizeof(gsh_cnav_message) == 60 && sizeof(gsh_cnav_job) == 32,
    "layouts of include/gnss_sdr_hip.h");

// every range check of a job table, before anything touches the device
int check_jobs(int n_channels, uint64_t n_symbols, uint32_t n_results, const gsh_cnav_job* jobs, int n_jobs)
{
    std::vector<char> taken(static_cast<size_t>(n_channels), 0);
    std::vector<std::pair<uint64_t, int>> slices;
    slices.reserve(static_cast<size_t>(n_jobs));
    for (int j = 0; j < n_jobs; j++)
        {
            const gsh_cnav_job& job = jobs[j];
            GSH_REQUIRE(job.channel >= 0 && job.channel < n_channels, "job %d: channel %d outside 0..%d", j, job.channel, n_channels - 1);
            GSH_REQUIRE(!taken[job.channel], "job %d: channel %d has another job in this call", j, job.channel);
            taken[job.channel] = 1;
            GSH_REQUIRE(job.n_symbols <= (1ull << 31), "job %d: %llu symbols are too many for one job", j, static_cast<unsigned long long>(job.n_symbols));
            GSH_REQUIRE(job.symbol_offset <= n_symbols && n_symbols - job.symbol_offset >= job.n_symbols, "job %d: symbols %llu..+%llu leave the array of %llu",
                j, static_cast<unsigned long long>(job.symbol_offset), static_cast<unsigned long long>(job.n_symbols),
                static_cast<unsigned long long>(n_symbols));
            GSH_REQUIRE(job.result_capacity >= cnav_result_capacity(job.n_symbols), "job %d: result capacity %u below the %llu that %llu symbols can deliver",
                j, job.result_capacity, static_cast<unsigned long long>(cnav_result_capacity(job.n_symbols)),
                static_cast<unsigned long long>(job.n_symbols));
            GSH_REQUIRE(job.result_offset <= n_results && n_results - job.result_offset >= job.result_capacity,
                "job %d: results %u..+%u leave the array of %u", j, job.result_offset, job.result_capacity, n_results);
            slices.emplace_back(job.result_offset, j);
        }
    std::sort(slices.begin(), slices.end());
    for (size_t s = 1; s < slices.size(); s++)
        {
            const gsh_cnav_job& before = jobs[slices[s - 1].second];
            GSH_REQUIRE(static_cast<uint64_t>(before.result_offset) + before.result_capacity <= slices[s].first,
                "job %d: its result slice overlaps that of job %d", std::max(slices[s].second, slices[s - 1].second),
                std::min(slices[s].second, slices[s - 1].second));
        }
    return GSH_OK;
}

int reserve(gsh_cnav* h, size_t n_jobs, size_t n_results)
{
    if (h->jobs_capacity < n_jobs)
        {
            if (h->d_jobs) (void)hipFree(h->d_jobs);
            if (h->d_counts) (void)hipFree(h->d_counts);
            h->d_jobs = nullptr;
            h->d_counts = nullptr;
            h->jobs_capacity = 0;
            GSH_HIP(hipMalloc(&h->d_jobs, sizeof(gsh_cnav_job) * n_jobs));
            GSH_HIP(hipMalloc(&h->d_counts, sizeof(int32_t) * n_jobs));
            h->jobs_capacity = n_jobs;
        }
    if (h->results_capacity < n_results)
        {
            if (h->d_results) (void)hipFree(h->d_results);
            h->d_results = nullptr;
            h->results_capacity = 0;
            GSH_HIP(hipMalloc(&h->d_results, sizeof(gsh_cnav_message) * n_results));
            h->results_capacity = n_results;
        }
    return GSH_OK;
}

int stage_symbols(gsh_cnav* h, const void* symbols, size_t bytes)
{
    if (h->symbols_capacity < bytes)
        {
            if (h->d_symbols) (void)hipFree(h->d_symbols);
            h->d_symbols = nullptr;
            h->symbols_capacity = 0;
            GSH_HIP(hipMalloc(&h->d_symbols, bytes));
            h->symbols_capacity = bytes;
        }
    GSH_HIP(hipMemcpy(h->d_symbols, symbols, bytes, hipMemcpyHostToDevice));
    return GSH_OK;
}

void launch(gsh_cnav* h, const void* device_symbols, bool float_input, int n_jobs)
{
    if (float_input)
        hipLaunchKernelGGL(cnav_stream_kernel<true>, dim3(n_jobs), dim3(CNAV_STATES), 0, h->stream, device_symbols, h->d_jobs, h->d_states, h->d_results,
            h->d_counts, h->quantiser_mode, h->soft_scale);
    else
        hipLaunchKernelGGL(cnav_stream_kernel<false>, dim3(n_jobs), dim3(CNAV_STATES), 0, h->stream, device_symbols, h->d_jobs, h->d_states, h->d_results,
            h->d_counts, h->quantiser_mode, h->soft_scale);
}

int reset_channels(gsh_cnav* h, int first_channel, int n)
{
    gsh_cnav_channel_state fresh;
    cnav_channel_init(fresh);
    std::vector<gsh_cnav_channel_state> all(static_cast<size_t>(n), fresh);
    GSH_HIP(hipMemcpy(h->d_states + first_channel, all.data(), sizeof(gsh_cnav_channel_state) * all.size(), hipMemcpyHostToDevice));
    return GSH_OK;
}

// checks, upload, launch, and the messages each job wrote back into the caller's arrays; symbols == nullptr: device_symbols is the caller's
int push(gsh_cnav* h, const void* symbols, const void* device_symbols, bool float_input, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs,
    gsh_cnav_message* results, uint32_t n_results, int32_t* counts)
{
    GSH_REQUIRE(h != nullptr, "null handle");
    GSH_REQUIRE(n_jobs >= 0, "negative job count");
    if (n_jobs == 0) return GSH_OK;
    GSH_REQUIRE(jobs != nullptr && results != nullptr && counts != nullptr, "null job table");
    int rc = check_jobs(h->n_channels, n_symbols, n_results, jobs, n_jobs);
    if (rc != GSH_OK) return rc;
    GSH_REQUIRE(n_symbols == 0 || symbols != nullptr || device_symbols != nullptr, "null buffer");
    GSH_HIP(hipSetDevice(h->device));
    if (symbols != nullptr && n_symbols > 0)
        {
            rc = stage_symbols(h, symbols, static_cast<size_t>(n_symbols) * (float_input ? sizeof(float) : 1u));
            if (rc != GSH_OK) return rc;
            device_symbols = h->d_symbols;
        }
    rc = reserve(h, static_cast<size_t>(n_jobs), n_results);
    if (rc != GSH_OK) return rc;
    GSH_HIP(hipMemcpy(h->d_jobs, jobs, sizeof(gsh_cnav_job) * n_jobs, hipMemcpyHostToDevice));
    launch(h, device_symbols, float_input, n_jobs);
    GSH_HIP(hipGetLastError());
    std::vector<gsh_cnav_message> back(n_results);
    GSH_HIP(hipMemcpyAsync(counts, h->d_counts, sizeof(int32_t) * n_jobs, hipMemcpyDeviceToHost, h->stream));
    GSH_HIP(hipMemcpyAsync(back.data(), h->d_results, sizeof(gsh_cnav_message) * n_results, hipMemcpyDeviceToHost, h->stream));
    GSH_HIP(hipStreamSynchronize(h->stream));
    for (int j = 0; j < n_jobs; j++)
        {
            const uint32_t written = std::min(static_cast<uint32_t>(std::max(counts[j], 0)), jobs[j].result_capacity);
            std::copy(back.begin() + jobs[j].result_offset, back.begin() + jobs[j].result_offset + written, results + jobs[j].result_offset);
        }
    for (int j = 0; j < n_jobs; j++)  // only a channel whose state was imported with a message's worth of bits already decoded can come here
        if (counts[j] > 0 && static_cast<uint32_t>(counts[j]) > jobs[j].result_capacity)
            return set_error(GSH_ERR_STATE, "job %d: channel %d delivered %d messages, its result capacity is %u; the first %u of each job were written",
                j, jobs[j].channel, counts[j], jobs[j].result_capacity, jobs[j].result_capacity);
    return GSH_OK;
}
}  // namespace
}  // namespace gsh

extern "C"
{
    int gsh_cnav_create(int device, int n_channels, int quantiser_mode, float soft_scale, gsh_cnav_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null argument");
        *out = nullptr;
        GSH_REQUIRE(n_channels >= 1 && n_channels <= GSH_CNAV_MAX_CHANNELS, "n_channels %d outside 1..%d", n_channels, GSH_CNAV_MAX_CHANNELS);
        GSH_REQUIRE(quantiser_mode == GSH_CNAV_QUANTISER_HARD || quantiser_mode == GSH_CNAV_QUANTISER_SOFT, "unknown quantiser mode %d", quantiser_mode);
        GSH_REQUIRE(quantiser_mode == GSH_CNAV_QUANTISER_HARD || (soft_scale > 0.0f && soft_scale < 3e38f), "soft scale %g is not a positive number",
            static_cast<double>(soft_scale));
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_cnav* h = new (std::nothrow) gsh_cnav();
        GSH_REQUIRE(h != nullptr, "out of host memory");
        h->device = device;
        h->n_channels = n_channels;
        h->quantiser_mode = quantiser_mode;
        h->soft_scale = quantiser_mode == GSH_CNAV_QUANTISER_SOFT ? soft_scale : 1.0f;
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_cnav_destroy(h);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipMalloc(&h->d_states, sizeof(gsh_cnav_channel_state) * n_channels)) != hipSuccess) return fail(e, "hipMalloc(states)");
        rc = gsh::reset_channels(h, 0, n_channels);
        if (rc != GSH_OK)
            {
                gsh_cnav_destroy(h);
                return rc;
            }
        *out = h;
        return GSH_OK;
    }

    void gsh_cnav_destroy(gsh_cnav_t* h)
    {
        if (!h) return;
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void* p : {static_cast<void*>(h->d_states), static_cast<void*>(h->d_saved), h->d_symbols, static_cast<void*>(h->d_jobs),
                 static_cast<void*>(h->d_counts), static_cast<void*>(h->d_results)})
            if (p) (void)hipFree(p);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
    }

    int gsh_cnav_channel_reset(gsh_cnav_t* h, int channel)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        GSH_REQUIRE(channel >= 0 && channel < h->n_channels, "channel %d outside 0..%d", channel, h->n_channels - 1);
        GSH_HIP(hipSetDevice(h->device));
        return gsh::reset_channels(h, channel, 1);
    }

    int gsh_cnav_check_jobs(int n_channels, uint64_t n_symbols, uint32_t n_results, const gsh_cnav_job* jobs, int n_jobs)
    {
        GSH_REQUIRE(n_channels >= 1 && n_channels <= GSH_CNAV_MAX_CHANNELS, "n_channels %d outside 1..%d", n_channels, GSH_CNAV_MAX_CHANNELS);
        GSH_REQUIRE(n_jobs >= 0 && (n_jobs == 0 || jobs != nullptr), "no job table");
        return gsh::check_jobs(n_channels, n_symbols, n_results, jobs, n_jobs);
    }

    int gsh_cnav_push_u8(gsh_cnav_t* h, const uint8_t* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, gsh_cnav_message* results,
        uint32_t n_results, int32_t* counts)
    {
        return gsh::push(h, symbols, nullptr, false, n_symbols, jobs, n_jobs, results, n_results, counts);
    }

    int gsh_cnav_push_f32(gsh_cnav_t* h, const float* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, gsh_cnav_message* results,
        uint32_t n_results, int32_t* counts)
    {
        return gsh::push(h, symbols, nullptr, true, n_symbols, jobs, n_jobs, results, n_results, counts);
    }

    int gsh_cnav_push_f32_device(gsh_cnav_t* h, const void* device_symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs,
        gsh_cnav_message* results, uint32_t n_results, int32_t* counts)
    {
        return gsh::push(h, nullptr, device_symbols, true, n_symbols, jobs, n_jobs, results, n_results, counts);
    }

    int gsh_cnav_time_push(gsh_cnav_t* h, const uint8_t* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, int reps, float* avg_ms)
    {
        GSH_REQUIRE(h != nullptr && avg_ms != nullptr, "null argument");
        GSH_REQUIRE(n_jobs >= 1 && reps >= 1, "nothing to time");
        GSH_REQUIRE(jobs != nullptr && symbols != nullptr && n_symbols >= 1, "null buffer");
        uint64_t n_results = 0;
        std::vector<gsh_cnav_job> table(jobs, jobs + n_jobs);
        for (gsh_cnav_job& job : table)  // the timing run lays the result slices out itself
            {
                job.result_offset = static_cast<uint32_t>(n_results);
                job.result_capacity = static_cast<uint32_t>(gsh::cnav_result_capacity(std::min<uint64_t>(job.n_symbols, 1ull << 31)));
                n_results += job.result_capacity;
            }
        GSH_REQUIRE(n_results <= 0xFFFFFFFFull, "too many results");
        int rc = gsh::check_jobs(h->n_channels, n_symbols, static_cast<uint32_t>(n_results), table.data(), n_jobs);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(h->device));
        rc = gsh::stage_symbols(h, symbols, static_cast<size_t>(n_symbols));
        if (rc != GSH_OK) return rc;
        rc = gsh::reserve(h, static_cast<size_t>(n_jobs), static_cast<size_t>(n_results));
        if (rc != GSH_OK) return rc;
        const size_t state_bytes = sizeof(gsh_cnav_channel_state) * h->n_channels;
        if (!h->d_saved) GSH_HIP(hipMalloc(&h->d_saved, state_bytes));
        GSH_HIP(hipMemcpy(h->d_jobs, table.data(), sizeof(gsh_cnav_job) * n_jobs, hipMemcpyHostToDevice));
        GSH_HIP(hipMemcpyAsync(h->d_saved, h->d_states, state_bytes, hipMemcpyDeviceToDevice, h->stream));
        hipEvent_t t0 = nullptr, t1 = nullptr;
        float total = 0.0f;
        hipError_t e = hipEventCreate(&t0);
        if (e == hipSuccess) e = hipEventCreate(&t1);
        for (int r = -1; r < reps && e == hipSuccess; r++)  // r = -1: warm-up
            {
                if ((e = hipEventRecord(t0, h->stream)) != hipSuccess) break;
                gsh::launch(h, h->d_symbols, false, n_jobs);
                if ((e = hipEventRecord(t1, h->stream)) != hipSuccess) break;
                if ((e = hipMemcpyAsync(h->d_states, h->d_saved, state_bytes, hipMemcpyDeviceToDevice, h->stream)) != hipSuccess) break;
                if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) break;
                float ms = 0.0f;
                if ((e = hipEventElapsedTime(&ms, t0, t1)) != hipSuccess) break;
                if (r >= 0) total += ms;
            }
        if (e == hipSuccess) e = hipGetLastError();
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (e != hipSuccess) return gsh::hip_fail(e, "gsh_cnav_time_push", __FILE__, __LINE__);
        *avg_ms = total / static_cast<float>(reps);
        return GSH_OK;
    }

    int gsh_cnav_channel_get_state(gsh_cnav_t* h, int channel, gsh_cnav_channel_state* state)
    {
        GSH_REQUIRE(h != nullptr && state != nullptr, "null argument");
        GSH_REQUIRE(channel >= 0 && channel < h->n_channels, "channel %d outside 0..%d", channel, h->n_channels - 1);
        GSH_HIP(hipSetDevice(h->device));
        GSH_HIP(hipStreamSynchronize(h->stream));
        GSH_HIP(hipMemcpy(state, h->d_states + channel, sizeof(gsh_cnav_channel_state), hipMemcpyDeviceToHost));
        return GSH_OK;
    }

    int gsh_cnav_channel_set_state(gsh_cnav_t* h, int channel, const gsh_cnav_channel_state* state)
    {
        GSH_REQUIRE(h != nullptr && state != nullptr, "null argument");
        GSH_REQUIRE(channel >= 0 && channel < h->n_channels, "channel %d outside 0..%d", channel, h->n_channels - 1);
        GSH_REQUIRE(gsh::cnav_state_valid(*state), "channel state with an index or count outside its array");
        GSH_HIP(hipSetDevice(h->device));
        GSH_HIP(hipStreamSynchronize(h->stream));
        GSH_HIP(hipMemcpy(h->d_states + channel, state, sizeof(gsh_cnav_channel_state), hipMemcpyHostToDevice));
        return GSH_OK;
    }
}
