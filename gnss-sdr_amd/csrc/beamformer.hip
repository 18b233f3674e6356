// gsh_beam_*: the spatial filter of Array_Signal_Conditioner (Beamformer_Filter, src/algorithms/input_filter/gnuradio_blocks/beamformer.{h,cc}) for
// up to 8 antennas and up to 8 beams at once, each beam straight into its own sample ring, and the array covariance the weights are computed from.
// See include/gnss_sdr_hip.h for the contract.  The arithmetic is beamformer.cc:53-61 in float32, one rounding per operation (-ffp-contract=off).
// Adaptive mode (gsh_adaptive_beam_set): a call first forms the block's covariance, accumulates it and solves for every beam's weights on the device
// (array_weights.h is that arithmetic), then forms the beams with the weights it finds in device memory -- one chain on the call's stream.
#include "array_weights.h"
#include "sample_convert.h"
#include "sample_stream.h"
#include <new>

namespace
{
using gsh::set_error;

constexpr int BF_THREADS = 256;
constexpr int BF_MAX = 8;            // GSH_ARRAY_MAX_ANTENNAS = GSH_ARRAY_MAX_BEAMS
constexpr int BF_GRID_CAP = 256 * 8; // grid-stride beyond eight work-groups per compute unit: the kernel streams, 16 A .. 64 A bytes in flight per lane

// one item of the array's streams as it lies in memory: two values of the item type (which of them is I: first_is_q)
template <typename T>
struct alignas(2 * sizeof(T)) Item
{
    T first, second;
};

// what a launch reads and writes, passed by value: the weights are kernel arguments (wave-uniform, scalar loads), so a launch uses the weights as they
// stood when it was queued and gsh_beam_set_weights needs no ordering on the device
struct BeamArgs
{
    const void* src[BF_MAX];  // planar: antenna a's items; interleaved: src[0], item k * A + a
    float2* dst[BF_MAX];      // beam b's output, sample 0 of the launch first
    float2 w[BF_MAX][BF_MAX]; // [beam][antenna]
    unsigned long long n;
    int n_ant, n_beams;
    int first_is_q;
    float qsign;              // -1: inverted spectrum (conjugate)
    int vec;                  // interleaved only: frames are whole 16-byte words at 16-byte aligned addresses
};

template <typename T>
__device__ __forceinline__ float2 to_sample(T u, T v, int first_is_q, float qsign)
{
    const float fu = static_cast<float>(u), fv = static_cast<float>(v);
    return make_float2(first_is_q ? fv : fu, qsign * (first_is_q ? fu : fv));
}

// item a of a frame held as 32-bit words
template <typename T>
__device__ __forceinline__ float2 word_sample(const uint32_t (&raw)[16], int a, int first_is_q, float qsign)
{
    if constexpr (sizeof(T) == 1)
        {
            const uint32_t h = raw[a >> 1] >> (16 * (a & 1));
            return to_sample(static_cast<int8_t>(h & 0xffu), static_cast<int8_t>((h >> 8) & 0xffu), first_is_q, qsign);
        }
    else if constexpr (sizeof(T) == 2)
        return to_sample(static_cast<int16_t>(raw[a] & 0xffffu), static_cast<int16_t>(raw[a] >> 16), first_is_q, qsign);
    else
        return to_sample(__uint_as_float(raw[2 * a]), __uint_as_float(raw[2 * a + 1]), first_is_q, qsign);
}

// the A items of sample k as complex floats: the integer -> float cast of the ring pushes (sample_convert.hip), (I, Q) per first_is_q, conjugated by qsign
template <typename T, int LAYOUT>
__device__ __forceinline__ void load_frame(const BeamArgs& g, unsigned long long k, float2 (&x)[BF_MAX])
{
    const int A = g.n_ant;
    if (LAYOUT == GSH_ARRAY_INTERLEAVED && g.vec)
        {
            constexpr int PER_VEC = 16 / static_cast<int>(sizeof(Item<T>));  // items per 16-byte load: 8 / 4 / 2
            constexpr int N_VEC = BF_MAX / PER_VEC;                          // loads of the longest frame: 1 / 2 / 4
            const uint4* p = reinterpret_cast<const uint4*>(static_cast<const char*>(g.src[0]) + k * (static_cast<unsigned long long>(A) * sizeof(Item<T>)));
            uint32_t raw[16];
#pragma unroll
            for (int c = 0; c < N_VEC; c++)
                if (c * PER_VEC < A)
                    {
                        const uint4 v = p[c];
                        raw[4 * c] = v.x;
                        raw[4 * c + 1] = v.y;
                        raw[4 * c + 2] = v.z;
                        raw[4 * c + 3] = v.w;
                    }
#pragma unroll
            for (int a = 0; a < BF_MAX; a++)
                if (a < A) x[a] = word_sample<T>(raw, a, g.first_is_q, g.qsign);
        }
    else
        {
#pragma unroll
            for (int a = 0; a < BF_MAX; a++)
                if (a < A)
                    {
                        const Item<T> it = LAYOUT == GSH_ARRAY_INTERLEAVED ? static_cast<const Item<T>*>(g.src[0])[k * static_cast<unsigned long long>(A) + a]
                                                                           : static_cast<const Item<T>*>(g.src[a])[k];
                        x[a] = to_sample(it.first, it.second, g.first_is_q, g.qsign);
                    }
        }
}

// One lane owns a sample and forms every beam's sum over the antennas in the block's order (beamformer.cc:56-61): sum = (0, 0); sum = sum + x[a] * w[a].
// Lanes of a wave read consecutive frames (interleaved: consecutive 16-byte words where the frame is whole words) or consecutive items of each antenna
// (planar) and write consecutive float2 per beam.  Algorithmic bytes per sample: A x item size in, 8 B out.
template <typename T, int LAYOUT>
__global__ __launch_bounds__(BF_THREADS) void beam_kernel(const BeamArgs g)
{
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * BF_THREADS;
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * BF_THREADS + threadIdx.x; k < g.n; k += stride)
        {
            float2 x[BF_MAX];
            load_frame<T, LAYOUT>(g, k, x);
#pragma unroll
            for (int b = 0; b < BF_MAX; b++)
                if (b < g.n_beams)
                    {
                        float2 sum = make_float2(0.0f, 0.0f);
#pragma unroll
                        for (int a = 0; a < BF_MAX; a++)
                            if (a < g.n_ant)
                                {
                                    const float2 w = g.w[b][a];
                                    const float pre = x[a].x * w.x - x[a].y * w.y;
                                    const float pim = x[a].x * w.y + x[a].y * w.x;
                                    sum.x += pre;
                                    sum.y += pim;
                                }
                        g.dst[b][k] = sum;
                    }
        }
}

// The beam pass of an adaptive handle: beam_kernel term for term, the weights read from device memory (gsh::AwState::w, [beam][antenna]) where the solver
// of the same chain left them.  They are the same for every lane of the grid and nothing in the launch writes them (const __restrict__): the compiler
// takes them with scalar loads, as it takes beam_kernel's from the kernel arguments.  Equal weights give equal bits.
template <typename T, int LAYOUT>
__global__ __launch_bounds__(BF_THREADS) void beam_kernel_device_weights(const BeamArgs g, const float2* __restrict__ w_dev)
{
    const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * BF_THREADS;
    for (unsigned long long k = static_cast<unsigned long long>(blockIdx.x) * BF_THREADS + threadIdx.x; k < g.n; k += stride)
        {
            float2 x[BF_MAX];
            load_frame<T, LAYOUT>(g, k, x);
#pragma unroll
            for (int b = 0; b < BF_MAX; b++)
                if (b < g.n_beams)
                    {
                        float2 sum = make_float2(0.0f, 0.0f);
#pragma unroll
                        for (int a = 0; a < BF_MAX; a++)
                            if (a < g.n_ant)
                                {
                                    const float2 w = w_dev[b * BF_MAX + a];
                                    const float pre = x[a].x * w.x - x[a].y * w.y;
                                    const float pim = x[a].x * w.y + x[a].y * w.x;
                                    sum.x += pre;
                                    sum.y += pim;
                                }
                        g.dst[b][k] = sum;
                    }
        }
}

// ---- covariance: R[i][j] = sum_n x_i[n] conj(x_j[n]) over the upper triangle, FP64 products (exact for float32 factors) and sums.
// A work-group stages a tile of COV_TILE samples of every antenna in LDS; its threads are dealt P = A (A + 1) / 2 pairs x S = 256 / P sample slices, thread
// (pair, slice s) adds samples s, s + S, ... of every tile the group walks; the S slices of a pair are then added in slice order and the group writes one
// partial per pair.  A second kernel adds the groups' partials in group order.  The grid depends on n alone: the same data give the same bits every run.
constexpr int COV_TILE = 256;
constexpr int COV_GRID_CAP = 512;
constexpr int COV_PAIRS = BF_MAX * (BF_MAX + 1) / 2;

template <typename T, int LAYOUT>
__global__ __launch_bounds__(BF_THREADS) void cov_partial_kernel(const BeamArgs g, double2* __restrict__ partial)
{
    __shared__ float2 tile[BF_MAX][COV_TILE];
    __shared__ double2 red[BF_THREADS];
    const int A = g.n_ant;
    const int P = A * (A + 1) / 2;
    const int S = BF_THREADS / P;
    const int t = threadIdx.x;
    const int pair = t / S, s = t - pair * S;
    int i = 0, j = pair;  // pair -> (i, j), i <= j, row by row of the upper triangle
    while (i < A - 1 && j >= A - i)
        {
            j -= A - i;
            i++;
        }
    j += i;
    double re = 0.0, im = 0.0;
    const unsigned long long n_tiles = (g.n + COV_TILE - 1) / COV_TILE;
    for (unsigned long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x)
        {
            const unsigned long long k = tl * COV_TILE + t;
            float2 x[BF_MAX];
#pragma unroll
            for (int a = 0; a < BF_MAX; a++) x[a] = make_float2(0.0f, 0.0f);
            if (k < g.n) load_frame<T, LAYOUT>(g, k, x);
            __syncthreads();  // the previous tile has been read
#pragma unroll
            for (int a = 0; a < BF_MAX; a++)
                if (a < A) tile[a][t] = x[a];
            __syncthreads();
            if (pair < P)
                for (int m = s; m < COV_TILE; m += S)
                    {
                        const float2 u = tile[i][m], v = tile[j][m];
                        const double ur = u.x, ui = u.y, vr = v.x, vi = v.y;
                        re += ur * vr;
                        re += ui * vi;
                        im += ui * vr;
                        im -= ur * vi;
                    }
        }
    red[t] = make_double2(re, im);
    __syncthreads();
    if (pair < P && s == 0)
        {
            double2 acc = red[t];
            for (int m = 1; m < S; m++)
                {
                    acc.x += red[t + m].x;
                    acc.y += red[t + m].y;
                }
            partial[static_cast<size_t>(blockIdx.x) * COV_PAIRS + pair] = acc;
        }
}

__global__ __launch_bounds__(64) void cov_final_kernel(const double2* __restrict__ partial, int groups, int pairs, double2* __restrict__ out)
{
    const int p = threadIdx.x;
    if (p >= pairs) return;
    double2 acc = make_double2(0.0, 0.0);
    for (int gidx = 0; gidx < groups; gidx++)
        {
            const double2 v = partial[static_cast<size_t>(gidx) * COV_PAIRS + p];
            acc.x += v.x;
            acc.y += v.y;
        }
    out[p] = acc;
}

// ---- adaptive mode: accumulate the block's covariance and solve for every beam's weights (array_weights.h is the arithmetic), one work-group of one wave.
// Lane p < P accumulates pair p; lane 0 loads and factorises into LDS; lane b < n_beams walks beam b's solve; then every lane stores one weight and lane 0
// the counters.  The state is read before the first barrier and written after it with ordinary vector stores.
struct AdaptArgs
{
    gsh::AwConf conf;
    int n_ant, n_beams;
    int reset;  // the mode was set since the last chain: the state in memory counts as zero
};

__global__ __launch_bounds__(64) void adapt_solve_kernel(const AdaptArgs g, const double2* __restrict__ block, gsh::AwState* __restrict__ s)
{
    __shared__ double acc[2 * gsh::AW_PAIRS];
    __shared__ double l_re[BF_MAX * BF_MAX], l_im[BF_MAX * BF_MAX], d[BF_MAX];
    __shared__ float w[BF_MAX][BF_MAX][2];
    __shared__ int went[BF_MAX + 1];
    const int t = threadIdx.x;
    const int A = g.n_ant;
    const int P = A * (A + 1) / 2;
    const bool had = !g.reset && s->solved != 0;
    const unsigned long long blocks = g.reset ? 0ull : s->blocks, failures = g.reset ? 0ull : s->failures;
    if (t < P)
        {
            acc[2 * t] = g.reset ? 0.0 : s->r_acc[2 * t];
            acc[2 * t + 1] = g.reset ? 0.0 : s->r_acc[2 * t + 1];
            gsh::aw_accumulate_pair(A, t, g.conf.forgetting, reinterpret_cast<const double*>(block), acc);
        }
    __syncthreads();
    if (t < P)
        {
            s->r_acc[2 * t] = acc[2 * t];
            s->r_acc[2 * t + 1] = acc[2 * t + 1];
        }
    if (t == 0)
        {
            bool ok = true;
            for (int p = 0; p < 2 * P; p++) ok = ok && gsh::aw_finite(acc[p]);
            const double delta = gsh::aw_loading(A, acc, g.conf.loading_rel, g.conf.loading_abs);
            s->delta = delta;
            ok = gsh::aw_factor(A, acc, delta, l_re, l_im, d) && ok;
            went[BF_MAX] = ok ? 1 : 0;
        }
    __syncthreads();
    if (t < g.n_beams) went[t] = gsh::aw_solve(A, l_re, l_im, d, g.conf.c[t], nullptr, w[t]) ? 1 : 0;
    __syncthreads();
    bool ok = went[BF_MAX] != 0;
    for (int b = 0; b < g.n_beams; b++) ok = went[b] != 0 && ok;
    const int b = t / BF_MAX, a = t % BF_MAX;
    if (b < g.n_beams && a < A)
        for (int q = 0; q < 2; q++)
            {
                if (ok)
                    s->w[b][a][q] = w[b][a][q];
                else if (!had)
                    s->w[b][a][q] = g.conf.fixed_w[b][a][q];
            }
    if (t == 0)
        {
            s->blocks = blocks + 1;
            s->failures = failures + (ok ? 0ull : 1ull);
            s->solved = (ok || had) ? 1ull : 0ull;
        }
}
}  // namespace

struct gsh_beam
{
    int device{0};
    gsh_array_format fmt{};
    int n_beams{0};
    float2 w[BF_MAX][BF_MAX]{};
    hipStream_t stream{nullptr};
    hipEvent_t ev0{nullptr}, ev1{nullptr};
    void* d_raw{nullptr};  // host items of gsh_beam_covariance
    size_t raw_cap{0};
    double2* d_partial{nullptr};  // COV_GRID_CAP x COV_PAIRS partials, then COV_PAIRS sums
    // adaptive mode (gsh_adaptive_beam_set): what the chain of a call works with.  The scratch is the chain's own -- gsh_beam_covariance* keeps d_partial
    // and the handle's stream -- and consecutive chains, on whatever streams, are ordered by chain_done.
    bool adaptive{false};
    bool reset_pending{false};     // the mode was set since the last chain: that chain starts from R_acc = 0 and zero counters
    gsh_beam_adapt conf{};
    double2* d_chain{nullptr};     // as d_partial
    gsh::AwState* d_state{nullptr};
    hipEvent_t chain_done{nullptr};  // recorded behind the beam pass of the latest chain
    bool has_chain{false};
};

namespace
{
size_t item_size(const gsh_beam* b) { return gsh::item_bytes(b->fmt.item_type); }
int n_buffers(const gsh_beam* b) { return b->fmt.layout == GSH_ARRAY_PLANAR ? b->fmt.n_antennas : 1; }

// the input pointers of a call: all there, aligned to the item
int check_items(const gsh_beam* b, const void* const* items, unsigned long long n, bool device)
{
    if (n == 0) return GSH_OK;
    GSH_REQUIRE(items != nullptr, "null items");
    for (int a = 0; a < n_buffers(b); a++)
        {
            GSH_REQUIRE(items[a] != nullptr, "null items (buffer %d)", a);
            if (device)
                GSH_REQUIRE(reinterpret_cast<uintptr_t>(items[a]) % item_size(b) == 0, "buffer %d is not aligned to its %zu-byte items", a, item_size(b));
        }
    return GSH_OK;
}

// kernel arguments for samples [first, first + n) of the call's buffers
BeamArgs make_args(const gsh_beam* b, const void* const* d_items, unsigned long long first, unsigned long long n, int conj)
{
    BeamArgs g{};
    const size_t isz = item_size(b);
    const int A = b->fmt.n_antennas;
    if (b->fmt.layout == GSH_ARRAY_PLANAR)
        for (int a = 0; a < A; a++) g.src[a] = static_cast<const char*>(d_items[a]) + first * isz;
    else
        {
            const size_t frame = isz * A;
            g.src[0] = static_cast<const char*>(d_items[0]) + first * frame;
            g.vec = frame % 16 == 0 && reinterpret_cast<uintptr_t>(g.src[0]) % 16 == 0 ? 1 : 0;
        }
    std::memcpy(g.w, b->w, sizeof(g.w));
    g.n = n;
    g.n_ant = A;
    g.n_beams = b->n_beams;
    g.first_is_q = b->fmt.first_is_q;
    g.qsign = conj ? -1.0f : 1.0f;
    return g;
}

template <int LAYOUT>
void launch_beam_layout(const gsh_beam* b, const BeamArgs& g, unsigned blocks, hipStream_t st, const float2* d_w)
{
    if (d_w != nullptr)
        {
            switch (b->fmt.item_type)
                {
                case GSH_ITEM_GR_COMPLEX:
                    beam_kernel_device_weights<float, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_w);
                    break;
                case GSH_ITEM_SHORT:
                    beam_kernel_device_weights<int16_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_w);
                    break;
                default:
                    beam_kernel_device_weights<int8_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_w);
                    break;
                }
            return;
        }
    switch (b->fmt.item_type)
        {
        case GSH_ITEM_GR_COMPLEX:
            beam_kernel<float, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g);
            break;
        case GSH_ITEM_SHORT:
            beam_kernel<int16_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g);
            break;
        default:
            beam_kernel<int8_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g);
            break;
        }
}

// queue the beams of samples [first, first + n) into dst[0 .. n_beams) on st; d_w: the weights in device memory (adaptive), nullptr: the handle's fixed ones
int launch_beam(const gsh_beam* b, const void* const* d_items, unsigned long long first, unsigned long long n, int conj, float2* const* dst, hipStream_t st,
    const float2* d_w = nullptr)
{
    if (n == 0) return GSH_OK;
    BeamArgs g = make_args(b, d_items, first, n, conj);
    for (int r = 0; r < b->n_beams; r++) g.dst[r] = dst[r];
    const unsigned long long want = (n + BF_THREADS - 1) / BF_THREADS;
    const unsigned blocks = static_cast<unsigned>(want < BF_GRID_CAP ? want : BF_GRID_CAP);
    if (b->fmt.layout == GSH_ARRAY_PLANAR)
        launch_beam_layout<GSH_ARRAY_PLANAR>(b, g, blocks, st, d_w);
    else
        launch_beam_layout<GSH_ARRAY_INTERLEAVED>(b, g, blocks, st, d_w);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

template <int LAYOUT>
void launch_cov_layout(const gsh_beam* b, const BeamArgs& g, unsigned blocks, double2* d_partial, hipStream_t st)
{
    switch (b->fmt.item_type)
        {
        case GSH_ITEM_GR_COMPLEX:
            cov_partial_kernel<float, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_partial);
            break;
        case GSH_ITEM_SHORT:
            cov_partial_kernel<int16_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_partial);
            break;
        default:
            cov_partial_kernel<int8_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, d_partial);
            break;
        }
}

// the arguments of a push, all or nothing
int check_push(const gsh_beam* b, gsh_stream_t* const* rings, const void* const* items, unsigned long long n, bool device)
{
    GSH_REQUIRE(b != nullptr, "null beamformer");
    GSH_REQUIRE(rings != nullptr, "null rings");
    int rc = check_items(b, items, n, device);
    if (rc != GSH_OK) return rc;
    rc = gsh::stream_multi_check_rings(rings, b->n_beams, n);
    if (rc != GSH_OK) return rc;
    for (int r = 0; r < b->n_beams; r++)
        GSH_REQUIRE(rings[r]->device == b->device, "ring %d lies on device %d, the beamformer on device %d", r, rings[r]->device, b->device);
    return gsh::stream_multi_check_live(rings, b->n_beams, n);
}

struct PushCtx
{
    const gsh_beam* b;
    const void* const* d_items;
    int conj;
    const float2* d_w;  // adaptive: the weights the chain's solver leaves in device memory
};

int push_segment(void* ctx, unsigned long long first, unsigned long long len, float2* const* dst, hipStream_t st)
{
    const PushCtx* p = static_cast<const PushCtx*>(ctx);
    return launch_beam(p->b, p->d_items, first, len, p->conj, dst, st, p->d_w);
}

// bytes of one buffer of a call, and the distance between the planar buffers in a staging area (whole 16-byte words)
size_t buffer_bytes(const gsh_beam* b, unsigned long long n) { return static_cast<size_t>(n) * item_size(b) * (b->fmt.layout == GSH_ARRAY_PLANAR ? 1 : b->fmt.n_antennas); }
size_t staging_pitch(const gsh_beam* b, unsigned long long n) { return (buffer_bytes(b, n) + 15) & ~static_cast<size_t>(15); }

// host items -> the staging area d_raw on st, one copy per buffer; d_items: where they went
int stage_items(const gsh_beam* b, const void* const* items, unsigned long long n, void* d_raw, hipStream_t st, const void** d_items)
{
    const size_t bytes = buffer_bytes(b, n), pitch = staging_pitch(b, n);
    for (int a = 0; a < n_buffers(b); a++)
        {
            d_items[a] = static_cast<char*>(d_raw) + a * pitch;
            GSH_HIP(hipMemcpyAsync(const_cast<void*>(d_items[a]), items[a], bytes, hipMemcpyHostToDevice, st));
        }
    return GSH_OK;
}

// queue the block's covariance on st: partials into d_scratch, their sums (the upper triangle, COV_PAIRS entries) behind them
int launch_covariance(const gsh_beam* b, const void* const* d_items, unsigned long long n, int conj, double2* d_scratch, hipStream_t st)
{
    const int A = b->fmt.n_antennas;
    const BeamArgs g = make_args(b, d_items, 0, n, conj);
    const unsigned long long tiles = (n + COV_TILE - 1) / COV_TILE;
    const unsigned blocks = static_cast<unsigned>(tiles < COV_GRID_CAP ? tiles : COV_GRID_CAP);
    if (b->fmt.layout == GSH_ARRAY_PLANAR)
        launch_cov_layout<GSH_ARRAY_PLANAR>(b, g, blocks, d_scratch, st);
    else
        launch_cov_layout<GSH_ARRAY_INTERLEAVED>(b, g, blocks, d_scratch, st);
    GSH_HIP(hipGetLastError());
    cov_final_kernel<<<dim3(1), dim3(64), 0, st>>>(d_scratch, static_cast<int>(blocks), A * (A + 1) / 2, d_scratch + static_cast<size_t>(COV_GRID_CAP) * COV_PAIRS);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

// The head of an adaptive call's chain on st, n >= 1: covariance -> final sums -> accumulate and solve, on the state and scratch given (the handle's, or
// gsh_beam_time_process's copies).  The beam pass that follows reads d_state->w.
int launch_adapt(const gsh_beam* b, const void* const* d_items, unsigned long long n, int conj, gsh::AwState* d_state, double2* d_scratch, bool reset, hipStream_t st)
{
    int rc = launch_covariance(b, d_items, n, conj, d_scratch, st);
    if (rc != GSH_OK) return rc;
    AdaptArgs g{};
    g.conf.forgetting = b->conf.forgetting;
    g.conf.loading_rel = b->conf.loading_rel;
    g.conf.loading_abs = b->conf.loading_abs;
    static_assert(sizeof(g.conf.c) == sizeof(b->conf.constraint_iq), "the constraint vectors of gsh_beam_adapt and gsh::AwConf");
    std::memcpy(g.conf.c, b->conf.constraint_iq, sizeof(g.conf.c));
    for (int r = 0; r < BF_MAX; r++)
        for (int a = 0; a < BF_MAX; a++)
            {
                g.conf.fixed_w[r][a][0] = b->w[r][a].x;
                g.conf.fixed_w[r][a][1] = b->w[r][a].y;
            }
    g.n_ant = b->fmt.n_antennas;
    g.n_beams = b->n_beams;
    g.reset = reset ? 1 : 0;
    adapt_solve_kernel<<<dim3(1), dim3(64), 0, st>>>(g, d_scratch + static_cast<size_t>(COV_GRID_CAP) * COV_PAIRS, d_state);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

// An adaptive call on the handle's own state: st comes behind the previous chain (which may have run on another stream: it wrote the state this one
// reads, and its beam pass read the weights this one rewrites) ...
int chain_begin(gsh_beam* b, const void* const* d_items, unsigned long long n, int conj, hipStream_t st)
{
    if (b->has_chain) GSH_HIP(hipStreamWaitEvent(st, b->chain_done, 0));
    int rc = launch_adapt(b, d_items, n, conj, b->d_state, b->d_chain, b->reset_pending, st);
    if (rc != GSH_OK) return rc;
    b->reset_pending = false;
    return GSH_OK;
}
// ... and the next chain behind this one's beam pass
int chain_end(gsh_beam* b, hipStream_t st)
{
    GSH_HIP(hipEventRecord(b->chain_done, st));
    b->has_chain = true;
    return GSH_OK;
}
const float2* chain_weights(const gsh_beam* b) { return reinterpret_cast<const float2*>(&b->d_state->w[0][0][0]); }

// the device work of a validated push on st.  Adaptive: the solver's chain first -- it touches no ring -- then the frame every push shares, its pieces
// formed with the weights in device memory
int push_chain(gsh_beam* b, gsh_stream_t* const* rings, unsigned long long n, hipStream_t st, PushCtx* ctx)
{
    if (!b->adaptive) return gsh::stream_write_device_multi(rings, b->n_beams, n, st, push_segment, ctx);
    int rc = chain_begin(b, ctx->d_items, n, ctx->conj, st);
    if (rc != GSH_OK) return rc;
    ctx->d_w = chain_weights(b);
    rc = gsh::stream_write_device_multi(rings, b->n_beams, n, st, push_segment, ctx);
    if (rc != GSH_OK) return rc;
    return chain_end(b, st);
}

int covariance_device(gsh_beam* b, const void* const* d_items, unsigned long long n, int conj, double* r_iq)
{
    const int A = b->fmt.n_antennas;
    const int P = A * (A + 1) / 2;
    double2 upper[COV_PAIRS];
    for (int p = 0; p < P; p++) upper[p] = make_double2(0.0, 0.0);
    if (n > 0)
        {
            const int rc = launch_covariance(b, d_items, n, conj, b->d_partial, b->stream);
            if (rc != GSH_OK) return rc;
            const double2* d_sum = b->d_partial + static_cast<size_t>(COV_GRID_CAP) * COV_PAIRS;
            GSH_HIP(hipMemcpyAsync(upper, d_sum, sizeof(double2) * P, hipMemcpyDeviceToHost, b->stream));
            GSH_HIP(hipStreamSynchronize(b->stream));
        }
    int p = 0;
    for (int i = 0; i < A; i++)
        for (int j = i; j < A; j++, p++)
            {
                r_iq[2 * (i * A + j)] = upper[p].x;
                r_iq[2 * (i * A + j) + 1] = upper[p].y;
                if (j != i)  // the lower triangle is the conjugate of the upper
                    {
                        r_iq[2 * (j * A + i)] = upper[p].x;
                        r_iq[2 * (j * A + i) + 1] = -upper[p].y;
                    }
            }
    return GSH_OK;
}
}  // namespace

extern "C"
{
    int gsh_beam_create(int device, const gsh_array_format* fmt, int n_beams, gsh_beam_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null out pointer");
        *out = nullptr;
        GSH_REQUIRE(fmt != nullptr, "null array format");
        GSH_REQUIRE(fmt->n_antennas >= 1 && fmt->n_antennas <= GSH_ARRAY_MAX_ANTENNAS, "%d antennas: an array has 1..%d", fmt->n_antennas, GSH_ARRAY_MAX_ANTENNAS);
        GSH_REQUIRE(n_beams >= 1 && n_beams <= GSH_ARRAY_MAX_BEAMS, "%d beams: a beamformer forms 1..%d", n_beams, GSH_ARRAY_MAX_BEAMS);
        GSH_REQUIRE(gsh::item_bytes(fmt->item_type) != 0, "unknown item type %d", fmt->item_type);
        GSH_REQUIRE(fmt->layout == GSH_ARRAY_PLANAR || fmt->layout == GSH_ARRAY_INTERLEAVED, "unknown array layout %d", fmt->layout);
        GSH_REQUIRE(fmt->first_is_q == 0 || fmt->first_is_q == 1, "first_is_q %d is neither 0 nor 1", fmt->first_is_q);
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_beam* b = new (std::nothrow) gsh_beam();
        GSH_REQUIRE(b != nullptr, "out of host memory");
        b->device = device;
        b->fmt = *fmt;
        b->n_beams = n_beams;
        for (int r = 0; r < BF_MAX; r++)
            for (int a = 0; a < BF_MAX; a++) b->w[r][a] = make_float2(1.0f, 0.0f);  // beamformer.h:52
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_beam_destroy(b);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipEventCreate(&b->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipEventCreate(&b->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipMalloc(&b->d_partial, sizeof(double2) * (static_cast<size_t>(COV_GRID_CAP) + 1) * COV_PAIRS)) != hipSuccess) return fail(e, "hipMalloc(partials)");
        *out = b;
        return GSH_OK;
    }

    void gsh_beam_destroy(gsh_beam_t* b)
    {
        if (!b) return;
        (void)hipSetDevice(b->device);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        if (b->d_raw) (void)hipFree(b->d_raw);
        if (b->d_partial) (void)hipFree(b->d_partial);
        if (b->chain_done) (void)hipEventSynchronize(b->chain_done);  // a chain may have run on a caller's stream
        if (b->d_chain) (void)hipFree(b->d_chain);
        if (b->d_state) (void)hipFree(b->d_state);
        if (b->chain_done) (void)hipEventDestroy(b->chain_done);
        if (b->ev0) (void)hipEventDestroy(b->ev0);
        if (b->ev1) (void)hipEventDestroy(b->ev1);
        if (b->stream) (void)hipStreamDestroy(b->stream);
        delete b;
    }

    int gsh_beam_set_weights(gsh_beam_t* b, const float* w_iq)
    {
        GSH_REQUIRE(b != nullptr && w_iq != nullptr, "null argument");
        const int A = b->fmt.n_antennas;
        for (int r = 0; r < b->n_beams; r++)
            for (int a = 0; a < A; a++) b->w[r][a] = make_float2(w_iq[2 * (r * A + a)], w_iq[2 * (r * A + a) + 1]);
        return GSH_OK;
    }

    int gsh_beam_get_weights(const gsh_beam_t* b, float* w_iq)
    {
        GSH_REQUIRE(b != nullptr && w_iq != nullptr, "null argument");
        const int A = b->fmt.n_antennas;
        for (int r = 0; r < b->n_beams; r++)
            for (int a = 0; a < A; a++)
                {
                    w_iq[2 * (r * A + a)] = b->w[r][a].x;
                    w_iq[2 * (r * A + a) + 1] = b->w[r][a].y;
                }
        return GSH_OK;
    }

    int gsh_beam_process_device(gsh_beam_t* b, const void* const* device_items, uint64_t n, int inverted_spectrum, void* const* device_out, void* hip_stream)
    {
        GSH_REQUIRE(b != nullptr, "null beamformer");
        int rc = check_items(b, device_items, n, true);
        if (rc != GSH_OK) return rc;
        GSH_REQUIRE(n == 0 || device_out != nullptr, "null outputs");
        if (n == 0) return GSH_OK;
        float2* dst[BF_MAX];
        for (int r = 0; r < b->n_beams; r++)
            {
                GSH_REQUIRE(device_out[r] != nullptr, "null output (beam %d)", r);
                GSH_REQUIRE((reinterpret_cast<uintptr_t>(device_out[r]) & 7u) == 0, "output %d must be 8-byte aligned", r);
                dst[r] = static_cast<float2*>(device_out[r]);
            }
        GSH_HIP(hipSetDevice(b->device));
        hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream;
        if (b->adaptive)
            {
                rc = chain_begin(b, device_items, n, inverted_spectrum ? 1 : 0, st);
                if (rc != GSH_OK) return rc;
                rc = launch_beam(b, device_items, 0, n, inverted_spectrum ? 1 : 0, dst, st, chain_weights(b));
                if (rc != GSH_OK) return rc;
                rc = chain_end(b, st);
            }
        else
            rc = launch_beam(b, device_items, 0, n, inverted_spectrum ? 1 : 0, dst, st);
        if (rc != GSH_OK) return rc;
        if (!hip_stream) GSH_HIP(hipStreamSynchronize(st));
        return GSH_OK;
    }

    int gsh_beam_push_device(gsh_beam_t* b, gsh_stream_t* const* rings, const void* const* device_items, uint64_t n, int inverted_spectrum, void* hip_stream,
        uint64_t* first_index)
    {
        int rc = check_push(b, rings, device_items, n, true);
        if (rc != GSH_OK) return rc;
        if (first_index)
            for (int r = 0; r < b->n_beams; r++) first_index[r] = rings[r]->next;
        if (n == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(b->device));
        hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : rings[0]->stream;
        PushCtx ctx{b, device_items, inverted_spectrum ? 1 : 0, nullptr};
        rc = push_chain(b, rings, n, st, &ctx);
        if (rc != GSH_OK) return rc;
        if (!hip_stream) GSH_HIP(hipStreamSynchronize(st));
        return GSH_OK;
    }

    int gsh_beam_push(gsh_beam_t* b, gsh_stream_t* const* rings, const void* const* items, uint64_t n, int inverted_spectrum, uint64_t* first_index)
    {
        // the raw block crosses PCIe once, into the first ring's raw staging buffer (as gsh_stream_push_packed_multi); one pass over it writes every ring
        int rc = check_push(b, rings, items, n, false);
        if (rc != GSH_OK) return rc;
        if (first_index)
            for (int r = 0; r < b->n_beams; r++) first_index[r] = rings[r]->next;
        if (n == 0) return GSH_OK;
        gsh_stream* s = rings[0];
        GSH_HIP(hipSetDevice(b->device));
        rc = gsh::stream_raw_staging(s, staging_pitch(b, n) * n_buffers(b));
        if (rc != GSH_OK) return rc;
        const void* d_items[BF_MAX];
        rc = stage_items(b, items, n, s->d_raw, s->stream, d_items);
        if (rc != GSH_OK) return rc;
        PushCtx ctx{b, d_items, inverted_spectrum ? 1 : 0, nullptr};
        rc = push_chain(b, rings, n, s->stream, &ctx);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipStreamSynchronize(s->stream));
        return GSH_OK;
    }

    int gsh_beam_covariance_device(gsh_beam_t* b, const void* const* device_items, uint64_t n, int inverted_spectrum, double* r_iq)
    {
        GSH_REQUIRE(b != nullptr && r_iq != nullptr, "null argument");
        int rc = check_items(b, device_items, n, true);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(b->device));
        return covariance_device(b, device_items, n, inverted_spectrum ? 1 : 0, r_iq);
    }

    int gsh_beam_covariance(gsh_beam_t* b, const void* const* items, uint64_t n, int inverted_spectrum, double* r_iq)
    {
        GSH_REQUIRE(b != nullptr && r_iq != nullptr, "null argument");
        int rc = check_items(b, items, n, false);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(b->device));
        const void* d_items[BF_MAX] = {};
        if (n > 0)
            {
                const size_t bytes = staging_pitch(b, n) * n_buffers(b);
                if (bytes > b->raw_cap)
                    {
                        if (b->d_raw) GSH_HIP(hipFree(b->d_raw));
                        b->d_raw = nullptr;
                        b->raw_cap = 0;
                        GSH_HIP(hipMalloc(&b->d_raw, bytes));
                        b->raw_cap = bytes;
                    }
                rc = stage_items(b, items, n, b->d_raw, b->stream, d_items);
                if (rc != GSH_OK) return rc;
            }
        return covariance_device(b, d_items, n, inverted_spectrum ? 1 : 0, r_iq);
    }

    int gsh_beam_time_process(gsh_beam_t* b, uint64_t n, int reps, float* avg_ms)
    {
        GSH_REQUIRE(b != nullptr && avg_ms != nullptr, "null argument");
        GSH_REQUIRE(n >= 1 && reps >= 1, "%llu samples x %d", static_cast<unsigned long long>(n), reps);
        GSH_HIP(hipSetDevice(b->device));
        // a zero-filled block of the handle's format and n_beams outputs, released again: the rate of the beam kernel alone
        const size_t in_bytes = staging_pitch(b, n) * n_buffers(b), out_bytes = sizeof(float2) * static_cast<size_t>(n);
        char* d_in = nullptr;
        char* d_out = nullptr;
        int rc = GSH_OK;
        hipError_t e = hipMalloc(&d_in, in_bytes);
        if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes * b->n_beams);
        if (e == hipSuccess) e = hipMemsetAsync(d_in, 0, in_bytes, b->stream);
        // adaptive: the whole chain of a call, on a copy of the state and scratch of its own -- the handle's state stays as it is
        double2* d_scratch = nullptr;
        gsh::AwState* d_state = nullptr;
        bool reset = false;
        if (b->adaptive && e == hipSuccess)
            {
                const size_t scratch_bytes = sizeof(double2) * (static_cast<size_t>(COV_GRID_CAP) + 1) * COV_PAIRS;
                e = hipMalloc(&d_scratch, scratch_bytes + sizeof(gsh::AwState));
                if (e == hipSuccess)
                    {
                        d_state = reinterpret_cast<gsh::AwState*>(reinterpret_cast<char*>(d_scratch) + scratch_bytes);
                        reset = b->reset_pending;
                        if (b->has_chain) e = hipStreamWaitEvent(b->stream, b->chain_done, 0);
                        if (e == hipSuccess) e = hipMemcpyAsync(d_state, b->d_state, sizeof(gsh::AwState), hipMemcpyDeviceToDevice, b->stream);
                    }
            }
        if (e != hipSuccess) rc = gsh::hip_fail(e, "hipMalloc(timing buffers)", __FILE__, __LINE__);
        const void* src[BF_MAX];
        float2* dst[BF_MAX];
        for (int a = 0; a < n_buffers(b); a++) src[a] = d_in + a * staging_pitch(b, n);
        for (int r = 0; r < b->n_beams; r++) dst[r] = reinterpret_cast<float2*>(d_out + r * out_bytes);
        auto pass = [&]() {
            if (d_state == nullptr) return launch_beam(b, src, 0, n, 0, dst, b->stream);
            const int rc_head = launch_adapt(b, src, n, 0, d_state, d_scratch, reset, b->stream);
            reset = false;
            if (rc_head != GSH_OK) return rc_head;
            return launch_beam(b, src, 0, n, 0, dst, b->stream, reinterpret_cast<const float2*>(&d_state->w[0][0][0]));
        };
        float ms = 0.0f;
        for (int i = 0; i < 3 && rc == GSH_OK; i++) rc = pass();  // clocks up
        if (rc == GSH_OK && (e = hipEventRecord(b->ev0, b->stream)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        for (int i = 0; i < reps && rc == GSH_OK; i++) rc = pass();
        if (rc == GSH_OK && (e = hipEventRecord(b->ev1, b->stream)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventSynchronize(b->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventSynchronize", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventElapsedTime(&ms, b->ev0, b->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventElapsedTime", __FILE__, __LINE__);
        (void)hipStreamSynchronize(b->stream);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (d_scratch) (void)hipFree(d_scratch);
        if (rc != GSH_OK) return rc;
        *avg_ms = ms / static_cast<float>(reps);
        return GSH_OK;
    }

    int gsh_adaptive_beam_set(gsh_beam_t* b, const gsh_beam_adapt* conf)
    {
        if (conf != nullptr)  // what can be said of the numbers alone comes first: it needs no handle, let alone a device
            {
                const double scalars[3] = {conf->forgetting, conf->loading_rel, conf->loading_abs};
                for (double v : scalars) GSH_REQUIRE(gsh::aw_finite(v), "forgetting / loading %g is not a finite number", v);
                GSH_REQUIRE(conf->forgetting >= 0.0 && conf->forgetting <= 1.0, "forgetting factor %g lies outside [0, 1]", conf->forgetting);
                GSH_REQUIRE(conf->loading_rel >= 0.0 && conf->loading_abs >= 0.0, "negative loading (%g relative, %g absolute)", conf->loading_rel,
                    conf->loading_abs);
                for (int r = 0; r < BF_MAX; r++)
                    for (int a = 0; a < BF_MAX; a++)
                        GSH_REQUIRE(gsh::aw_finite(conf->constraint_iq[r][a][0]) && gsh::aw_finite(conf->constraint_iq[r][a][1]),
                            "constraint vector of beam %d: element %d is not a finite number", r, a);
            }
        GSH_REQUIRE(b != nullptr, "null beamformer");
        if (conf == nullptr)
            {
                b->adaptive = false;
                return GSH_OK;
            }
        const int A = b->fmt.n_antennas;
        for (int r = 0; r < b->n_beams; r++)
            {
                bool any = false;
                for (int a = 0; a < A; a++) any = any || conf->constraint_iq[r][a][0] != 0.0 || conf->constraint_iq[r][a][1] != 0.0;
                GSH_REQUIRE(any, "the constraint vector of beam %d is all zero", r);
            }
        if (b->d_state == nullptr)
            {
                GSH_HIP(hipSetDevice(b->device));
                if (b->chain_done == nullptr) GSH_HIP(hipEventCreateWithFlags(&b->chain_done, hipEventDisableTiming));
                if (b->d_chain == nullptr) GSH_HIP(hipMalloc(&b->d_chain, sizeof(double2) * (static_cast<size_t>(COV_GRID_CAP) + 1) * COV_PAIRS));
                GSH_HIP(hipMalloc(&b->d_state, sizeof(gsh::AwState)));
            }
        b->conf = gsh_beam_adapt{};
        b->conf.forgetting = conf->forgetting;
        b->conf.loading_rel = conf->loading_rel;
        b->conf.loading_abs = conf->loading_abs;
        for (int r = 0; r < b->n_beams; r++)
            for (int a = 0; a < A; a++)
                for (int q = 0; q < 2; q++) b->conf.constraint_iq[r][a][q] = conf->constraint_iq[r][a][q];
        b->adaptive = true;
        b->reset_pending = true;  // nothing is queued: the next chain takes the state in memory for zero
        return GSH_OK;
    }

    int gsh_adaptive_beam_state(gsh_beam_t* b, struct gsh_beam_adapt_state* out)
    {
        GSH_REQUIRE(b != nullptr && out != nullptr, "null argument");
        if (!b->adaptive) return set_error(GSH_ERR_STATE, "the beamformer is not in adaptive mode (gsh_adaptive_beam_set)");
        const int A = b->fmt.n_antennas;
        std::memset(out, 0, sizeof(*out));
        gsh::AwState s{};
        if (b->reset_pending)  // no call since the mode was set: R_acc = 0, the caller's weights in force
            for (int r = 0; r < b->n_beams; r++)
                for (int a = 0; a < A; a++)
                    {
                        s.w[r][a][0] = b->w[r][a].x;
                        s.w[r][a][1] = b->w[r][a].y;
                    }
        else
            {
                GSH_HIP(hipSetDevice(b->device));
                if (b->has_chain) GSH_HIP(hipEventSynchronize(b->chain_done));
                GSH_HIP(hipMemcpy(&s, b->d_state, sizeof(s), hipMemcpyDeviceToHost));
            }
        out->blocks = s.blocks;
        out->failures = s.failures;
        out->delta = s.delta;
        for (int i = 0; i < A; i++)
            for (int j = i; j < A; j++)
                {
                    const int p = gsh::aw_pair(i, j, A);
                    out->r_acc_iq[2 * (i * A + j)] = s.r_acc[2 * p];
                    out->r_acc_iq[2 * (i * A + j) + 1] = s.r_acc[2 * p + 1];
                    if (j != i)  // the lower triangle is the conjugate of the upper
                        {
                            out->r_acc_iq[2 * (j * A + i)] = s.r_acc[2 * p];
                            out->r_acc_iq[2 * (j * A + i) + 1] = -s.r_acc[2 * p + 1];
                        }
                }
        for (int r = 0; r < b->n_beams; r++)
            for (int a = 0; a < A; a++)
                {
                    out->w_iq[2 * (r * A + a)] = s.w[r][a][0];
                    out->w_iq[2 * (r * A + a) + 1] = s.w[r][a][1];
                }
        return GSH_OK;
    }
}
