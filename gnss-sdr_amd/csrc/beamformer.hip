// gsh_beam_*: the spatial filter of Array_Signal_Conditioner (Beamformer_Filter, src/algorithms/input_filter/gnuradio_blocks/beamformer.{h,cc}) for
// up to 8 antennas and up to 8 beams at once, each beam straight into its own sample ring, and the array covariance the weights are computed from.
// See include/gnss_sdr_hip.h for the contract.  The arithmetic is beamformer.cc:53-61 in float32, one rounding per operation (-ffp-contract=off).
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
void launch_beam_layout(const gsh_beam* b, const BeamArgs& g, unsigned blocks, hipStream_t st)
{
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

// queue the beams of samples [first, first + n) into dst[0 .. n_beams) on st
int launch_beam(const gsh_beam* b, const void* const* d_items, unsigned long long first, unsigned long long n, int conj, float2* const* dst, hipStream_t st)
{
    if (n == 0) return GSH_OK;
    BeamArgs g = make_args(b, d_items, first, n, conj);
    for (int r = 0; r < b->n_beams; r++) g.dst[r] = dst[r];
    const unsigned long long want = (n + BF_THREADS - 1) / BF_THREADS;
    const unsigned blocks = static_cast<unsigned>(want < BF_GRID_CAP ? want : BF_GRID_CAP);
    if (b->fmt.layout == GSH_ARRAY_PLANAR)
        launch_beam_layout<GSH_ARRAY_PLANAR>(b, g, blocks, st);
    else
        launch_beam_layout<GSH_ARRAY_INTERLEAVED>(b, g, blocks, st);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}

template <int LAYOUT>
void launch_cov_layout(const gsh_beam* b, const BeamArgs& g, unsigned blocks, hipStream_t st)
{
    switch (b->fmt.item_type)
        {
        case GSH_ITEM_GR_COMPLEX:
            cov_partial_kernel<float, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, b->d_partial);
            break;
        case GSH_ITEM_SHORT:
            cov_partial_kernel<int16_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, b->d_partial);
            break;
        default:
            cov_partial_kernel<int8_t, LAYOUT><<<dim3(blocks), dim3(BF_THREADS), 0, st>>>(g, b->d_partial);
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
};

int push_segment(void* ctx, unsigned long long first, unsigned long long len, float2* const* dst, hipStream_t st)
{
    const PushCtx* p = static_cast<const PushCtx*>(ctx);
    return launch_beam(p->b, p->d_items, first, len, p->conj, dst, st);
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

int covariance_device(gsh_beam* b, const void* const* d_items, unsigned long long n, int conj, double* r_iq)
{
    const int A = b->fmt.n_antennas;
    const int P = A * (A + 1) / 2;
    double2 upper[COV_PAIRS];
    for (int p = 0; p < P; p++) upper[p] = make_double2(0.0, 0.0);
    if (n > 0)
        {
            const BeamArgs g = make_args(b, d_items, 0, n, conj);
            const unsigned long long tiles = (n + COV_TILE - 1) / COV_TILE;
            const unsigned blocks = static_cast<unsigned>(tiles < COV_GRID_CAP ? tiles : COV_GRID_CAP);
            if (b->fmt.layout == GSH_ARRAY_PLANAR)
                launch_cov_layout<GSH_ARRAY_PLANAR>(b, g, blocks, b->stream);
            else
                launch_cov_layout<GSH_ARRAY_INTERLEAVED>(b, g, blocks, b->stream);
            GSH_HIP(hipGetLastError());
            double2* d_sum = b->d_partial + static_cast<size_t>(COV_GRID_CAP) * COV_PAIRS;
            cov_final_kernel<<<dim3(1), dim3(64), 0, b->stream>>>(b->d_partial, static_cast<int>(blocks), P, d_sum);
            GSH_HIP(hipGetLastError());
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
        PushCtx ctx{b, device_items, inverted_spectrum ? 1 : 0};
        rc = gsh::stream_write_device_multi(rings, b->n_beams, n, st, push_segment, &ctx);
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
        PushCtx ctx{b, d_items, inverted_spectrum ? 1 : 0};
        rc = gsh::stream_write_device_multi(rings, b->n_beams, n, s->stream, push_segment, &ctx);
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
        if (e != hipSuccess) rc = gsh::hip_fail(e, "hipMalloc(timing buffers)", __FILE__, __LINE__);
        const void* src[BF_MAX];
        float2* dst[BF_MAX];
        for (int a = 0; a < n_buffers(b); a++) src[a] = d_in + a * staging_pitch(b, n);
        for (int r = 0; r < b->n_beams; r++) dst[r] = reinterpret_cast<float2*>(d_out + r * out_bytes);
        float ms = 0.0f;
        for (int i = 0; i < 3 && rc == GSH_OK; i++) rc = launch_beam(b, src, 0, n, 0, dst, b->stream);  // clocks up
        if (rc == GSH_OK && (e = hipEventRecord(b->ev0, b->stream)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        for (int i = 0; i < reps && rc == GSH_OK; i++) rc = launch_beam(b, src, 0, n, 0, dst, b->stream);
        if (rc == GSH_OK && (e = hipEventRecord(b->ev1, b->stream)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventSynchronize(b->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventSynchronize", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventElapsedTime(&ms, b->ev0, b->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventElapsedTime", __FILE__, __LINE__);
        (void)hipStreamSynchronize(b->stream);
        if (d_in) (void)hipFree(d_in);
        if (d_out) (void)hipFree(d_out);
        if (rc != GSH_OK) return rc;
        *avg_ms = ms / static_cast<float>(reps);
        return GSH_OK;
    }
}
