// gsh_cond_*: the signal conditioner (Signal_Conditioner, src/algorithms/conditioner/adapters/signal_conditioner.cc:60-87: DataTypeAdapter ->
// InputFilter -> Resampler) as one handle and one call per block, one pass over the raw block straight into a sample ring.  See
// include/gnss_sdr_hip.h for the contract.  This file is the host side: the handle, the integer bookkeeping and the pushes; the kernels are in
// fir_filter.hip (conditioner.h), the ring's wrap, mirror, fences, push event and live words are kept by stream_write_device_multi.
//
// Bookkeeping.  After N input samples the filter has completed M = ceil(N / D) outputs (output m needs inputs up to m D) and the resampler every
// output j whose filter output m(j) is below M:
//     decimation     m(j) = ceil(j 2^32 / step) < M   <=>   j <= floor((M - 1) step / 2^32)
//     interpolation  m(j) = floor((j + 1) step / 2^32) < M   <=>   j + 1 < ceil(M 2^32 / step)
// -- a function of N alone, so the ring's content does not depend on where the stream is cut.  The first output of a push has m(j) >= M of the
// stream before it, so it reaches back K - 1 input samples at most: that is the history the handle keeps (an interpolating resampler that takes
// a filter output twice takes it twice in the same push).
//
// With the blanking stage (gsh_cond_set_blanking; kernels in cond_blanking.hip) the resampler sees whole segments only: M' = floor(M / L) L in place
// of M above.  A push forms every new filter output behind the carry of the open segment (at most L - 1 outputs, kept in device memory,
// double-buffered and ordered by the same event as the history) in the handle's stage buffer, decides the segments these complete on the device, and
// gathers mask ? 0 : stage[m(j) - base] into the ring; the state never comes back to the host.
//
// With the notch stage (gsh_cond_set_notch; kernels in cond_notch.hip) the resampler sees W' = floor((M - 1) / L) L notch outputs in place of M: output
// k is the mitigated filter output k + 1, and a segment is decided once its last sample is there.  The recurrence is chained over chunks of NF_CHUNK
// outputs counted from output 0, so a push keeps, in device memory and double-buffered like the history, the filter outputs from the start of the
// open chunk on, the modes (NotchLite: and coefficients) of the decided segments that overlap it, and in the state the carry in front of it; it
// forms the chunk again from its start and writes the outputs that are new.
#include "conditioner.h"
#include "pulse_blanking.h"
#include "resample_index.h"
#include "sample_convert.h"
#include "sample_stream.h"
#include <cmath>
#include <new>

namespace
{
using gsh::CondArgs;
using gsh::set_error;

constexpr int COND_MAX_TAPS = 1024;  // FIR_MAX_TAPS of fir_filter.hip
constexpr int COND_NSTAGE = 4;       // device staging buffers of the page-locked asynchronous push, in rotation

// a validated gsh_cond_conf, reduced to what the pushes need
struct CondPlan
{
    int kind{0};                // COND_* of conditioner.h
    gsh::PackedCode packed{};
    size_t item_bytes{0};       // bytes per input sample (not packed)
    int conj{0};
    int n_taps{0}, decimation{1};
    double rev_per_sample{0.0};
    unsigned step{0};
    int rs_mode{gsh::COND_RS_NONE};
};

int reduce_conf(const gsh_cond_conf* conf, CondPlan* p)
{
    GSH_REQUIRE(conf != nullptr, "null configuration");
    bool real = false;
    switch (conf->input)
        {
        case GSH_COND_INPUT_ITEMS:
            GSH_REQUIRE(gsh::item_bytes(conf->item_type) != 0, "unknown item type %d", conf->item_type);
            p->kind = conf->item_type == GSH_ITEM_GR_COMPLEX ? gsh::COND_CPX_FLOAT : conf->item_type == GSH_ITEM_SHORT ? gsh::COND_CPX_SHORT : gsh::COND_CPX_BYTE;
            p->item_bytes = gsh::item_bytes(conf->item_type);
            break;
        case GSH_COND_INPUT_REAL:
            GSH_REQUIRE(conf->item_type >= 1 && conf->item_type <= 3, "real item kind %d outside 1..3 (float32, int16, int8)", conf->item_type);
            p->kind = conf->item_type;  // COND_REAL_* are the FIR's input kinds
            p->item_bytes = conf->item_type == 1 ? 4 : conf->item_type == 2 ? 2 : 1;
            real = true;
            break;
        case GSH_COND_INPUT_PACKED:
            {
                int rc = gsh::packed_code(&conf->packed, &p->packed);
                if (rc != GSH_OK) return rc;
                p->kind = gsh::COND_PACKED;
                real = !p->packed.cplx;
                break;
            }
        default:
            return set_error(GSH_ERR_INVALID, "unknown conditioner input %d", conf->input);
        }
    GSH_REQUIRE(!real || conf->n_taps != 0, "real input without a filter: the ring holds complex samples (give the taps of a Freq_Xlating_Fir_Filter / Fir_Filter)");
    GSH_REQUIRE(!real || !conf->inverted_spectrum, "inverted_spectrum on real input: there is no spectrum to mirror before the filter");
    p->conj = conf->inverted_spectrum ? 1 : 0;
    p->n_taps = conf->n_taps;
    p->decimation = 1;
    if (conf->n_taps != 0)
        {
            GSH_REQUIRE(conf->taps != nullptr, "null taps");
            GSH_REQUIRE(conf->n_taps >= 1 && conf->n_taps <= COND_MAX_TAPS, "n_taps %d outside 1..%d", conf->n_taps, COND_MAX_TAPS);
            p->decimation = conf->decimation == 0 ? 1 : conf->decimation;
            GSH_REQUIRE(p->decimation >= 1 && p->decimation <= 64, "decimation %d outside 1..64", conf->decimation);
            GSH_REQUIRE(conf->sampling_freq_hz > 0.0, "sampling frequency must be positive");
            p->rev_per_sample = conf->center_freq_hz / conf->sampling_freq_hz;  // (fir_create)
        }
    else
        GSH_REQUIRE(conf->decimation == 0 || conf->decimation == 1, "decimation %d without a filter", conf->decimation);
    if (conf->fs_in != 0.0 || conf->fs_out != 0.0)
        {
            GSH_REQUIRE(conf->fs_in > 0.0 && conf->fs_out > 0.0, "sample rates must be positive");
            int decimating = 1;
            p->step = gsh::phase_step_of(conf->fs_in, conf->fs_out, &decimating);
            GSH_REQUIRE(p->step != 0u || conf->fs_in == conf->fs_out, "resampling ratio %g too extreme for the 32-bit phase accumulator", conf->fs_out / conf->fs_in);
            p->rs_mode = p->step == 0u ? gsh::COND_RS_NONE : decimating ? gsh::COND_RS_DECIMATE : gsh::COND_RS_INTERPOLATE;  // (a ratio of one copies)
        }
    return GSH_OK;
}

// filter outputs complete once n_in input samples have arrived
unsigned long long filter_outputs_after(const CondPlan& p, unsigned long long n_in)
{
    const unsigned long long D = static_cast<unsigned long long>(p.decimation);
    return (n_in + D - 1) / D;
}

// ring samples produced once n_in input samples have arrived (see the head of the file); length > 0: with the blanking stage, which hands the
// resampler whole segments only; notch_length > 0: with the notch stage, whose segments need one more filter output
unsigned long long outputs_after(const CondPlan& p, unsigned long long n_in, int length = 0, int notch_length = 0)
{
    unsigned long long M = filter_outputs_after(p, n_in);
    if (length > 0) M -= M % static_cast<unsigned long long>(length);
    if (notch_length > 0) M = M == 0 ? 0 : (M - 1) - (M - 1) % static_cast<unsigned long long>(notch_length);
    if (M == 0 || p.rs_mode == gsh::COND_RS_NONE) return M;
    if (p.rs_mode == gsh::COND_RS_DECIMATE) return static_cast<unsigned long long>((static_cast<unsigned __int128>(M - 1) * p.step) >> 32) + 1;
    return static_cast<unsigned long long>(((static_cast<unsigned __int128>(M) << 32) + p.step - 1) / p.step) - 1;
}

// gsh_pb_create's ranges
int check_blanking(const gsh_cond_blanking* b)
{
    GSH_REQUIRE(b->pfa > 0.0f && b->pfa < 1.0f, "pfa %g outside (0, 1)", static_cast<double>(b->pfa));
    GSH_REQUIRE(b->length >= 1 && b->length <= gsh::PB_MAX_LENGTH, "length %d outside 1..%d", b->length, gsh::PB_MAX_LENGTH);
    GSH_REQUIRE(b->n_segments_est >= 0 && b->n_segments_reset >= 0, "negative segment count");
    return GSH_OK;
}

// what a push of n_in samples does to the segments: stage[0] is filter output `base`, the first of the open segment
struct BlankFrame
{
    unsigned long long M0, base, c0;  // filter outputs before the push, the mitigated ones of them, the carry M0 - base
    unsigned long long n_new;         // filter outputs the push completes
    unsigned long long n_seg, c1;     // segments it completes, and the carry it leaves
};

// gsh_notch_create's ranges
int check_notch(const gsh_cond_notch* n)
{
    GSH_REQUIRE(n->pfa > 0.0f && n->pfa < 1.0f, "pfa %g outside (0, 1)", static_cast<double>(n->pfa));
    GSH_REQUIRE(n->length >= 2 && n->length <= 1024, "length %d outside 2..1024", n->length);
    GSH_REQUIRE(n->n_segments_est >= 0 && n->n_segments_reset >= 0 && n->n_segments_coeff >= 0, "negative segment count");
    GSH_REQUIRE(std::isfinite(n->p_c_factor), "p_c_factor is not finite");
    return GSH_OK;
}

constexpr unsigned long long NOTCH_CARRY_MODES = 66;  // decided segments that overlap the open chunk: fewer than NF_CHUNK / length + 1

// what a push of n_in samples does to the notch stage (the names of CondNotchArgs, conditioner.h)
struct NotchFrame
{
    unsigned long long M0, n_new;         // filter outputs before the push, and those it completes
    unsigned long long S0, n_seg;         // segments decided before the push, and those it decides
    unsigned long long W0, W1;            // notch outputs before and after
    unsigned long long c0, y0, seg_base, origin, n_y_in;
    unsigned long long y1, seg_base1, n_y_out;
    unsigned long long n_chunks, n_full;
};
}  // namespace

struct gsh_cond
{
    int device{0};
    CondPlan plan;
    CondArgs base{};                 // what every launch of the handle shares (taps, filter, ratio, tile)
    float* d_taps{nullptr};
    float2* d_hist[2]{nullptr, nullptr};  // the converted history, double-buffered: a push reads [cur] and leaves the new tail in [cur ^ 1]
    int cur{0};
    hipEvent_t hist_ev{nullptr};     // behind the latest push's device work: the next push, on whatever stream, comes after it
    bool hist_recorded{false};
    gsh_stream* ring{nullptr};
    unsigned long long ring_base{0};   // ring index of output 0
    unsigned long long n_in_total{0}, n_out_total{0};
    hipStream_t stream{nullptr};     // gsh_cond_time_push
    hipEvent_t ev0{nullptr}, ev1{nullptr};
    void* d_raw{nullptr};            // staging of gsh_cond_push
    size_t raw_cap{0};
    void* d_stage[COND_NSTAGE]{};    // staging of gsh_cond_push_pinned_async
    size_t stage_cap[COND_NSTAGE]{};
    hipEvent_t stage_done[COND_NSTAGE]{};  // the launch that read d_stage[i] has finished
    int stage_next{0};
    // the blanking stage (gsh_cond_set_blanking)
    bool blank_on{false};
    gsh_cond_blanking blank{};
    float thres{0.0f};
    gsh::CondBlankState* d_bstate{nullptr};   // [0] the state, [1] the copy gsh_cond_time_push writes
    float2* d_carry[2]{nullptr, nullptr};     // the open segment's filter outputs, double-buffered like the history (ordered by hist_ev too)
    int carry_cur{0};
    int stage_tile{0}, stage_span{0};         // cond_tile() of the launch that forms every filter output
    void* d_y{nullptr};                       // stage buffer: the carry, then the push's filter outputs
    size_t y_cap{0};
    void* d_energy{nullptr};
    size_t energy_cap{0};
    void* d_mask{nullptr};
    size_t mask_cap{0};
    // the notch stage (gsh_cond_set_notch); it shares stage_tile / stage_span, d_y and d_energy with the blanking stage: a handle has one of the two
    bool notch_on{false};
    gsh_cond_notch notch{};
    float notch_thres{0.0f};
    gsh::CondNotchState* d_nstate{nullptr};   // [0] the state, [1] the copy gsh_cond_time_push writes
    float2* d_ycarry[2]{nullptr, nullptr};    // filter outputs from the start of the open chunk on; these three double-buffered like the history
    unsigned char* d_mcarry[2]{nullptr, nullptr};  // modes of the decided segments that overlap the open chunk
    float2* d_zcarry[2]{nullptr, nullptr};    // (NotchLite) their coefficients
    int notch_cur{0};
    void* d_floor{nullptr};
    size_t floor_cap{0};
    void* d_mode{nullptr};
    size_t mode_cap{0};
    void* d_z0{nullptr};
    size_t z0_cap{0};
    void* d_comp{nullptr};
    size_t comp_cap{0};
    void* d_w{nullptr};                       // the notch outputs a push adds
    size_t w_cap{0};
};

namespace
{
// bytes of a block of n_in samples; GSH_ERR_INVALID for a partial packed item
int block_bytes(const gsh_cond* h, unsigned long long n_in, unsigned long long* bytes)
{
    if (h->plan.kind == gsh::COND_PACKED) return gsh::packed_size(h->plan.packed, n_in, bytes);
    *bytes = n_in * h->plan.item_bytes;
    return GSH_OK;
}

// ring samples the handle's chain, with its stage, has produced once n_in_total input samples have arrived
unsigned long long outputs_total(const gsh_cond* h, unsigned long long n_in_total)
{
    return outputs_after(h->plan, n_in_total, h->blank_on ? h->blank.length : 0, h->notch_on ? h->notch.length : 0);
}

// a stage's buffer of filter outputs is indexed with 32 bits
int check_stage_span(const gsh_cond* h, unsigned long long n_in)
{
    if (h->blank_on)
        GSH_REQUIRE(filter_outputs_after(h->plan, n_in) + static_cast<unsigned long long>(h->blank.length) < (1ull << 32), "more than 2^32 filter outputs in one push");
    if (h->notch_on)
        GSH_REQUIRE(filter_outputs_after(h->plan, n_in) + 2ull * static_cast<unsigned long long>(h->notch.length) + gsh::NF_CHUNK < (1ull << 32),
            "more than 2^32 filter outputs in one push");
    return GSH_OK;
}

// the arguments of a push, all or nothing: *count = ring samples it completes
int check_push(const gsh_cond* h, const void* items, unsigned long long n_in, unsigned long long* bytes, unsigned long long* count)
{
    GSH_REQUIRE(h != nullptr, "null conditioner");
    GSH_REQUIRE(n_in == 0 || items != nullptr, "null items");
    GSH_REQUIRE(h->ring != nullptr, "no ring bound (gsh_cond_bind)");
    int rc = block_bytes(h, n_in, bytes);
    if (rc != GSH_OK) return rc;
    *count = outputs_total(h, h->n_in_total + n_in) - h->n_out_total;
    rc = check_stage_span(h, n_in);
    if (rc != GSH_OK) return rc;
    gsh_stream* ring = h->ring;
    rc = gsh::stream_multi_check_rings(&ring, 1, *count);
    if (rc != GSH_OK) return rc;
    GSH_REQUIRE(*count < (1ull << 32), "more than 2^32 outputs in one push");  // (the launch's index arithmetic, as gsh_direct_resample_device)
    if (ring->next != h->ring_base + h->n_out_total)
        return set_error(GSH_ERR_STATE, "the ring's next index is %llu, the conditioner left it at %llu: someone else pushed or sought", ring->next,
            h->ring_base + h->n_out_total);
    return gsh::stream_multi_check_live(&ring, 1, *count);
}

// the launch arguments of a block at d_block from the handle's present state
CondArgs block_args(const gsh_cond* h, const void* d_block, unsigned long long n_in)
{
    CondArgs a = h->base;
    a.in = d_block;
    a.hist = h->d_hist[h->cur];
    a.hist_out = h->d_hist[h->cur ^ 1];
    a.in0 = h->n_in_total;
    a.n_in = n_in;
    return a;
}

// what the segments of a push share; a push with a stage adds what its gather needs (BlankSegmentCtx, NotchSegmentCtx) and launches that instead
struct SegmentCtx
{
    CondArgs a;                      // of the whole push
    unsigned long long out0;         // absolute output index of the push's first ring sample
    int launch(const CondArgs& seg, hipStream_t st) const { return gsh::cond_launch(seg, st); }
};

// MultiSegmentWriter: ring samples [first, first + len) of the push into dst[0], by the launcher of the push's context
template <class Ctx>
int write_segment(void* ctx, unsigned long long first, unsigned long long len, float2* const* dst, hipStream_t st)
{
    const Ctx* c = static_cast<const Ctx*>(ctx);
    CondArgs a = c->a;
    a.out = dst[0];
    a.out0 = c->out0 + first;
    a.n_out = len;
    gsh::cond_plan_resampler(&a);
    return c->launch(a, st);
}

int grow(void** buf, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return GSH_OK;
    if (*buf) GSH_HIP(hipFree(*buf));  // (hipFree waits for the device: nothing still reads the old buffer)
    *buf = nullptr;
    *cap = 0;
    GSH_HIP(hipMalloc(buf, bytes + bytes / 2));
    *cap = bytes + bytes / 2;
    return GSH_OK;
}

BlankFrame blank_frame(const gsh_cond* h, unsigned long long n_in)
{
    const unsigned long long L = static_cast<unsigned long long>(h->blank.length);
    BlankFrame f;
    f.M0 = filter_outputs_after(h->plan, h->n_in_total);
    const unsigned long long M1 = filter_outputs_after(h->plan, h->n_in_total + n_in);
    f.base = f.M0 - f.M0 % L;
    f.c0 = f.M0 - f.base;
    f.n_new = M1 - f.M0;
    f.n_seg = (M1 - f.base) / L;
    f.c1 = M1 - f.base - f.n_seg * L;
    return f;
}

// the handle's buffers for a frame, before anything is queued
int blank_reserve(gsh_cond* h, const BlankFrame& f)
{
    int rc = grow(&h->d_y, &h->y_cap, sizeof(float2) * (f.c0 + f.n_new));
    if (rc == GSH_OK) rc = grow(&h->d_energy, &h->energy_cap, sizeof(float) * f.n_seg);
    if (rc == GSH_OK) rc = grow(&h->d_mask, &h->mask_cap, f.n_seg);
    return rc;
}

// queue the carry, the push's filter outputs behind it, the energies and the decision of the segments they complete, and the carry the push leaves
// in the other half; *b = what the gather needs
int blank_stage(const gsh_cond* h, const CondArgs& block, const BlankFrame& f, gsh::CondBlankState* state_out, hipStream_t st, gsh::CondBlankArgs* b)
{
    float2* y = static_cast<float2*>(h->d_y);
    if (f.c0 > 0) GSH_HIP(hipMemcpyAsync(y, h->d_carry[h->carry_cur], sizeof(float2) * f.c0, hipMemcpyDeviceToDevice, st));
    if (f.n_new > 0)
        {
            CondArgs a = block;  // every filter output: the chain's launch without its resampler
            a.rs_mode = gsh::COND_RS_NONE;
            a.step = 0u;
            a.q0 = a.r0 = 0;
            a.tile = h->stage_tile;
            a.max_span = h->stage_span;
            a.out = y + f.c0;
            a.out0 = f.M0;
            a.n_out = f.n_new;
            int rc = gsh::cond_launch(a, st);
            if (rc != GSH_OK) return rc;
        }
    b->stage = y;
    b->energy = static_cast<float*>(h->d_energy);
    b->mask = static_cast<unsigned char*>(h->d_mask);
    b->state_in = h->d_bstate;
    b->state_out = state_out;
    b->base = f.base;
    b->n_seg = f.n_seg;
    b->length = h->blank.length;
    b->n_segments_est = h->blank.n_segments_est;
    b->n_segments_reset = h->blank.n_segments_reset;
    b->thres = h->thres;
    if (f.n_seg > 0)
        {
            int rc = gsh::cond_blank_launch_decide(*b, st);
            if (rc != GSH_OK) return rc;
        }
    if (f.c1 > 0)
        GSH_HIP(hipMemcpyAsync(h->d_carry[h->carry_cur ^ 1], y + f.n_seg * static_cast<unsigned long long>(h->blank.length), sizeof(float2) * f.c1,
            hipMemcpyDeviceToDevice, st));
    return GSH_OK;
}

// SegmentCtx of a push with the blanking stage
struct BlankSegmentCtx
{
    CondArgs a;
    unsigned long long out0;
    gsh::CondBlankArgs b;
    int launch(const CondArgs& seg, hipStream_t st) const { return gsh::cond_blank_launch_gather(seg, b, st); }
};

NotchFrame notch_frame(const gsh_cond* h, unsigned long long n_in)
{
    const unsigned long long L = static_cast<unsigned long long>(h->notch.length), C = gsh::NF_CHUNK;
    NotchFrame f;
    f.M0 = filter_outputs_after(h->plan, h->n_in_total);
    const unsigned long long M1 = filter_outputs_after(h->plan, h->n_in_total + n_in);
    f.n_new = M1 - f.M0;
    f.S0 = f.M0 == 0 ? 0 : (f.M0 - 1) / L;
    const unsigned long long S1 = M1 == 0 ? 0 : (M1 - 1) / L;
    f.n_seg = S1 - f.S0;
    f.W0 = f.S0 * L;
    f.W1 = S1 * L;
    f.c0 = f.W0 / C;
    f.y0 = f.c0 * C;
    f.seg_base = f.y0 / L;
    f.origin = f.seg_base * L;
    f.n_y_in = f.M0 - f.y0;          // (M0 > W0 >= y0 once there is a filter output; 0 - 0 before)
    const unsigned long long c1 = f.W1 / C;
    f.y1 = c1 * C;
    f.seg_base1 = f.y1 / L;
    f.n_y_out = M1 - f.y1;           // at most NF_CHUNK - 1 + length: M1 <= W1 + length, W1 - y1 < NF_CHUNK
    f.n_full = c1 - f.c0;
    f.n_chunks = (f.W1 + C - 1) / C - f.c0;
    return f;
}

// the handle's buffers for a frame, before anything is queued
int notch_reserve(gsh_cond* h, const NotchFrame& f)
{
    const unsigned long long n_modes = f.S0 - f.seg_base + f.n_seg;
    int rc = grow(&h->d_y, &h->y_cap, sizeof(float2) * (f.y0 - f.origin + f.n_y_in + f.n_new));
    if (rc == GSH_OK) rc = grow(&h->d_energy, &h->energy_cap, sizeof(float) * f.n_seg);
    if (rc == GSH_OK) rc = grow(&h->d_floor, &h->floor_cap, sizeof(float) * f.n_seg);
    if (rc == GSH_OK) rc = grow(&h->d_mode, &h->mode_cap, n_modes);
    if (rc == GSH_OK) rc = grow(&h->d_z0, &h->z0_cap, sizeof(float2) * n_modes);
    if (rc == GSH_OK) rc = grow(&h->d_comp, &h->comp_cap, sizeof(float2) * 2 * f.n_chunks);
    if (rc == GSH_OK) rc = grow(&h->d_w, &h->w_cap, sizeof(float2) * (f.W1 - f.W0));
    return rc;
}

// queue the carried filter outputs, the push's filter outputs behind them, the stage's launches over the segments they complete, and what the push
// leaves for the next one in the other halves; *n = what the gather needs
int notch_stage(const gsh_cond* h, const CondArgs& block, const NotchFrame& f, gsh::CondNotchState* state_out, hipStream_t st, gsh::CondNotchArgs* n)
{
    const int in = h->notch_cur, out = h->notch_cur ^ 1;
    n->x = static_cast<float2*>(h->d_y);
    n->energy = static_cast<float*>(h->d_energy);
    n->floor_lin = static_cast<float*>(h->d_floor);
    n->mode = static_cast<unsigned char*>(h->d_mode);
    n->z0_seg = static_cast<float2*>(h->d_z0);
    n->comp = static_cast<float2*>(h->d_comp);
    n->w = static_cast<float2*>(h->d_w);
    n->y_in = h->d_ycarry[in];
    n->mode_in = h->d_mcarry[in];
    n->z0_in = h->d_zcarry[in];
    n->y_out = h->d_ycarry[out];
    n->mode_out = h->d_mcarry[out];
    n->z0_out = h->d_zcarry[out];
    n->state_in = h->d_nstate;
    n->state_out = state_out;
    n->origin = f.origin;
    n->seg_base = f.seg_base;
    n->y0 = f.y0;
    n->n_y_in = f.n_y_in;
    n->y1 = f.y1;
    n->n_y_out = f.n_y_out;
    n->seg_base1 = f.seg_base1;
    n->S0 = f.S0;
    n->n_seg = f.n_seg;
    n->W0 = f.W0;
    n->W1 = f.W1;
    n->c0 = f.c0;
    n->n_chunks = f.n_chunks;
    n->n_full = f.n_full;
    n->length = h->notch.length;
    n->n_segments_est = h->notch.n_segments_est;
    n->n_segments_reset = h->notch.n_segments_reset;
    n->n_segments_coeff = h->notch.n_segments_coeff;
    n->thres = h->notch_thres;
    n->p_c_factor = h->notch.p_c_factor;
    int rc = gsh::cond_notch_launch_load(*n, st);
    if (rc != GSH_OK) return rc;
    if (f.n_new > 0)
        {
            CondArgs a = block;  // every filter output: the chain's launch without its resampler
            a.rs_mode = gsh::COND_RS_NONE;
            a.step = 0u;
            a.q0 = a.r0 = 0;
            a.tile = h->stage_tile;
            a.max_span = h->stage_span;
            a.out = n->x + (f.M0 - f.origin);
            a.out0 = f.M0;
            a.n_out = f.n_new;
            rc = gsh::cond_launch(a, st);
            if (rc != GSH_OK) return rc;
        }
    if (f.n_seg > 0)
        {
            rc = gsh::cond_notch_launch_filter(*n, st);
            if (rc != GSH_OK) return rc;
        }
    return gsh::cond_notch_launch_save(*n, st);
}

// SegmentCtx of a push with the notch stage
struct NotchSegmentCtx
{
    CondArgs a;
    unsigned long long out0;
    gsh::CondNotchArgs n;
    int launch(const CondArgs& seg, hipStream_t st) const { return gsh::cond_notch_launch_gather(seg, n, st); }
};

// What every push shares, around its stage's own launches.  Before anything is queued: st comes behind the latest push's device work, which wrote the
// history (and the stage's carry) this one reads ...
int await_history(const gsh_cond* h, hipStream_t st)
{
    if (h->hist_recorded) GSH_HIP(hipStreamWaitEvent(st, h->hist_ev, 0));
    return GSH_OK;
}

// ... and behind the stage: the push's ring samples by its context's launcher, the new history tail into the other half, the event the next push
// waits for, the totals
template <class Ctx>
int write_and_advance(gsh_cond* h, Ctx& ctx, unsigned long long n_in, unsigned long long count, hipStream_t st)
{
    if (count > 0)
        {
            int rc = gsh::stream_write_device_multi(&h->ring, 1, count, st, write_segment<Ctx>, &ctx);
            if (rc != GSH_OK) return rc;
        }
    if (n_in > 0)
        {
            if (h->plan.n_taps > 1)
                {
                    int rc = gsh::cond_launch_history(ctx.a, st);
                    if (rc != GSH_OK) return rc;
                    h->cur ^= 1;
                }
            GSH_HIP(hipEventRecord(h->hist_ev, st));
            h->hist_recorded = true;
        }
    h->n_in_total += n_in;
    h->n_out_total += count;
    return GSH_OK;
}

int push_block_blanked(gsh_cond* h, const void* d_block, unsigned long long n_in, unsigned long long count, hipStream_t st)
{
    const BlankFrame f = blank_frame(h, n_in);
    int rc = blank_reserve(h, f);
    if (rc == GSH_OK) rc = await_history(h, st);
    if (rc != GSH_OK) return rc;
    BlankSegmentCtx ctx{block_args(h, d_block, n_in), h->n_out_total, {}};
    rc = blank_stage(h, ctx.a, f, h->d_bstate, st, &ctx.b);
    if (rc == GSH_OK) rc = write_and_advance(h, ctx, n_in, count, st);
    if (rc != GSH_OK) return rc;
    if (f.c1 > 0) h->carry_cur ^= 1;
    return GSH_OK;
}

int push_block_notched(gsh_cond* h, const void* d_block, unsigned long long n_in, unsigned long long count, hipStream_t st)
{
    const NotchFrame f = notch_frame(h, n_in);
    int rc = notch_reserve(h, f);
    if (rc == GSH_OK) rc = await_history(h, st);
    if (rc != GSH_OK) return rc;
    NotchSegmentCtx ctx{block_args(h, d_block, n_in), h->n_out_total, {}};
    rc = notch_stage(h, ctx.a, f, h->d_nstate, st, &ctx.n);
    if (rc == GSH_OK) rc = write_and_advance(h, ctx, n_in, count, st);
    if (rc != GSH_OK) return rc;
    h->notch_cur ^= 1;  // (the save wrote the other halves, an unchanged carry included)
    return GSH_OK;
}

// queue the device work of a checked push on st and advance the handle
int push_block(gsh_cond* h, const void* d_block, unsigned long long n_in, unsigned long long count, hipStream_t st)
{
    if (h->blank_on) return push_block_blanked(h, d_block, n_in, count, st);
    if (h->notch_on) return push_block_notched(h, d_block, n_in, count, st);
    int rc = await_history(h, st);
    if (rc != GSH_OK) return rc;
    SegmentCtx ctx{block_args(h, d_block, n_in), h->n_out_total};
    return write_and_advance(h, ctx, n_in, count, st);
}

void report(const gsh_cond* h, unsigned long long count, uint64_t* first_out, uint64_t* n_out)
{
    if (first_out) *first_out = h->ring_base + h->n_out_total;
    if (n_out) *n_out = count;
}
}  // namespace

extern "C"
{
    int gsh_cond_plan(const gsh_cond_conf* conf, uint64_t n_in_total, uint64_t* n_out_total)
    {
        GSH_REQUIRE(n_out_total != nullptr, "null n_out_total");
        *n_out_total = 0;
        CondPlan p;
        int rc = reduce_conf(conf, &p);
        if (rc != GSH_OK) return rc;
        *n_out_total = outputs_after(p, n_in_total);
        return GSH_OK;
    }

    int gsh_cond_plan_blanked(const gsh_cond_conf* conf, const gsh_cond_blanking* blanking, uint64_t n_in_total, uint64_t* n_out_total)
    {
        if (blanking == nullptr) return gsh_cond_plan(conf, n_in_total, n_out_total);
        GSH_REQUIRE(n_out_total != nullptr, "null n_out_total");
        *n_out_total = 0;
        CondPlan p;
        int rc = reduce_conf(conf, &p);
        if (rc == GSH_OK) rc = check_blanking(blanking);
        if (rc != GSH_OK) return rc;
        *n_out_total = outputs_after(p, n_in_total, blanking->length);
        return GSH_OK;
    }

    int gsh_cond_set_blanking(gsh_cond_t* h, const gsh_cond_blanking* blanking)
    {
        GSH_REQUIRE(h != nullptr, "null conditioner");
        if (h->n_in_total != 0 || h->hist_recorded) return set_error(GSH_ERR_STATE, "the blanking stage is set before the handle's first push (%llu samples taken)", h->n_in_total);
        if (blanking == nullptr)
            {
                h->blank_on = false;
                return GSH_OK;
            }
        int rc = check_blanking(blanking);
        if (rc != GSH_OK) return rc;
        if (h->notch_on) return set_error(GSH_ERR_STATE, "the conditioner has a notch stage: one mitigation stage per handle (gsh_cond_set_notch(h, NULL) turns it off)");
        GSH_HIP(hipSetDevice(h->device));
        h->blank_on = false;
        if (h->d_bstate == nullptr) GSH_HIP(hipMalloc(&h->d_bstate, 2 * sizeof(gsh::CondBlankState)));
        GSH_HIP(hipMemset(h->d_bstate, 0, 2 * sizeof(gsh::CondBlankState)));  // pulse_blanking_cc.cc:38-44
        if (h->d_carry[0]) GSH_HIP(hipFree(h->d_carry[0]));
        h->d_carry[0] = h->d_carry[1] = nullptr;
        GSH_HIP(hipMalloc(&h->d_carry[0], sizeof(float2) * 2 * static_cast<size_t>(blanking->length)));
        h->d_carry[1] = h->d_carry[0] + blanking->length;
        h->carry_cur = 0;
        CondArgs a = h->base;
        a.rs_mode = gsh::COND_RS_NONE;
        gsh::cond_tile(&a);
        h->stage_tile = a.tile;
        h->stage_span = a.max_span;
        h->blank = *blanking;
        h->thres = gsh::pb_threshold(blanking->pfa, blanking->length);
        h->blank_on = true;
        return GSH_OK;
    }

    int gsh_cond_blanking_state(gsh_cond_t* h, struct gsh_cond_blanking_state* state)
    {
        GSH_REQUIRE(h != nullptr && state != nullptr, "null argument");
        if (!h->blank_on) return set_error(GSH_ERR_STATE, "the conditioner has no blanking stage (gsh_cond_set_blanking)");
        GSH_HIP(hipSetDevice(h->device));
        if (h->hist_recorded) GSH_HIP(hipEventSynchronize(h->hist_ev));
        gsh::CondBlankState s{};
        GSH_HIP(hipMemcpy(&s, h->d_bstate, sizeof(s), hipMemcpyDeviceToHost));
        state->thres = h->thres;
        state->noise_power_estimation = s.noise_power_estimation;
        state->n_segments = s.n_segments;
        state->last_filtered = s.last_filtered;
        state->n_decided = s.n_decided;
        state->n_blanked = s.n_blanked;
        return GSH_OK;
    }

    int gsh_cond_plan_notched(const gsh_cond_conf* conf, const gsh_cond_notch* notch, uint64_t n_in_total, uint64_t* n_out_total)
    {
        if (notch == nullptr) return gsh_cond_plan(conf, n_in_total, n_out_total);
        GSH_REQUIRE(n_out_total != nullptr, "null n_out_total");
        *n_out_total = 0;
        CondPlan p;
        int rc = reduce_conf(conf, &p);
        if (rc == GSH_OK) rc = check_notch(notch);
        if (rc != GSH_OK) return rc;
        *n_out_total = outputs_after(p, n_in_total, 0, notch->length);
        return GSH_OK;
    }

    int gsh_cond_set_notch(gsh_cond_t* h, const gsh_cond_notch* notch)
    {
        GSH_REQUIRE(h != nullptr, "null conditioner");
        if (h->n_in_total != 0 || h->hist_recorded) return set_error(GSH_ERR_STATE, "the notch stage is set before the handle's first push (%llu samples taken)", h->n_in_total);
        if (notch == nullptr)
            {
                h->notch_on = false;
                return GSH_OK;
            }
        int rc = check_notch(notch);
        if (rc != GSH_OK) return rc;
        if (h->blank_on) return set_error(GSH_ERR_STATE, "the conditioner has a blanking stage: one mitigation stage per handle (gsh_cond_set_blanking(h, NULL) turns it off)");
        GSH_HIP(hipSetDevice(h->device));
        h->notch_on = false;
        if (h->d_nstate == nullptr) GSH_HIP(hipMalloc(&h->d_nstate, 2 * sizeof(gsh::CondNotchState)));
        GSH_HIP(hipMemset(h->d_nstate, 0, 2 * sizeof(gsh::CondNotchState)));  // notch_cc.cc:41-51; the recurrence starts from 0
        if (h->d_ycarry[0]) GSH_HIP(hipFree(h->d_ycarry[0]));
        h->d_ycarry[0] = h->d_ycarry[1] = nullptr;
        const size_t n_y = static_cast<size_t>(gsh::NF_CHUNK) + static_cast<size_t>(notch->length) + 1;  // NotchFrame::n_y_out at most
        GSH_HIP(hipMalloc(&h->d_ycarry[0], sizeof(float2) * 2 * n_y));
        h->d_ycarry[1] = h->d_ycarry[0] + n_y;
        if (h->d_zcarry[0] == nullptr)
            {
                GSH_HIP(hipMalloc(&h->d_zcarry[0], (sizeof(float2) + 1) * 2 * NOTCH_CARRY_MODES));
                h->d_zcarry[1] = h->d_zcarry[0] + NOTCH_CARRY_MODES;
                h->d_mcarry[0] = reinterpret_cast<unsigned char*>(h->d_zcarry[1] + NOTCH_CARRY_MODES);
                h->d_mcarry[1] = h->d_mcarry[0] + NOTCH_CARRY_MODES;
            }
        h->notch_cur = 0;
        CondArgs a = h->base;
        a.rs_mode = gsh::COND_RS_NONE;
        gsh::cond_tile(&a);
        h->stage_tile = a.tile;
        h->stage_span = a.max_span;
        h->notch = *notch;
        h->notch_thres = gsh::nf_threshold(notch->pfa, notch->length);
        h->notch_on = true;
        return GSH_OK;
    }

    int gsh_cond_notch_state(gsh_cond_t* h, struct gsh_cond_notch_state* state)
    {
        GSH_REQUIRE(h != nullptr && state != nullptr, "null argument");
        if (!h->notch_on) return set_error(GSH_ERR_STATE, "the conditioner has no notch stage (gsh_cond_set_notch)");
        GSH_HIP(hipSetDevice(h->device));
        if (h->hist_recorded) GSH_HIP(hipEventSynchronize(h->hist_ev));
        gsh::CondNotchState s{};
        GSH_HIP(hipMemcpy(&s, h->d_nstate, sizeof(s), hipMemcpyDeviceToHost));
        const bool lite = h->notch.n_segments_coeff > 0;
        state->thres = h->notch_thres;
        state->noise_pow_est = s.s.noise_pow_est;
        state->n_segments = s.s.n_segments;
        state->filter_state = s.s.filter_state;
        state->n_segments_coeff = s.s.n_segments_coeff;
        state->reserved = 0;
        state->z0[0] = lite ? s.s.z0.x : 0.0f;
        state->z0[1] = lite ? s.s.z0.y : 0.0f;
        state->n_decided = s.n_decided;
        state->n_filtered = s.n_filtered;
        return GSH_OK;
    }

    int gsh_cond_create(int device, const gsh_cond_conf* conf, gsh_cond_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null out pointer");
        *out = nullptr;
        CondPlan p;
        int rc = reduce_conf(conf, &p);
        if (rc != GSH_OK) return rc;
        rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_cond* h = new (std::nothrow) gsh_cond();
        GSH_REQUIRE(h != nullptr, "out of host memory");
        h->device = device;
        h->plan = p;
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_cond_destroy(h);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&h->hist_ev, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
        if (p.n_taps > 0)
            {
                if ((e = hipMalloc(&h->d_taps, sizeof(float) * p.n_taps)) != hipSuccess) return fail(e, "hipMalloc(taps)");
                if ((e = hipMemcpy(h->d_taps, conf->taps, sizeof(float) * p.n_taps, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy(taps)");
                // a fresh stream has zero history (a fresh GNU Radio buffer, fir_filter.hip)
                if ((e = hipMalloc(&h->d_hist[0], sizeof(float2) * 2 * static_cast<size_t>(p.n_taps))) != hipSuccess) return fail(e, "hipMalloc(hist)");
                if ((e = hipMemset(h->d_hist[0], 0, sizeof(float2) * 2 * static_cast<size_t>(p.n_taps))) != hipSuccess) return fail(e, "hipMemset(hist)");
                h->d_hist[1] = h->d_hist[0] + p.n_taps;
            }
        CondArgs& a = h->base;
        a.taps = h->d_taps;
        a.rev_per_sample = p.rev_per_sample;
        a.step = p.step;
        a.rs_mode = p.rs_mode;
        a.n_taps = p.n_taps;
        a.decimation = p.decimation;
        a.kind = p.kind;
        a.conj = p.conj;
        a.packed = p.packed;
        gsh::cond_tile(&a);
        *out = h;
        return GSH_OK;
    }

    void gsh_cond_destroy(gsh_cond_t* h)
    {
        if (!h) return;
        (void)hipSetDevice(h->device);
        if (h->hist_recorded) (void)hipEventSynchronize(h->hist_ev);  // the latest push's device work, on the ring's or the caller's stream, and all before it
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (h->d_taps) (void)hipFree(h->d_taps);
        if (h->d_hist[0]) (void)hipFree(h->d_hist[0]);
        if (h->d_raw) (void)hipFree(h->d_raw);
        if (h->d_bstate) (void)hipFree(h->d_bstate);
        if (h->d_carry[0]) (void)hipFree(h->d_carry[0]);
        if (h->d_y) (void)hipFree(h->d_y);
        if (h->d_energy) (void)hipFree(h->d_energy);
        if (h->d_mask) (void)hipFree(h->d_mask);
        if (h->d_nstate) (void)hipFree(h->d_nstate);
        if (h->d_ycarry[0]) (void)hipFree(h->d_ycarry[0]);
        if (h->d_zcarry[0]) (void)hipFree(h->d_zcarry[0]);  // (the carried modes lie behind the coefficients)
        for (void* q : {h->d_floor, h->d_mode, h->d_z0, h->d_comp, h->d_w})
            if (q) (void)hipFree(q);
        for (int i = 0; i < COND_NSTAGE; i++)
            {
                if (h->d_stage[i]) (void)hipFree(h->d_stage[i]);
                if (h->stage_done[i]) (void)hipEventDestroy(h->stage_done[i]);
            }
        if (h->hist_ev) (void)hipEventDestroy(h->hist_ev);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
    }

    int gsh_cond_bind(gsh_cond_t* h, gsh_stream_t* ring)
    {
        GSH_REQUIRE(h != nullptr, "null conditioner");
        GSH_REQUIRE(ring == nullptr || ring->device == h->device, "the ring lies on device %d, the conditioner on device %d", ring ? ring->device : 0, h->device);
        h->ring = ring;
        // output n_out_total, the next one, goes to the ring's next index
        h->ring_base = ring ? ring->next - h->n_out_total : 0ull;
        return GSH_OK;
    }

    int gsh_cond_position(const gsh_cond_t* h, uint64_t* n_in_total, uint64_t* n_out_total)
    {
        GSH_REQUIRE(h != nullptr, "null conditioner");
        if (n_in_total) *n_in_total = h->n_in_total;
        if (n_out_total) *n_out_total = h->n_out_total;
        return GSH_OK;
    }

    int gsh_cond_push_device(gsh_cond_t* h, const void* device_items, uint64_t n_in, void* hip_stream, uint64_t* first_out, uint64_t* n_out)
    {
        unsigned long long bytes = 0, count = 0;
        int rc = check_push(h, device_items, n_in, &bytes, &count);
        if (rc != GSH_OK) return rc;
        const size_t align = h->plan.kind == gsh::COND_PACKED ? gsh::packed_alignment(h->plan.packed) : h->plan.item_bytes;
        GSH_REQUIRE(n_in == 0 || reinterpret_cast<uintptr_t>(device_items) % align == 0, "the block must be aligned to its item (%zu bytes)", align);
        report(h, count, first_out, n_out);
        if (n_in == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(h->device));
        hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->ring->stream;
        rc = push_block(h, device_items, n_in, count, st);
        if (rc != GSH_OK) return rc;
        if (!hip_stream) GSH_HIP(hipStreamSynchronize(st));
        return GSH_OK;
    }

    int gsh_cond_push(gsh_cond_t* h, const void* items, uint64_t n_in, uint64_t* first_out, uint64_t* n_out)
    {
        // the raw block crosses PCIe once, into the handle's staging buffer; one pass over it writes the ring
        unsigned long long bytes = 0, count = 0;
        int rc = check_push(h, items, n_in, &bytes, &count);
        if (rc != GSH_OK) return rc;
        report(h, count, first_out, n_out);
        if (n_in == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(h->device));
        hipStream_t st = h->ring->stream;
        rc = grow(&h->d_raw, &h->raw_cap, bytes);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipMemcpyAsync(h->d_raw, items, bytes, hipMemcpyHostToDevice, st));
        rc = push_block(h, h->d_raw, n_in, count, st);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipStreamSynchronize(st));
        return GSH_OK;
    }

    int gsh_cond_push_pinned_async(gsh_cond_t* h, const void* items, uint64_t n_in, uint64_t* first_out, uint64_t* n_out)
    {
        // page-locked block -> device staging (DMA straight out of the caller's memory) -> the fused launch; nothing waits here but for the launch that
        // read this staging buffer four pushes ago
        unsigned long long bytes = 0, count = 0;
        int rc = check_push(h, items, n_in, &bytes, &count);
        if (rc != GSH_OK) return rc;
        report(h, count, first_out, n_out);
        if (n_in == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(h->device));
        hipStream_t st = h->ring->stream;
        const int slot = h->stage_next;
        if (h->stage_done[slot] == nullptr)
            GSH_HIP(hipEventCreateWithFlags(&h->stage_done[slot], hipEventDisableTiming));
        else
            GSH_HIP(hipEventSynchronize(h->stage_done[slot]));
        rc = grow(&h->d_stage[slot], &h->stage_cap[slot], bytes);
        if (rc != GSH_OK) return rc;
        h->stage_next = (slot + 1) % COND_NSTAGE;
        GSH_HIP(hipMemcpyAsync(h->d_stage[slot], items, bytes, hipMemcpyHostToDevice, st));
        rc = push_block(h, h->d_stage[slot], n_in, count, st);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipEventRecord(h->stage_done[slot], st));
        return GSH_OK;
    }

    int gsh_cond_time_push(gsh_cond_t* h, const void* device_block, uint64_t n_in, int reps, float* avg_ms)
    {
        GSH_REQUIRE(h != nullptr && avg_ms != nullptr && device_block != nullptr, "null argument");
        GSH_REQUIRE(n_in >= 1 && reps >= 1, "%llu samples x %d", static_cast<unsigned long long>(n_in), reps);
        unsigned long long bytes = 0;
        int rc = block_bytes(h, n_in, &bytes);
        if (rc != GSH_OK) return rc;
        const unsigned long long count = outputs_total(h, h->n_in_total + n_in) - h->n_out_total;
        GSH_REQUIRE(count >= 1 && count < (1ull << 32), "a block of %llu samples completes %llu outputs: nothing to time", static_cast<unsigned long long>(n_in), count);
        rc = check_stage_span(h, n_in);
        if (rc != GSH_OK) return rc;
        GSH_HIP(hipSetDevice(h->device));
        // the launches of a push, into a scratch destination instead of the ring; the history update lands in the half no push has flipped to (with
        // the blanking or the notch stage: so does what the stage carries, and the decision writes the copy of the state)
        BlankFrame f{};
        NotchFrame nf{};
        if (h->blank_on)
            {
                f = blank_frame(h, n_in);
                rc = blank_reserve(h, f);
                if (rc != GSH_OK) return rc;
            }
        if (h->notch_on)
            {
                nf = notch_frame(h, n_in);
                rc = notch_reserve(h, nf);
                if (rc != GSH_OK) return rc;
            }
        float2* d_out = nullptr;
        GSH_HIP(hipMalloc(&d_out, sizeof(float2) * count));
        CondArgs a = block_args(h, device_block, n_in);
        a.out = d_out;
        a.out0 = h->n_out_total;
        a.n_out = count;
        gsh::cond_plan_resampler(&a);
        hipStream_t st = h->stream;
        hipError_t e = hipSuccess;
        if (h->hist_recorded && (e = hipStreamWaitEvent(st, h->hist_ev, 0)) != hipSuccess) rc = gsh::hip_fail(e, "hipStreamWaitEvent", __FILE__, __LINE__);
        auto once = [&]() {
            int r = GSH_OK;
            if (h->blank_on)
                {
                    gsh::CondBlankArgs b{};
                    r = blank_stage(h, a, f, h->d_bstate + 1, st, &b);
                    if (r == GSH_OK) r = gsh::cond_blank_launch_gather(a, b, st);
                }
            else if (h->notch_on)
                {
                    gsh::CondNotchArgs n{};
                    r = notch_stage(h, a, nf, h->d_nstate + 1, st, &n);
                    if (r == GSH_OK) r = gsh::cond_notch_launch_gather(a, n, st);
                }
            else
                r = gsh::cond_launch(a, st);
            if (r == GSH_OK && h->plan.n_taps > 1) r = gsh::cond_launch_history(a, st);
            return r;
        };
        float ms = 0.0f;
        for (int i = 0; i < 3 && rc == GSH_OK; i++) rc = once();  // clocks up
        if (rc == GSH_OK && (e = hipEventRecord(h->ev0, st)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        for (int i = 0; i < reps && rc == GSH_OK; i++) rc = once();
        if (rc == GSH_OK && (e = hipEventRecord(h->ev1, st)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventSynchronize(h->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventSynchronize", __FILE__, __LINE__);
        if (rc == GSH_OK && (e = hipEventElapsedTime(&ms, h->ev0, h->ev1)) != hipSuccess) rc = gsh::hip_fail(e, "hipEventElapsedTime", __FILE__, __LINE__);
        (void)hipStreamSynchronize(st);
        (void)hipFree(d_out);
        if (rc != GSH_OK) return rc;
        *avg_ms = ms / static_cast<float>(reps);
        return GSH_OK;
    }
}
