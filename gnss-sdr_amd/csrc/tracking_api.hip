// C-ABI tracking entry points (include/gnss_sdr_hip.h): the batched correlator bank
// (gsh_bank_*) and the one-to-one Cpu_Multicorrelator_Real_Codes replacement (gsh_mcorr_*)
// built on top of it.  Host-side bookkeeping only; the arithmetic is in multicorrelator.hip.
// Every entry is a short sequence of the file-local steps below (and of bank_host.h); each step is written once.
#include "bank_host.h"
#include "multicorrelator.h"
#include "multicorrelator_wide.h"
#include "sample_stream.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

namespace
{
// What bank_stage_jobs learns about a batch of the narrow bank.  Committed to the bank once, when the batch is staged; invalidate() whenever the staged table no
// longer stands for what a launch may run.
struct StagedBatch
{
    int n_jobs{0};
    int max_taps{0};
    int mode{0};
    int min_samples{0};
    int max_samples{0};
    unsigned long long max_end{0};  // flat streams; 0 on a ring, where residency is checked per job
    unsigned long long ring_min_start{0}, ring_max_end{0};  // absolute sample range of the batch (ring-bound banks)
    // windowed code staging (multicorrelator.hip): possible when every job of the batch is mode 0 with code_step >= 0
    bool window_eligible{false};
    bool pair{false};  // the batch's 2- / 3-tap jobs are all mcorr_pair_eligible (multicorrelator.h)
    bool half{false};  // ... and all mcorr_half_chip_eligible: taps at exactly -0.5 / 0 / +0.5 chip, no code of the bank too long
    double win_step_max{0.0};       // largest code_phase_step_chips of the batch (code samples per input sample)
    double win_code_span_max{0.0};  // largest code_phase_step_chips * n_samples of the batch: code samples one window walks
    double win_shift_span{0.0};     // largest (max shift - min shift) of the batch
    // pair fusion (multicorrelator.hip, AUX kernels): a single-tap job that follows a job with the same window and NCO parameters (the data
    // prompt track_pilot adds to a pilot channel, trk.cc:1246-1256) is computed by that job's work-groups instead of a second pass
    int n_fused{0};
    // per-flavour launch lists (jobs grouped by tap-count class, fused partners left out); used when a batch mixes classes or has fused jobs
    bool use_classes{false};
    bool lists_fused{false};
    gsh::McorrClassPlan class_plan{};

    void invalidate() { *this = StagedBatch{}; }
};
}  // namespace

struct gsh_bank
{
    int device{0};
    hipStream_t stream{nullptr};
    int n_slots{0};
    int max_code_len{0};
    float* d_codes{nullptr};
    float* d_code_images{nullptr};      // per slot, the LDS image of the half-chip flavour (multicorrelator.h mcorr_build_half_image); banks of codes short enough for it only
    int* d_code_lens{nullptr};
    std::vector<int> h_code_lens;
    gsh::DeviceBuf<float2> stream_owned;
    const float2* d_stream{nullptr};
    unsigned long long stream_len{0};
    gsh_stream* ring{nullptr};          // when set, job windows are absolute sample indices inside this ring
    int splits_user{0};
    int fusion_user{1};
    unsigned long long sample_base{0};  // gsh_bank_set_sample_base
    hipEvent_t ev0{nullptr}, ev1{nullptr};
    StagedBatch batch;
    gsh::DeviceBuf<gsh_corr_job> jobs;
    gsh::DeviceBuf<float2> out, partials;
    gsh::DeviceBuf<int> aux, list;
    std::vector<int> h_aux, h_list;
    gsh::PinnedBuf<gsh_corr_job> h_jobs;  // staging (ring translation; one-synchronisation gsh_bank_correlate)
    gsh::PinnedBuf<float2> h_out;
    // the wide bank (gsh_bank_correlate_wide, multicorrelator_wide.hip): a job table, outputs and staging of its own -- the narrow calls' staged batch stays as it is
    gsh::DeviceBuf<gsh_corr_job_wide> wjobs;
    gsh::DeviceBuf<float2> wout, wpartials;
    gsh::PinnedBuf<gsh_corr_job_wide> h_wjobs;
    gsh::PinnedBuf<float2> h_wout;
};

namespace
{
using gsh::release_all;
using gsh::set_error;

int validate_job(const gsh_bank* b, const gsh_corr_job& j, int idx);

// the position in the bank's ring of job idx's window [start, start + n_samples) (windows never wrap: the ring mirrors its head)
int ring_position(const gsh_bank* b, int idx, unsigned long long start, int n_samples, uint64_t* pos)
{
    const float2* w = nullptr;
    const int rc = gsh::stream_window(b->ring, start, static_cast<unsigned long long>(n_samples), &w);
    if (rc != GSH_OK)
        {
            const std::string why = gsh_last_error();
            return set_error(rc, "job %d: %s", idx, why.c_str());
        }
    *pos = static_cast<uint64_t>(w - b->ring->d_ring);
    return GSH_OK;
}

// launch classes: a 3-tap job inside a 5-tap launch would pay for five taps, so a batch that mixes tap counts is launched per kernel flavour;
// with_fusion leaves the fused partners out (their leaders write their rows).  Reads the staged copy of the batch (h_jobs, h_aux).
int bank_build_lists(gsh_bank* b, StagedBatch& s, bool with_fusion)
{
    const int n_jobs = s.n_jobs;
    const gsh_corr_job* jobs = b->h_jobs.p;
    int count[4] = {0, 0, 0, 0};
    bool has_aux[4] = {false, false, false, false};
    auto cls_of = [](int taps) { return taps <= 1 ? 0 : (taps <= 3 ? 1 : (taps <= 5 ? 2 : 3)); };
    for (int i = 0; i < n_jobs; i++)
        {
            if (with_fusion && b->h_aux[i] == -2) continue;
            const int c = cls_of(jobs[i].n_taps);
            count[c]++;
            if (with_fusion && b->h_aux[i] >= 0) has_aux[c] = true;
        }
    const int classes = (count[0] > 0) + (count[1] > 0) + (count[2] > 0) + (count[3] > 0);
    s.use_classes = (classes > 1) || with_fusion;
    s.lists_fused = with_fusion;
    if (!s.use_classes) return GSH_OK;
    int off[4];
    off[0] = 0;
    for (int c = 1; c < 4; c++) off[c] = off[c - 1] + count[c - 1];
    b->h_list.assign(static_cast<size_t>(n_jobs), 0);
    int fill[4] = {off[0], off[1], off[2], off[3]};
    for (int i = 0; i < n_jobs; i++)
        {
            if (with_fusion && b->h_aux[i] == -2) continue;
            b->h_list[static_cast<size_t>(fill[cls_of(jobs[i].n_taps)]++)] = i;
        }
    GSH_TRY(b->list.grow(static_cast<size_t>(n_jobs)));
    GSH_HIP(hipMemcpyAsync(b->list.p, b->h_list.data(), sizeof(int) * static_cast<size_t>(n_jobs), hipMemcpyHostToDevice, b->stream));
    s.class_plan.list = b->list.p;
    for (int c = 0; c < 4; c++)
        {
            s.class_plan.offset[c] = off[c];
            s.class_plan.count[c] = count[c];
            s.class_plan.aux[c] = has_aux[c];
        }
    return GSH_OK;
}

// staging, part 1: validate the jobs and derive the batch's facts.  No HIP call, nothing of the bank changes.
int batch_facts(const gsh_bank* b, const gsh_corr_job* jobs, int n_jobs, StagedBatch& s)
{
    s.n_jobs = n_jobs;
    s.mode = jobs[0].high_dyn;
    s.min_samples = jobs[0].n_samples;
    s.window_eligible = (s.mode == 0);
    s.pair = true;      // every job the 3-tap launch will see may read its early tap next to the late one (multicorrelator.h mcorr_pair_eligible)
    bool half = true;   // ... and take all three taps from the prompt's index chain (mcorr_half_chip_eligible)
    unsigned long long min_start = ~0ull;
    for (int i = 0; i < n_jobs; i++)
        {
            const gsh_corr_job& j = jobs[i];
            GSH_TRY(validate_job(b, j, i));
            if ((j.n_taps == 2 || j.n_taps == 3) && !gsh::mcorr_pair_eligible(j.n_taps, j.shifts_chips, j.code_phase_step_chips, j.high_dyn)) s.pair = false;
            if ((j.n_taps == 2 || j.n_taps == 3) && !gsh::mcorr_half_chip_eligible(j.n_taps, j.shifts_chips, j.code_phase_step_chips, j.high_dyn, b->max_code_len))
                half = false;
            s.max_samples = std::max(s.max_samples, j.n_samples);
            if (!(j.code_phase_step_chips >= 0.0f)) s.window_eligible = false;
            s.win_step_max = std::max(s.win_step_max, static_cast<double>(j.code_phase_step_chips));
            s.win_code_span_max = std::max(s.win_code_span_max, static_cast<double>(j.code_phase_step_chips) * static_cast<double>(j.n_samples));
            float smin = j.shifts_chips[0], smax = j.shifts_chips[0];
            for (int t = 1; t < j.n_taps; t++)
                {
                    smin = std::min(smin, j.shifts_chips[t]);
                    smax = std::max(smax, j.shifts_chips[t]);
                }
            s.win_shift_span = std::max(s.win_shift_span, static_cast<double>(smax) - static_cast<double>(smin));
            if (j.high_dyn != s.mode)
                return set_error(GSH_ERR_UNSUPPORTED, "job %d: all jobs of one batch must share high_dyn (%d vs %d); split the batch", i, j.high_dyn, s.mode);
            s.max_taps = std::max(s.max_taps, j.n_taps);
            s.min_samples = std::min(s.min_samples, j.n_samples);
            min_start = std::min<unsigned long long>(min_start, j.sample_offset);
            s.max_end = std::max(s.max_end, static_cast<unsigned long long>(j.sample_offset) + static_cast<unsigned long long>(j.n_samples));
        }
    s.half = s.pair && half;
    if (b->ring != nullptr)
        {
            s.ring_min_start = min_start;
            s.ring_max_end = s.max_end;
            s.max_end = 0;  // residency is checked per job (bank_stage_table)
        }
    return GSH_OK;
}

// staging, part 2: the job table into pinned memory (ring mode: absolute sample indices -> ring positions) and from there to the device, queued on the bank's stream
int bank_stage_table(gsh_bank* b, const gsh_corr_job* jobs, int n_jobs)
{
    const size_t n = static_cast<size_t>(n_jobs), staged = static_cast<size_t>(std::max(n_jobs, 64));
    if (n > b->jobs.cap) GSH_TRY(release_all(b->jobs, b->out));
    GSH_TRY(b->jobs.grow(n));
    GSH_TRY(b->out.grow(GSH_MAX_TAPS * n));
    if (staged > b->h_jobs.cap) GSH_TRY(release_all(b->h_jobs, b->h_out));
    GSH_TRY(b->h_jobs.grow(staged));
    GSH_TRY(b->h_out.grow(GSH_MAX_TAPS * staged));
    std::memcpy(b->h_jobs.p, jobs, sizeof(gsh_corr_job) * n);
    if (b->ring != nullptr)
        {
            for (int i = 0; i < n_jobs; i++) GSH_TRY(ring_position(b, i, jobs[i].sample_offset, jobs[i].n_samples, &b->h_jobs.p[i].sample_offset));
            b->d_stream = b->ring->d_ring;
            b->stream_len = b->ring->capacity + b->ring->max_window;
        }
    GSH_HIP(hipMemcpyAsync(b->jobs.p, b->h_jobs.p, sizeof(gsh_corr_job) * n, hipMemcpyHostToDevice, b->stream));
    return GSH_OK;
}

// staging, part 3, pair fusion: job i + 1 rides on job i when it is a single tap over exactly the same samples with exactly the same NCO parameters
int bank_pair_fusion(gsh_bank* b, const gsh_corr_job* jobs, StagedBatch& s)
{
    if (!b->fusion_user || s.mode != 0 || s.max_taps < 2 || s.max_taps > 5) return GSH_OK;
    const int n_jobs = s.n_jobs;
    b->h_aux.assign(static_cast<size_t>(n_jobs), -1);
    for (int i = 0; i + 1 < n_jobs; i++)
        {
            const gsh_corr_job &p = jobs[i], &q = jobs[i + 1];
            if (p.n_taps < 2 || q.n_taps != 1 || b->h_aux[i] == -2) continue;
            if (p.sample_offset != q.sample_offset || p.n_samples != q.n_samples) continue;
            if (std::memcmp(&p.rem_carr_phase_rad, &q.rem_carr_phase_rad, sizeof(float)) != 0 || std::memcmp(&p.phase_step_rad, &q.phase_step_rad, sizeof(float)) != 0 ||
                std::memcmp(&p.rem_code_phase_chips, &q.rem_code_phase_chips, sizeof(float)) != 0 ||
                std::memcmp(&p.code_phase_step_chips, &q.code_phase_step_chips, sizeof(float)) != 0)
                continue;
            b->h_aux[i] = i + 1;
            b->h_aux[i + 1] = -2;
            s.n_fused++;
            i++;
        }
    if (s.n_fused == 0) return GSH_OK;
    GSH_TRY(b->aux.grow(static_cast<size_t>(n_jobs)));
    GSH_HIP(hipMemcpyAsync(b->aux.p, b->h_aux.data(), sizeof(int) * static_cast<size_t>(n_jobs), hipMemcpyHostToDevice, b->stream));
    return GSH_OK;
}

// validate a batch, stage it and queue its host-to-device copies on the bank's stream; the bank's staged batch is the new one on success and none on
// failure.  No synchronisation.
int bank_stage_jobs(gsh_bank* b, const gsh_corr_job* jobs, int n_jobs)
{
    b->batch.invalidate();
    StagedBatch s;
    GSH_TRY(batch_facts(b, jobs, n_jobs, s));
    GSH_HIP(hipSetDevice(b->device));
    GSH_TRY(bank_stage_table(b, jobs, n_jobs));
    GSH_TRY(bank_pair_fusion(b, jobs, s));
    GSH_TRY(bank_build_lists(b, s, s.n_fused > 0));
    b->batch = s;
    return GSH_OK;
}

int bank_splits(const gsh_bank* b)
{
    int s = b->splits_user;
    if (s <= 0)
        {
            // throughput mode once there are a few work-groups per CU; otherwise spread each
            // epoch over several CUs (latency mode for closed-loop tracking)
            s = (b->batch.n_jobs >= 1024) ? 1 : (2048 + b->batch.n_jobs - 1) / std::max(b->batch.n_jobs, 1);
        }
    const int by_len = std::max(1, b->batch.min_samples / 2048);  // keep >= 2048 samples per work-group
    if (b->splits_user <= 0 && b->batch.window_eligible && static_cast<size_t>(b->max_code_len) * sizeof(float) > 20 * 1024)
        {
            // long codes (Galileo E1 / E5, GPS L5 / L2C): the whole code in LDS leaves room for 3-4 work-groups per compute unit.  Cut the
            // windows so that a work-group only walks ~2000 code samples and stages just those (bank_window_floats).
            const int want = static_cast<int>(std::ceil(b->batch.win_code_span_max / 2000.0));
            s = std::max(s, std::min(want, 16));
        }
    s = std::min(s, by_len);
    s = std::min(s, 64);
    return std::max(s, 1);
}

// LDS floats per work-group when only the code samples a segment can touch are staged; 0 when the whole code is staged instead
// (batch not eligible, or the window would not be clearly smaller than the code)
int bank_window_floats(const gsh_bank* b, int splits)
{
    if (!b->batch.window_eligible) return 0;
    // hi - lo + 1 <= step * (seg - 1) + (smax - smin) + 2 in exact arithmetic, seg the job's own segment length; the float evaluation on
    // the device moves either end by a few ulps of values below 2^24, far less than the slack added here (the kernel re-checks and
    // reports NaN if this were ever short)
    double walk = 0.0;
    for (int i = 0; i < b->batch.n_jobs; i++)
        {
            int seg = (b->h_jobs.p[i].n_samples + splits - 1) / splits;
            seg = (seg + 1) & ~1;
            walk = std::max(walk, static_cast<double>(b->h_jobs.p[i].code_phase_step_chips) * static_cast<double>(seg));
        }
    const double need = walk + b->batch.win_shift_span + 16.0;
    if (!(need < 1.0e6)) return 0;
    const int w = (static_cast<int>(std::ceil(need)) + 3) & ~3;
    const int full = b->max_code_len + 2 * 32;
    return (2 * w <= full) ? w : 0;
}

int validate_job(const gsh_bank* b, const gsh_corr_job& j, int idx)
{
    if (j.n_taps < 1 || j.n_taps > GSH_MAX_TAPS) return set_error(GSH_ERR_INVALID, "job %d: n_taps %d outside 1..%d", idx, j.n_taps, GSH_MAX_TAPS);
    if (j.n_samples < 1 || j.n_samples > (1 << 30)) return set_error(GSH_ERR_INVALID, "job %d: n_samples %d", idx, j.n_samples);
    if (j.code_slot < 0 || j.code_slot >= b->n_slots || b->h_code_lens[j.code_slot] <= 0)
        return set_error(GSH_ERR_STATE, "job %d: code slot %d has no local code", idx, j.code_slot);
    if (j.high_dyn < 0 || j.high_dyn > 2) return set_error(GSH_ERR_INVALID, "job %d: high_dyn %d", idx, j.high_dyn);
    if (j.high_dyn != 0)
        {
            // the reference derives taps 1..T-1 by rotating tap 0 by round(dshift/step) samples
            // (K/..high_dynamics_resampler..:82-90); a rotation outside [0, n] is undefined there.
            unsigned acc = 0;
            for (int t = 1; t < j.n_taps; t++)
                {
                    const float q = (j.shifts_chips[t] - j.shifts_chips[t - 1]) / j.code_phase_step_chips;
                    if (!std::isfinite(q)) return set_error(GSH_ERR_INVALID, "job %d: high-dynamics tap spacing / code step is not finite", idx);
                    acc += static_cast<unsigned>(static_cast<int>(std::round(q)));
                    if (acc > static_cast<unsigned>(j.n_samples))
                        return set_error(GSH_ERR_INVALID, "job %d: high-dynamics tap rotation %u outside [0, %d] (taps must ascend)", idx, acc, j.n_samples);
                }
        }
    return GSH_OK;
}

// ---- the wide bank: validation, staging and launch of a batch of gsh_corr_job_wide (the kernels: multicorrelator_wide.hip)
int validate_job_wide(const gsh_bank* b, const gsh_corr_job_wide& j, int idx)
{
    if (j.n_taps < 1 || j.n_taps > GSH_MAX_WIDE_TAPS) return set_error(GSH_ERR_INVALID, "job %d: n_taps %d outside 1..%d", idx, j.n_taps, GSH_MAX_WIDE_TAPS);
    if (j.n_samples < 1 || j.n_samples > (1 << 30)) return set_error(GSH_ERR_INVALID, "job %d: n_samples %d", idx, j.n_samples);
    if (j.code_slot < 0 || j.code_slot >= b->n_slots || b->h_code_lens[j.code_slot] <= 0)
        return set_error(GSH_ERR_STATE, "job %d: code slot %d has no local code", idx, j.code_slot);
    if (!std::isfinite(j.rem_carr_phase_rad) || !std::isfinite(j.phase_step_rad) || !std::isfinite(j.rem_code_phase_chips) || !std::isfinite(j.code_phase_step_chips))
        return set_error(GSH_ERR_INVALID, "job %d: a carrier or code parameter is not finite", idx);
    for (int t = 0; t < j.n_taps; t++)
        {
            if (!std::isfinite(j.shifts_chips[t])) return set_error(GSH_ERR_INVALID, "job %d: shift %d is not finite", idx, t);
            if (t > 0 && j.shifts_chips[t] < j.shifts_chips[t - 1])
                return set_error(GSH_ERR_INVALID, "job %d: shifts must ascend (shift %d = %g after %g)", idx, t, static_cast<double>(j.shifts_chips[t]),
                    static_cast<double>(j.shifts_chips[t - 1]));
        }
    return GSH_OK;
}

// an upper bound of the code-table entries one work-group of job j stages: the chip indices of one segment under the widest tap block.  In exact arithmetic
// hi - lo + 1 <= |step| (seg - 1) + (block's shift span) + 2; each of the chain's three roundings moves either end by at most half an ulp of a value no larger
// than `mag`.  (The kernel sizes its table from the indices themselves and reports NaN if this were ever short.)
double wide_table_need(const gsh_corr_job_wide& j, int splits)
{
    int seg = (j.n_samples + splits - 1) / splits;
    seg = (seg + 1) & ~1;
    const double step = std::fabs(static_cast<double>(j.code_phase_step_chips));
    double span = 0.0;
    for (int t0 = 0; t0 < j.n_taps; t0 += gsh::MCORR_WIDE_MAX_BLOCK)
        {
            const int t1 = std::min(j.n_taps, t0 + gsh::MCORR_WIDE_MAX_BLOCK) - 1;
            span = std::max(span, static_cast<double>(j.shifts_chips[t1]) - static_cast<double>(j.shifts_chips[t0]));
        }
    const double mag = step * static_cast<double>(j.n_samples) + std::max(std::fabs(static_cast<double>(j.shifts_chips[0])), std::fabs(static_cast<double>(j.shifts_chips[j.n_taps - 1])))
                       + std::fabs(static_cast<double>(j.rem_code_phase_chips));
    return step * static_cast<double>(seg) + span + 8.0 + mag * (1.0 / 1048576.0);
}

// what one wide batch needs besides its job table
struct WidePlan
{
    int max_taps{0};
    int max_splits{1};
    int table_floats{1};
    unsigned long long min_start{~0ull}, max_end{0};  // absolute sample range (sample base applied)
};

// validate the batch, stage it in pinned memory with every window turned into a position in the attached stream (sample base applied; ring-bound banks:
// the ring position of the absolute index -- windows never wrap, the ring mirrors its head) and queue the host-to-device copy.  No synchronisation.
int bank_stage_wide(gsh_bank* b, const gsh_corr_job_wide* jobs, int n_jobs, WidePlan* plan)
{
    if (b->d_stream == nullptr) return set_error(GSH_ERR_STATE, "no sample stream attached (gsh_bank_set_stream_*)");
    const int cap = gsh::mcorr_wide_table_cap();
    double need_max = 1.0;
    bool whole_code = false;
    for (int i = 0; i < n_jobs; i++)
        {
            GSH_TRY(validate_job_wide(b, jobs[i], i));
            const unsigned long long start = static_cast<unsigned long long>(jobs[i].sample_offset) + b->sample_base;
            const unsigned long long end = start + static_cast<unsigned long long>(jobs[i].n_samples);
            if (start < b->sample_base || end < start) return set_error(GSH_ERR_INVALID, "job %d: sample_offset %llu", i, static_cast<unsigned long long>(jobs[i].sample_offset));
            if (b->ring == nullptr && end > b->stream_len)
                return set_error(GSH_ERR_INVALID, "job %d: the window ends at sample %llu (sample_base %llu), past the %llu-sample stream", i, end, b->sample_base, b->stream_len);
            plan->min_start = std::min(plan->min_start, start);
            plan->max_end = std::max(plan->max_end, end);
            plan->max_taps = std::max(plan->max_taps, jobs[i].n_taps);
            const int splits = gsh::mcorr_wide_splits(jobs[i].n_samples, b->splits_user);
            plan->max_splits = std::max(plan->max_splits, splits);
            const double need = wide_table_need(jobs[i], splits);
            if (need <= static_cast<double>(cap))
                need_max = std::max(need_max, need);
            else
                whole_code = true;  // this job's tap blocks take the whole code and wrap every index
        }
    plan->table_floats = (static_cast<int>(std::ceil(need_max)) + 3) & ~3;
    if (whole_code) plan->table_floats = std::max(plan->table_floats, (b->max_code_len + 3) & ~3);
    plan->table_floats = std::min(plan->table_floats, cap);
    GSH_REQUIRE(!whole_code || b->max_code_len <= cap, "a code of %d samples does not fit the wide bank's table (%d)", b->max_code_len, cap);
    GSH_HIP(hipSetDevice(b->device));
    const size_t n = static_cast<size_t>(std::max(n_jobs, 32));
    if (n > b->wjobs.cap) GSH_TRY(release_all(b->wjobs, b->wout, b->h_wjobs, b->h_wout));
    GSH_TRY(b->wjobs.grow(n));
    GSH_TRY(b->wout.grow(GSH_MAX_WIDE_TAPS * n));
    GSH_TRY(b->h_wjobs.grow(n));
    GSH_TRY(b->h_wout.grow(GSH_MAX_WIDE_TAPS * n));
    if (plan->max_splits > 1) GSH_TRY(b->wpartials.grow(static_cast<size_t>(n_jobs) * plan->max_splits * GSH_MAX_WIDE_TAPS));
    std::memcpy(b->h_wjobs.p, jobs, sizeof(gsh_corr_job_wide) * static_cast<size_t>(n_jobs));
    for (int i = 0; i < n_jobs; i++)
        {
            const unsigned long long start = static_cast<unsigned long long>(jobs[i].sample_offset) + b->sample_base;
            if (b->ring != nullptr)
                GSH_TRY(ring_position(b, i, start, jobs[i].n_samples, &b->h_wjobs.p[i].sample_offset));
            else
                b->h_wjobs.p[i].sample_offset = start;
        }
    if (b->ring != nullptr) b->d_stream = b->ring->d_ring;
    GSH_HIP(hipMemcpyAsync(b->wjobs.p, b->h_wjobs.p, sizeof(gsh_corr_job_wide) * static_cast<size_t>(n_jobs), hipMemcpyHostToDevice, b->stream));
    return GSH_OK;
}

int bank_launch_wide(gsh_bank* b, int n_jobs, const WidePlan& plan)
{
    gsh::McorrWideArgs a{};
    a.stream = b->d_stream;
    a.jobs = b->wjobs.p;
    a.codes = b->d_codes;
    a.code_lens = b->d_code_lens;
    a.code_stride = b->max_code_len;
    a.out = b->wout.p;
    a.partials = b->wpartials.p;
    a.n_jobs = n_jobs;
    a.splits_user = b->splits_user;
    a.max_splits = plan.max_splits;
    a.table_floats = plan.table_floats;
    a.max_taps = plan.max_taps;
    if (b->ring != nullptr) GSH_TRY(gsh::stream_wait_pushed(b->ring, plan.max_end, b->stream));  // the push that completed this batch's newest window
    GSH_TRY(gsh::mcorr_wide_launch(a, b->stream));
    if (b->ring != nullptr) return gsh::stream_mark_read(b->ring, plan.min_start, b->stream);  // pushes that would overwrite these windows wait
    return GSH_OK;
}

// ---- the steps of a narrow launch
// may the staged batch run on what is attached now?  (Both may have changed since it was staged: set_stream_*, set_sample_base, pushes.)
int bank_may_launch(const gsh_bank* b)
{
    const StagedBatch& s = b->batch;
    if (b->ring == nullptr) return gsh::batch_fits_stream(b->d_stream, s.max_end, b->sample_base, b->stream_len);
    if (s.ring_max_end == 0) return GSH_OK;
    // the shifted windows must be resident and pushed: a base that points at samples the ring no longer (or not yet) holds would make
    // the kernel read whatever lives at those ring positions now
    const unsigned long long lo = s.ring_min_start + b->sample_base, hi = s.ring_max_end + b->sample_base;
    if (lo < gsh::stream_oldest(b->ring) || hi > b->ring->next)
        return set_error(GSH_ERR_INVALID, "windows [%llu, %llu) (sample_base %llu) are not resident (ring holds [%llu, %llu))", lo, hi, b->sample_base,
            gsh::stream_oldest(b->ring), static_cast<unsigned long long>(b->ring->next));
    return GSH_OK;
}

// what the launcher is told about the staged batch cut `splits` ways; aux is set when the batch's fused pairs run fused
gsh::McorrArgs bank_launch_args(const gsh_bank* b, int splits)
{
    gsh::McorrArgs a;
    a.stream = b->d_stream;
    a.stream_len = b->stream_len;
    a.jobs = b->jobs.p;
    a.codes = b->d_codes;
    a.code_lens = b->d_code_lens;
    a.code_stride = b->max_code_len;
    a.code_images = b->d_code_images;
    a.out = b->out.p;
    a.partials = b->partials.p;
    a.n_jobs = b->batch.n_jobs;
    a.splits = splits;
    a.window_floats = bank_window_floats(b, splits);
    a.packed = gsh::mcorr_packed_default();
    a.fac = gsh::mcorr_fac_default();
    a.pair = b->batch.pair ? 1 : 0;
    a.half = b->batch.half ? 1 : 0;
    a.sample_base = b->sample_base;
    a.ring_capacity = b->ring != nullptr ? b->ring->capacity : 0ull;
    // the second code table must not cost the occupancy the fusion is meant to win: only with windowed tables or short codes
    const bool fuse = b->batch.n_fused > 0 && (a.window_floats > 0 || static_cast<size_t>(b->max_code_len) * sizeof(float) <= 10 * 1024);
    a.aux = fuse ? b->aux.p : nullptr;
    a.job_list = nullptr;
    a.n_launch = b->batch.n_jobs;
    return a;
}

// ---- the tail of every synchronous entry.  `rc` is what staging and launch answered: a failure waits for whatever was queued (and leaves no staged batch
// where the narrow table was touched); a success brings bytes_d2h bytes from `d_from` through `pinned` and hands the first bytes_out of them to the caller.
int bank_fetch(gsh_bank* b, int rc, bool narrow, const float2* d_from, float2* pinned, size_t bytes_d2h, void* out, size_t bytes_out)
{
    if (rc != GSH_OK)
        {
            (void)hipStreamSynchronize(b->stream);
            if (narrow) b->batch.invalidate();
            return rc;
        }
    GSH_HIP(hipMemcpyAsync(pinned, d_from, bytes_d2h, hipMemcpyDeviceToHost, b->stream));
    GSH_HIP(hipStreamSynchronize(b->stream));
    std::memcpy(out, pinned, bytes_out);
    return GSH_OK;
}

int bank_run_wide(gsh_bank* b, const gsh_corr_job_wide* jobs, int n_jobs, WidePlan* plan)
{
    GSH_TRY(bank_stage_wide(b, jobs, n_jobs, plan));
    return bank_launch_wide(b, n_jobs, *plan);
}

int bank_run(gsh_bank* b, const gsh_corr_job* jobs, int n_jobs)
{
    GSH_TRY(bank_stage_jobs(b, jobs, n_jobs));
    return gsh_bank_launch(b, nullptr);
}
}  // namespace

extern "C"
{
    int gsh_bank_create(int device, int n_code_slots, int max_code_length, gsh_bank_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null out pointer");
        *out = nullptr;
        GSH_REQUIRE(n_code_slots >= 1 && n_code_slots <= 65536, "n_code_slots %d", n_code_slots);
        GSH_REQUIRE(max_code_length >= 1, "max_code_length %d", max_code_length);
        GSH_REQUIRE(gsh::mcorr_lds_bytes(max_code_length) <= 64 * 1024, "max_code_length %d does not fit the LDS code table (limit %d samples)", max_code_length, 64 * 1024 / 4 - 128);
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_bank* b = new (std::nothrow) gsh_bank();
        GSH_REQUIRE(b != nullptr, "out of host memory");
        b->device = device;
        b->n_slots = n_code_slots;
        b->max_code_len = max_code_length;
        b->h_code_lens.assign(n_code_slots, 0);
        auto fail = [&](hipError_t e, const char* what) {
            gsh::hip_fail(e, what, __FILE__, __LINE__);
            gsh_bank_destroy(b);
            return GSH_ERR_HIP;
        };
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        if ((e = hipMalloc(&b->d_codes, sizeof(float) * static_cast<size_t>(n_code_slots) * max_code_length)) != hipSuccess) return fail(e, "hipMalloc(codes)");
        if (max_code_length <= gsh::MCORR_HALF_MAX_CODE_LEN)
            {
                const size_t image_bytes = sizeof(float) * static_cast<size_t>(n_code_slots) * gsh::MCORR_HALF_IMAGE_WORDS;
                if ((e = hipMalloc(&b->d_code_images, image_bytes)) != hipSuccess) return fail(e, "hipMalloc(code images)");
                if ((e = hipMemset(b->d_code_images, 0, image_bytes)) != hipSuccess) return fail(e, "hipMemset");
            }
        if ((e = hipMalloc(&b->d_code_lens, sizeof(int) * n_code_slots)) != hipSuccess) return fail(e, "hipMalloc(code_lens)");
        if ((e = hipMemset(b->d_code_lens, 0, sizeof(int) * n_code_slots)) != hipSuccess) return fail(e, "hipMemset");
        if ((e = hipEventCreate(&b->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipEventCreate(&b->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
        *out = b;
        return GSH_OK;
    }

    void gsh_bank_destroy(gsh_bank_t* b)
    {
        if (!b) return;
        (void)hipSetDevice(b->device);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        if (b->d_codes) (void)hipFree(b->d_codes);
        if (b->d_code_images) (void)hipFree(b->d_code_images);
        if (b->d_code_lens) (void)hipFree(b->d_code_lens);
        (void)release_all(b->stream_owned, b->jobs, b->out, b->partials, b->aux, b->list);
        if (b->ev0) (void)hipEventDestroy(b->ev0);
        if (b->ev1) (void)hipEventDestroy(b->ev1);
        (void)release_all(b->h_jobs, b->h_out, b->wjobs, b->wout, b->wpartials, b->h_wjobs, b->h_wout);
        if (b->stream) (void)hipStreamDestroy(b->stream);
        delete b;
    }

    int gsh_bank_set_code(gsh_bank_t* b, int slot, const float* code, int code_length)
    {
        GSH_REQUIRE(b && code, "null argument");
        GSH_REQUIRE(slot >= 0 && slot < b->n_slots, "slot %d outside 0..%d", slot, b->n_slots - 1);
        GSH_REQUIRE(code_length >= 1 && code_length <= b->max_code_len, "code_length %d outside 1..%d", code_length, b->max_code_len);
        GSH_HIP(hipSetDevice(b->device));
        GSH_HIP(hipStreamSynchronize(b->stream));
        GSH_HIP(hipMemcpy(b->d_codes + static_cast<size_t>(slot) * b->max_code_len, code, sizeof(float) * code_length, hipMemcpyHostToDevice));
        if (b->d_code_images != nullptr)
            {
                // the slot's LDS image for the half-chip kernels: a host loop over 3 264 words and one copy of 13 KB
                float image[gsh::MCORR_HALF_IMAGE_WORDS];
                gsh::mcorr_build_half_image(code, code_length, image);
                GSH_HIP(hipMemcpy(b->d_code_images + static_cast<size_t>(slot) * gsh::MCORR_HALF_IMAGE_WORDS, image, sizeof(image), hipMemcpyHostToDevice));
            }
        GSH_HIP(hipMemcpy(b->d_code_lens + slot, &code_length, sizeof(int), hipMemcpyHostToDevice));
        b->h_code_lens[slot] = code_length;
        return GSH_OK;
    }

    int gsh_bank_set_stream_host(gsh_bank_t* b, const float* iq, uint64_t n_samples)
    {
        GSH_REQUIRE(b && iq, "null argument");
        GSH_REQUIRE(n_samples >= 1, "empty stream");
        GSH_HIP(hipSetDevice(b->device));
        GSH_HIP(hipStreamSynchronize(b->stream));
        GSH_TRY(b->stream_owned.grow(static_cast<size_t>(n_samples) + 2));  // one spare pair: 16-byte loads may touch sample n
        GSH_HIP(hipMemcpy(b->stream_owned.p, iq, sizeof(float2) * n_samples, hipMemcpyHostToDevice));
        GSH_HIP(hipMemset(b->stream_owned.p + n_samples, 0, sizeof(float2) * 2));
        b->d_stream = b->stream_owned.p;
        b->stream_len = n_samples;
        b->ring = nullptr;
        return GSH_OK;
    }

    int gsh_bank_set_stream_device(gsh_bank_t* b, const void* device_iq, uint64_t n_samples)
    {
        GSH_REQUIRE(b && device_iq, "null argument");
        GSH_REQUIRE(n_samples >= 1, "empty stream");
        GSH_REQUIRE((reinterpret_cast<uintptr_t>(device_iq) & 15u) == 0, "device stream must be 16-byte aligned");
        b->d_stream = static_cast<const float2*>(device_iq);
        b->stream_len = n_samples;
        b->ring = nullptr;
        return GSH_OK;
    }

    int gsh_bank_set_splits(gsh_bank_t* b, int splits)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_REQUIRE(splits >= 0 && splits <= 64, "splits %d outside 0..64", splits);
        b->splits_user = splits;
        return GSH_OK;
    }

    int gsh_bank_set_sample_base(gsh_bank_t* b, uint64_t sample_base)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        b->sample_base = sample_base;
        return GSH_OK;
    }

    int gsh_bank_set_pair_fusion(gsh_bank_t* b, int enable)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        b->fusion_user = enable ? 1 : 0;
        b->batch.invalidate();  // the staged batch was analysed under the previous setting
        return GSH_OK;
    }

    int gsh_bank_upload_jobs(gsh_bank_t* b, const gsh_corr_job* jobs, int n_jobs)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_REQUIRE(n_jobs >= 0, "n_jobs %d", n_jobs);
        GSH_REQUIRE(n_jobs == 0 || jobs != nullptr, "null jobs");
        b->batch.invalidate();
        if (n_jobs == 0) return GSH_OK;
        GSH_TRY(bank_stage_jobs(b, jobs, n_jobs));
        GSH_HIP(hipStreamSynchronize(b->stream));
        return GSH_OK;
    }

    int gsh_bank_set_stream_ring(gsh_bank_t* b, gsh_stream_t* s)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_REQUIRE(s == nullptr || s->device == b->device, "the ring lives on device %d, the bank on device %d", s ? s->device : -1, b->device);
        b->ring = s;
        b->batch.invalidate();  // an uploaded job table was translated against the previous attachment
        b->d_stream = s != nullptr ? s->d_ring : nullptr;
        b->stream_len = s != nullptr ? s->capacity + s->max_window : 0;
        return GSH_OK;
    }

    // check, reserve the partials, fill the arguments, wait for the push, regroup if the fusion verdict changed, launch, mark the ring read
    int gsh_bank_launch(gsh_bank_t* b, void* hip_stream)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        StagedBatch& batch = b->batch;
        if (batch.n_jobs == 0) return GSH_OK;
        GSH_TRY(bank_may_launch(b));
        GSH_HIP(hipSetDevice(b->device));
        const int splits = bank_splits(b);
        if (splits > 1) GSH_TRY(b->partials.grow(static_cast<size_t>(batch.n_jobs) * splits * GSH_MAX_TAPS));
        const gsh::McorrArgs a = bank_launch_args(b, splits);
        const bool fuse = a.aux != nullptr;
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : b->stream;
        // wait for the push that completed this batch's newest window -- not for a later block that may already be on its way
        if (b->ring != nullptr) GSH_TRY(gsh::stream_wait_pushed(b->ring, batch.ring_max_end ? batch.ring_max_end + b->sample_base : ~0ull, s));
        if (batch.lists_fused != fuse)
            {
                // the LDS rule of bank_launch_args changed its verdict since the batch was staged (set_splits in between): regroup
                GSH_TRY(bank_build_lists(b, batch, fuse));
                GSH_HIP(hipStreamSynchronize(b->stream));  // the list upload was queued on the bank's stream
            }
        GSH_TRY(batch.use_classes ? gsh::mcorr_launch_classes(a, batch.class_plan, batch.mode, b->max_code_len, s)
                                  : gsh::mcorr_launch(a, batch.max_taps, batch.mode, b->max_code_len, s));
        if (b->ring != nullptr) return gsh::stream_mark_read(b->ring, batch.ring_min_start + b->sample_base, s);  // pushes that would overwrite these windows wait
        return GSH_OK;
    }

    int gsh_bank_synchronize(gsh_bank_t* b)
    {
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_HIP(hipSetDevice(b->device));
        GSH_HIP(hipStreamSynchronize(b->stream));
        return GSH_OK;
    }

    int gsh_bank_read_outputs(gsh_bank_t* b, float* out_iq, int n_jobs)
    {
        GSH_REQUIRE(b && out_iq, "null argument");
        GSH_REQUIRE(n_jobs >= 0 && n_jobs <= b->batch.n_jobs, "n_jobs %d outside 0..%d", n_jobs, b->batch.n_jobs);
        if (n_jobs == 0) return GSH_OK;
        GSH_HIP(hipSetDevice(b->device));
        GSH_HIP(hipMemcpyAsync(out_iq, b->out.p, sizeof(float2) * GSH_MAX_TAPS * static_cast<size_t>(n_jobs), hipMemcpyDeviceToHost, b->stream));
        GSH_HIP(hipStreamSynchronize(b->stream));
        return GSH_OK;
    }

    int gsh_bank_correlate(gsh_bank_t* b, const gsh_corr_job* jobs, int n_jobs, float* out_iq)
    {
        // one synchronisation per batch: pinned job table -> H2D -> kernel -> D2H into pinned memory, all queued on the bank's stream
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_REQUIRE(n_jobs >= 0, "n_jobs %d", n_jobs);
        GSH_REQUIRE(n_jobs == 0 || (jobs != nullptr && out_iq != nullptr), "null argument");
        b->batch.invalidate();
        if (n_jobs == 0) return GSH_OK;
        const int rc = bank_run(b, jobs, n_jobs);
        const size_t bytes = sizeof(float2) * GSH_MAX_TAPS * static_cast<size_t>(n_jobs);
        return bank_fetch(b, rc, true, b->out.p, b->h_out.p, bytes, out_iq, bytes);
    }

    int gsh_bank_time_launches(gsh_bank_t* b, int reps, float* avg_ms)
    {
        GSH_REQUIRE(b && avg_ms, "null argument");
        GSH_REQUIRE(reps >= 1, "reps %d", reps);
        GSH_HIP(hipSetDevice(b->device));
        GSH_TRY(gsh_bank_launch(b, nullptr));  // warm-up, also validates state
        return gsh::time_launches(b->ev0, b->ev1, b->stream, reps, avg_ms, [b] { return gsh_bank_launch(b, nullptr); });
    }

    int gsh_bank_correlate_wide(gsh_bank_t* b, const gsh_corr_job_wide* jobs, int n_jobs, float* out_iq)
    {
        // one synchronisation per batch, as gsh_bank_correlate: pinned job table -> H2D -> kernel(s) -> D2H into pinned memory, all queued on the bank's stream
        GSH_REQUIRE(b != nullptr, "null bank");
        GSH_REQUIRE(n_jobs >= 0, "n_jobs %d", n_jobs);
        GSH_REQUIRE(n_jobs == 0 || (jobs != nullptr && out_iq != nullptr), "null argument");
        if (n_jobs == 0) return GSH_OK;
        WidePlan plan;
        const int rc = bank_run_wide(b, jobs, n_jobs, &plan);
        const size_t bytes = sizeof(float2) * GSH_MAX_WIDE_TAPS * static_cast<size_t>(n_jobs);
        return bank_fetch(b, rc, false, b->wout.p, b->h_wout.p, bytes, out_iq, bytes);
    }

    int gsh_bank_time_launches_wide(gsh_bank_t* b, const gsh_corr_job_wide* jobs, int n_jobs, int reps, float* avg_ms)
    {
        GSH_REQUIRE(b && avg_ms, "null argument");
        GSH_REQUIRE(n_jobs >= 1 && jobs != nullptr, "no jobs");
        GSH_REQUIRE(reps >= 1, "reps %d", reps);
        WidePlan plan;
        int rc = bank_run_wide(b, jobs, n_jobs, &plan);  // its launch is the warm-up
        if (rc == GSH_OK) rc = gsh::time_launches(b->ev0, b->ev1, b->stream, reps, avg_ms, [&] { return bank_launch_wide(b, n_jobs, plan); });
        if (rc != GSH_OK) (void)hipStreamSynchronize(b->stream);
        return rc;
    }
}

// ------------------------------------------------------------------------------------------
// gsh_mcorr_*: Cpu_Multicorrelator_Real_Codes replacement (mcorr.h:37-61)
// ------------------------------------------------------------------------------------------
struct gsh_mcorr
{
    int device{0};
    gsh_bank* bank{nullptr};
    int max_len{0};
    int n_correlators{0};
    int code_len{0};
    float* shifts{nullptr};       // borrowed, re-read every call (mcorr.cc:58)
    const float* sig_in{nullptr}; // borrowed (mcorr.cc:69)
    float* corr_out{nullptr};     // borrowed (mcorr.cc:70)
    bool high_dyn{true};          // mcorr.h:60 default
    float2* h_pinned_in{nullptr};
    float2* h_pinned_out{nullptr};
    float2* d_in{nullptr};
};

namespace
{
// the one job of a call, as far as both job records go: the whole epoch, slot 0, the taps as the caller's array holds them now
template <typename Job>
Job mcorr_job(const gsh_mcorr* h, float rem_carr, float phase_step, float rem_code, float code_step, int n)
{
    Job j;
    std::memset(&j, 0, sizeof(j));
    j.n_samples = n;
    j.rem_carr_phase_rad = rem_carr;
    j.phase_step_rad = phase_step;
    j.rem_code_phase_chips = rem_code;
    j.code_phase_step_chips = code_step;
    j.n_taps = h->n_correlators;
    for (int t = 0; t < h->n_correlators; t++) j.shifts_chips[t] = h->shifts[t];
    return j;
}

// the epoch through pinned staging onto the device, queued on the bank's stream, and attached as the bank's stream
int mcorr_attach_epoch(gsh_mcorr* h, int n)
{
    std::memcpy(h->h_pinned_in, h->sig_in, sizeof(float2) * static_cast<size_t>(n));
    GSH_HIP(hipMemcpyAsync(h->d_in, h->h_pinned_in, sizeof(float2) * static_cast<size_t>(n), hipMemcpyHostToDevice, h->bank->stream));
    h->bank->d_stream = h->d_in;
    h->bank->stream_len = static_cast<unsigned long long>(n);
    return GSH_OK;
}

// more than GSH_MAX_TAPS correlators: one job of the wide bank (standard resampler and rotator only)
int mcorr_run_wide(gsh_mcorr* h, int mode, float rem_carr, float phase_step, float rem_code, float code_step, int n)
{
    gsh_bank* b = h->bank;
    int rc = mode == 0 ? GSH_OK
                       : set_error(GSH_ERR_UNSUPPORTED,
                             "%d correlators: more than %d run the wide bank, which has the standard resampler only -- call set_high_dynamics_resampler(false)",
                             h->n_correlators, GSH_MAX_TAPS);
    if (rc == GSH_OK) rc = mcorr_attach_epoch(h, n);
    if (rc == GSH_OK)
        {
            const gsh_corr_job_wide j = mcorr_job<gsh_corr_job_wide>(h, rem_carr, phase_step, rem_code, code_step, n);
            WidePlan plan;
            rc = bank_run_wide(b, &j, 1, &plan);
            rc = bank_fetch(b, rc, false, b->wout.p, h->h_pinned_out, sizeof(float2) * GSH_MAX_WIDE_TAPS, h->corr_out, sizeof(float2) * static_cast<size_t>(h->n_correlators));
        }
    // the reference leaves valid results behind every call; a caller that does not look at the status must not see the previous epoch's
    if (rc != GSH_OK) std::memset(h->corr_out, 0, sizeof(float2) * static_cast<size_t>(h->n_correlators));
    return rc;
}

int mcorr_run(gsh_mcorr* h, int mode, float rem_carr, float phase_step, float phase_rate, float rem_code, float code_step, float code_rate, int n)
{
    GSH_REQUIRE(h != nullptr, "null handle");
    if (h->bank == nullptr || h->d_in == nullptr) return set_error(GSH_ERR_STATE, "init() has not been called");
    if (h->code_len <= 0 || h->shifts == nullptr) return set_error(GSH_ERR_STATE, "set_local_code_and_taps() has not been called");
    if (h->sig_in == nullptr || h->corr_out == nullptr) return set_error(GSH_ERR_STATE, "set_input_output_vectors() has not been called");
    GSH_REQUIRE(n >= 1 && n <= h->max_len, "signal_length_samples %d outside 1..%d (init size)", n, h->max_len);
    gsh_bank* b = h->bank;
    GSH_HIP(hipSetDevice(h->device));
    if (h->n_correlators > GSH_MAX_TAPS) return mcorr_run_wide(h, mode, rem_carr, phase_step, rem_code, code_step, n);

    gsh_corr_job j = mcorr_job<gsh_corr_job>(h, rem_carr, phase_step, rem_code, code_step, n);
    j.phase_rate_step_rad = phase_rate;
    j.code_phase_rate_step_chips = code_rate;
    j.high_dyn = mode;
    // one synchronisation per call: the epoch and the job record H2D, the kernel and D2H of T complex values are all queued on the bank's stream
    GSH_TRY(mcorr_attach_epoch(h, n));
    const int rc = bank_run(b, &j, 1);
    return bank_fetch(b, rc, true, b->out.p, h->h_pinned_out, sizeof(float2) * GSH_MAX_TAPS, h->corr_out, sizeof(float2) * static_cast<size_t>(h->n_correlators));
}
}  // namespace

extern "C"
{
    int gsh_mcorr_create(int device, gsh_mcorr_t** out)
    {
        GSH_REQUIRE(out != nullptr, "null out pointer");
        *out = nullptr;
        int rc = gsh::use_device(device);
        if (rc != GSH_OK) return rc;
        gsh_mcorr* h = new (std::nothrow) gsh_mcorr();
        GSH_REQUIRE(h != nullptr, "out of host memory");
        h->device = device;
        *out = h;
        return GSH_OK;
    }

    int gsh_mcorr_free(gsh_mcorr_t* h)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        (void)hipSetDevice(h->device);
        if (h->bank) gsh_bank_destroy(h->bank);
        h->bank = nullptr;
        if (h->h_pinned_in) (void)hipHostFree(h->h_pinned_in);
        if (h->h_pinned_out) (void)hipHostFree(h->h_pinned_out);
        if (h->d_in) (void)hipFree(h->d_in);
        h->h_pinned_in = nullptr;
        h->h_pinned_out = nullptr;
        h->d_in = nullptr;
        h->max_len = 0;
        h->code_len = 0;
        return GSH_OK;
    }

    void gsh_mcorr_destroy(gsh_mcorr_t* h)
    {
        if (!h) return;
        gsh_mcorr_free(h);
        delete h;
    }

    int gsh_mcorr_init(gsh_mcorr_t* h, int max_signal_length_samples, int n_correlators)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        GSH_REQUIRE(max_signal_length_samples >= 1, "max_signal_length_samples %d", max_signal_length_samples);
        GSH_REQUIRE(n_correlators >= 1 && n_correlators <= GSH_MAX_WIDE_TAPS, "n_correlators %d outside 1..%d", n_correlators, GSH_MAX_WIDE_TAPS);
        gsh_mcorr_free(h);
        GSH_HIP(hipSetDevice(h->device));
        h->max_len = max_signal_length_samples;
        h->n_correlators = n_correlators;
        GSH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_pinned_in), sizeof(float2) * static_cast<size_t>(max_signal_length_samples), hipHostMallocDefault));
        GSH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_pinned_out), sizeof(float2) * GSH_MAX_WIDE_TAPS, hipHostMallocDefault));
        GSH_HIP(hipMalloc(&h->d_in, sizeof(float2) * (static_cast<size_t>(max_signal_length_samples) + 2)));
        GSH_HIP(hipMemset(h->d_in, 0, sizeof(float2) * (static_cast<size_t>(max_signal_length_samples) + 2)));
        return GSH_OK;
    }

    int gsh_mcorr_set_local_code_and_taps(gsh_mcorr_t* h, int code_length_chips, const float* local_code_in, float* shifts_chips)
    {
        GSH_REQUIRE(h && local_code_in && shifts_chips, "null argument");
        GSH_REQUIRE(code_length_chips >= 1, "code_length_chips %d", code_length_chips);
        if (h->d_in == nullptr) return set_error(GSH_ERR_STATE, "init() has not been called");
        if (h->bank == nullptr || h->bank->max_code_len < code_length_chips)
            {
                if (h->bank) gsh_bank_destroy(h->bank);
                h->bank = nullptr;
                int rc = gsh_bank_create(h->device, 1, code_length_chips, &h->bank);
                if (rc != GSH_OK) return rc;
            }
        int rc = gsh_bank_set_code(h->bank, 0, local_code_in, code_length_chips);
        if (rc != GSH_OK) return rc;
        h->code_len = code_length_chips;
        h->shifts = shifts_chips;
        return GSH_OK;
    }

    int gsh_mcorr_set_input_output_vectors(gsh_mcorr_t* h, float* corr_out_iq, const float* sig_in_iq)
    {
        GSH_REQUIRE(h && corr_out_iq && sig_in_iq, "null argument");
        h->corr_out = corr_out_iq;
        h->sig_in = sig_in_iq;
        return GSH_OK;
    }

    int gsh_mcorr_set_high_dynamics_resampler(gsh_mcorr_t* h, int use_high_dynamics_resampler)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        h->high_dyn = use_high_dynamics_resampler != 0;
        return GSH_OK;
    }

    int gsh_mcorr_carrier_wipeoff_multicorrelator_resampler(gsh_mcorr_t* h, float rem_carrier_phase_in_rad, float phase_step_rad,
        float phase_rate_step_rad, float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
        int signal_length_samples)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        return mcorr_run(h, h->high_dyn ? 1 : 0, rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad, rem_code_phase_chips,
            code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples);
    }

    int gsh_mcorr_carrier_wipeoff_multicorrelator_resampler6(gsh_mcorr_t* h, float rem_carrier_phase_in_rad, float phase_step_rad,
        float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips, int signal_length_samples)
    {
        GSH_REQUIRE(h != nullptr, "null handle");
        return mcorr_run(h, h->high_dyn ? 2 : 0, rem_carrier_phase_in_rad, phase_step_rad, 0.0f, rem_code_phase_chips,
            code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples);
    }
}
