/*
 * gnss_sdr_hip.h -- C ABI of the MI355X (gfx950) acquisition + tracking correlator engine.
 *
 * This is the drop-in boundary for gnss-sdr's one data-parallel hot path.  Plain C,
 * plain pointers and sizes, opaque handles, int status returns (0 = GSH_OK); no HIP,
 * torch or C++ types cross it and no exception ever does.  The shared library that
 * implements it is gnss-sdr_amd/libgnss_sdr_hip.so (hand-written HIP, built by
 * __graft_entry__.build()).  There is NO CPU fallback: every entry point that needs the
 * GPU returns GSH_ERR_NO_DEVICE / GSH_ERR_HIP when it cannot run there.
 *
 * Each group of entry points names the reference interface it replaces; paths are
 * relative to the gnss-sdr tree (/root/reference):
 *   mcorr.h  = src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h
 *   mcorr.cc = src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.cc
 *   acq.cc   = src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.cc
 *   acq.h    = src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.h
 *   trk.cc   = src/algorithms/tracking/gnuradio_blocks/dll_pll_veml_tracking.cc
 *
 * Complex samples are interleaved little-endian float32 I,Q everywhere ("iq" pointers
 * address 2*n floats), i.e. gr_complex / std::complex<float> / lv_32fc_t memory.
 */
#ifndef GNSS_SDR_HIP_H
#define GNSS_SDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

#define GSH_ABI_VERSION 25
#define GSH_MAX_TAPS 8 /* VE/E/P/L/VL needs 5 (trk.cc:609-650); 8 leaves room for multi-tap dumps */

    enum
    {
        GSH_OK = 0,
        GSH_ERR_INVALID = 1,   /* bad argument (null pointer, size out of range, taps > GSH_MAX_TAPS ...) */
        GSH_ERR_NO_DEVICE = 2, /* no HIP device / device index out of range */
        GSH_ERR_HIP = 3,       /* a HIP runtime call failed; gsh_last_error() has the text */
        GSH_ERR_STATE = 4,     /* call order violated (e.g. correlate before set_local_code) */
        GSH_ERR_UNSUPPORTED = 5
    };

    /* ------------------------------------------------------------------ library */
    int gsh_abi_version(void);
    int gsh_device_count(void);               /* 0 when no GPU is visible */
    const char* gsh_last_error(void);         /* thread-local, never NULL */
    int gsh_device_name(int device, char* buf, size_t buflen);
    /* diagnostic: streaming-read bandwidth of the device as THIS library's loads see it -- a `bytes`-sized buffer (allocated here; larger than the 256 MiB Infinity
     * Cache to measure HBM) read `reps` times with 16-byte loads by a full grid, HIP-event timed; *gb_per_s = bytes x reps / time.  The figure rooflines are
     * stated against beside the nominal peak. */
    int gsh_probe_read_bandwidth(int device, uint64_t bytes, int reps, double* gb_per_s);

    /* ================================================================== TRACKING
     * (1) gsh_mcorr_*: one-to-one replacement of class Cpu_Multicorrelator_Real_Codes
     *     (mcorr.h:37-61).  Same call order, same argument meaning, same borrowed-pointer
     *     rules as the reference: `shifts_chips`, `corr_out` and `sig_in` are BORROWED
     *     (read / written at every correlate call, mcorr.cc:53-72); the local code is
     *     copied to the device once per set_local_code_and_taps (the reference keeps a
     *     pointer, trk.cc:1030 sets it once per start_tracking).
     *     The reference's bool returns (always true, never checked: mcorr.cc:49,62,71,125)
     *     become int status codes.
     */
    typedef struct gsh_mcorr gsh_mcorr_t;

    int gsh_mcorr_create(int device, gsh_mcorr_t** out);
    void gsh_mcorr_destroy(gsh_mcorr_t* h);

    /* mcorr.cc:36-50  bool init(int max_signal_length_samples, int n_correlators)
     * n_correlators: 1..GSH_MAX_WIDE_TAPS.  A handle with more than GSH_MAX_TAPS correlators runs the wide bank (section 2b), which has the
     * standard resampler only: with the high-dynamics flag set (the object's default, as in the reference) its correlate calls return
     * GSH_ERR_UNSUPPORTED and zero corr_out -- call set_high_dynamics_resampler(false), as dll_pll_veml_tracking and kf_tracking do. */
    int gsh_mcorr_init(gsh_mcorr_t* h, int max_signal_length_samples, int n_correlators);
    /* mcorr.cc:53-63  bool set_local_code_and_taps(int, const float*, float*) */
    int gsh_mcorr_set_local_code_and_taps(gsh_mcorr_t* h, int code_length_chips, const float* local_code_in, float* shifts_chips);
    /* mcorr.cc:66-72  bool set_input_output_vectors(std::complex<float>*, const std::complex<float>*) */
    int gsh_mcorr_set_input_output_vectors(gsh_mcorr_t* h, float* corr_out_iq, const float* sig_in_iq);
    /* mcorr.cc:163-167 void set_high_dynamics_resampler(bool)   (object default: true, mcorr.h:60) */
    int gsh_mcorr_set_high_dynamics_resampler(gsh_mcorr_t* h, int use_high_dynamics_resampler);
    /* mcorr.cc:103-126 bool Carrier_wipeoff_multicorrelator_resampler(7 args): synchronous,
     * corr_out[0..n_correlators) is valid on return. */
    int gsh_mcorr_carrier_wipeoff_multicorrelator_resampler(gsh_mcorr_t* h, float rem_carrier_phase_in_rad,
        float phase_step_rad, float phase_rate_step_rad, float rem_code_phase_chips, float code_phase_step_chips,
        float code_phase_rate_step_chips, int signal_length_samples);
    /* mcorr.cc:129-144 6-argument overload: always the standard rotator, but the code
     * resampler still follows the high-dynamics flag (mcorr.cc:137 calls update_local_code). */
    int gsh_mcorr_carrier_wipeoff_multicorrelator_resampler6(gsh_mcorr_t* h, float rem_carrier_phase_in_rad,
        float phase_step_rad, float rem_code_phase_chips, float code_phase_step_chips,
        float code_phase_rate_step_chips, int signal_length_samples);
    /* mcorr.cc:147-160 bool free() */
    int gsh_mcorr_free(gsh_mcorr_t* h);

    /*
     * (2) gsh_bank_*: the batched form the GPU wants -- one launch serves every
     *     (channel, epoch) "job" that is ready.  A job is exactly one reference
     *     Carrier_wipeoff_multicorrelator_resampler call (mcorr.cc:103-126) whose input
     *     window is addressed by sample index inside a device-resident IF stream instead
     *     of a host pointer, so each sample crosses PCIe / xGMI once, not once per channel.
     */
    typedef struct gsh_bank gsh_bank_t;

    typedef struct gsh_corr_job
    {
        uint64_t sample_offset;      /* first sample of the window inside the attached stream */
        int32_t n_samples;           /* signal_length_samples, trk.cc:1243 passes vector_length */
        int32_t code_slot;           /* which uploaded local code (one per channel / PRN) */
        float rem_carr_phase_rad;    /* mcorr.cc:104 */
        float phase_step_rad;        /* mcorr.cc:105 */
        float phase_rate_step_rad;   /* mcorr.cc:106 (used only when high_dyn) */
        float rem_code_phase_chips;  /* mcorr.cc:107, already multiplied by samples-per-chip (trk.cc:1240) */
        float code_phase_step_chips; /* mcorr.cc:108 */
        float code_phase_rate_step_chips; /* mcorr.cc:109 (used only when high_dyn) */
        int32_t n_taps;              /* 1..GSH_MAX_TAPS */
        int32_t high_dyn;            /* 0: resampler_32f_xn + rotator_dot_prod; 1: the high-dynamics pair */
        float shifts_chips[GSH_MAX_TAPS]; /* tap offsets in code samples, ascending (trk.cc:632-648) */
    } gsh_corr_job;                  /* 80 bytes, POD */

    int gsh_bank_create(int device, int n_code_slots, int max_code_length, gsh_bank_t** out);
    void gsh_bank_destroy(gsh_bank_t* b);
    /* copy one real-valued local code (trk.cc:810-1028 generate it) into slot `slot` */
    int gsh_bank_set_code(gsh_bank_t* b, int slot, const float* code, int code_length);
    /* IF sample stream.  _host copies n samples to the device (H2D);
     * _device borrows device memory the caller keeps alive (16-byte aligned). */
    int gsh_bank_set_stream_host(gsh_bank_t* b, const float* iq, uint64_t n_samples);
    int gsh_bank_set_stream_device(gsh_bank_t* b, const void* device_iq, uint64_t n_samples);
    /* one synchronous batch: upload jobs, launch, download.  out_iq: n_jobs*GSH_MAX_TAPS complex64
     * (job-major, tap-minor; taps >= n_taps are zero). */
    int gsh_bank_correlate(gsh_bank_t* b, const gsh_corr_job* jobs, int n_jobs, float* out_iq);
    /* the same, split so that a caller can keep the job table and results on the device and
     * time launches alone: upload once, launch many, read once.  hip_stream: a hipStream_t cast to
     * void* (NULL = the bank's own stream).  gsh_bank_launch is asynchronous. */
    /* Pair fusion (default on): a single-tap job placed directly after a job with the same window and the same NCO parameters -- the
     * data-component prompt that track_pilot adds to a pilot channel (trk.cc:1246-1256: a second correlator object over the same
     * samples) -- is computed by that job's work-groups while they hold the rotated samples, instead of a second pass over the window.
     * Results are unchanged (each tap is the same sum over the same products in the same order); 0 disables it for A/B runs. */
    int gsh_bank_set_pair_fusion(gsh_bank_t* b, int enable);
    int gsh_bank_upload_jobs(gsh_bank_t* b, const gsh_corr_job* jobs, int n_jobs);
    int gsh_bank_launch(gsh_bank_t* b, void* hip_stream);
    int gsh_bank_synchronize(gsh_bank_t* b);
    int gsh_bank_read_outputs(gsh_bank_t* b, float* out_iq, int n_jobs);
    /* HIP-event timing of `reps` back-to-back launches of the uploaded job table on the bank's
     * stream: average milliseconds per launch of the correlator kernel. */
    int gsh_bank_time_launches(gsh_bank_t* b, int reps, float* avg_ms);
    /* work-groups per job used by the next launches (1 = throughput mode; >1 spreads one epoch
     * over more CUs for latency-bound closed-loop use).  0 = choose automatically. */
    int gsh_bank_set_splits(gsh_bank_t* b, int splits);
    /* diagnostics of the E/P/L correlator's walk (one resident round of work-groups, each walking several jobs: csrc/mcorr_kernels.h):
     * the work-groups of that kernel the calling thread's current device holds at once (0: unknown, no launch walks of its own accord),
     * and how many launches of this process have taken the walk so far. */
    int gsh_mcorr_walk_capacity(void);
    uint64_t gsh_mcorr_walk_launches(void);
    /* an offset (in samples) added to every job's sample_offset at launch time: a job table uploaded once -- window positions relative to
     * the start of a block -- serves block after block of a long stream or of a ring (positions are taken modulo the ring's capacity)
     * without being re-staged and re-uploaded every time.  The caller keeps the shifted windows inside the stream / resident in the ring. */
    int gsh_bank_set_sample_base(gsh_bank_t* b, uint64_t sample_base);

    /*
     * (2b) The wide bank: a sampled correlation function -- up to GSH_MAX_WIDE_TAPS taps per job in one pass over the window (multipath
     *     estimation, signal-quality monitoring, side-peak monitoring), where gsh_corr_job stops at GSH_MAX_TAPS.  Every tap is one output
     *     of one reference Carrier_wipeoff_multicorrelator_resampler call in STANDARD mode (the standard resampler and rotator: what
     *     high_dyn = 0 means in gsh_corr_job); the high-dynamics modes exist for up to GSH_MAX_TAPS taps only.  Chip selection is bit-exact
     *     per tap for any ascending shifts (duplicates, spans wider than a code period, negative raw indices).  A job's output bits depend
     *     on the job record, the code, the samples and an explicit gsh_bank_set_splits value -- never on the other jobs of the batch.
     *     Same bank, same codes, same stream attachment (host, device or ring) and sample base as the narrow calls, whose staged job
     *     table these calls leave alone.
     */
#define GSH_MAX_WIDE_TAPS 64
    typedef struct gsh_corr_job_wide
    {
        uint64_t sample_offset;      /* as in gsh_corr_job (ring-bound banks: an absolute sample index) */
        int32_t n_samples;
        int32_t code_slot;
        float rem_carr_phase_rad;
        float phase_step_rad;
        float rem_code_phase_chips;
        float code_phase_step_chips;
        int32_t n_taps;              /* 1..GSH_MAX_WIDE_TAPS */
        int32_t reserved;            /* 0 */
        float shifts_chips[GSH_MAX_WIDE_TAPS]; /* tap offsets in code samples, ascending (equal neighbours allowed) */
    } gsh_corr_job_wide;             /* 296 bytes, POD */
    /* one synchronous batch: upload jobs, launch, download.  out_iq: n_jobs * GSH_MAX_WIDE_TAPS complex64 (job-major, tap-minor; taps >= n_taps
     * are zero).  Jobs of different tap counts may share a batch; n_jobs == 0 is a no-op.  Every job is validated before anything runs
     * (GSH_ERR_INVALID / GSH_ERR_STATE with the job's index in gsh_last_error()): an empty code slot, a window past the stream or not resident
     * in the ring, n_taps outside 1..GSH_MAX_WIDE_TAPS, descending shifts, parameters that are not finite. */
    int gsh_bank_correlate_wide(gsh_bank_t* b, const gsh_corr_job_wide* jobs, int n_jobs, float* out_iq);
    /* upload `jobs` once, then HIP-event timing of `reps` back-to-back launches on the bank's stream: average milliseconds per launch
     * (the wide counterpart of gsh_bank_upload_jobs + gsh_bank_time_launches) */
    int gsh_bank_time_launches_wide(gsh_bank_t* b, const gsh_corr_job_wide* jobs, int n_jobs, int reps, float* avg_ms);

    /*
     * (3) The 16-bit family: gsh_mcorr16_* replaces class Cpu_Multicorrelator_16sc
     *     (src/algorithms/tracking/libs/cpu_multicorrelator_16sc.h:38-57, .cc:25-120) method for method, gsh_bank16_* is its batched form.
     *     Samples, local code and correlator outputs are complex int16 (lv_16sc_t: interleaved I, Q).  Results are those of the reference's
     *     generic protokernels BIT FOR BIT (K/volk_gnsssdr_16ic_xn_resampler_16ic_xn.h:60-78, K/volk_gnsssdr_16ic_x2_rotator_dot_prod_16ic_xn.h:66-102):
     *     float32 rotation rounded to int16 per sample, the phasor recurrence with its renormalisation every 256 samples, integer products kept
     *     to 16 bits, sums that saturate at every addition in sample order.  (The reference's SSE / AVX2 protokernels of the same kernel differ
     *     from its generic one by a few units -- four interleaved partial sums, another phase schedule; the generic one is what its QA compares
     *     against and what is reproduced here.)  No block of the reference instantiates this class; it is built for completeness of the family.
     */
    typedef struct gsh_mcorr16 gsh_mcorr16_t;
    int gsh_mcorr16_create(int device, gsh_mcorr16_t** out);
    void gsh_mcorr16_destroy(gsh_mcorr16_t* h);
    /* cpu_multicorrelator_16sc.cc:25-41  bool init(int max_signal_length_samples, int n_correlators) */
    int gsh_mcorr16_init(gsh_mcorr16_t* h, int max_signal_length_samples, int n_correlators);
    /* .cc:44-53  bool set_local_code_and_taps(int, const lv_16sc_t*, float*): the code is copied to the device, `shifts_chips` is BORROWED and re-read at every call */
    int gsh_mcorr16_set_local_code_and_taps(gsh_mcorr16_t* h, int code_length_chips, const int16_t* local_code_in_iq, float* shifts_chips);
    /* .cc:56-62  bool set_input_output_vectors(lv_16sc_t* corr_out, const lv_16sc_t* sig_in): both BORROWED */
    int gsh_mcorr16_set_input_output_vectors(gsh_mcorr16_t* h, int16_t* corr_out_iq, const int16_t* sig_in_iq);
    /* .cc:80-96  bool Carrier_wipeoff_multicorrelator_resampler(5 args): synchronous, corr_out[0 .. n_correlators) valid on return */
    int gsh_mcorr16_carrier_wipeoff_multicorrelator_resampler(gsh_mcorr16_t* h, float rem_carrier_phase_in_rad, float phase_step_rad, float rem_code_phase_chips,
        float code_phase_step_chips, int signal_length_samples);
    /* .cc:107-120 bool free() */
    int gsh_mcorr16_free(gsh_mcorr16_t* h);

    typedef struct gsh_bank16 gsh_bank16_t;
    typedef struct gsh_corr16_job
    {
        uint64_t sample_offset;      /* first sample of the window inside the attached int16 stream */
        int32_t n_samples;           /* signal_length_samples */
        int32_t code_slot;
        float rem_carr_phase_rad;    /* .cc:81 */
        float phase_step_rad;        /* .cc:82 */
        float rem_code_phase_chips;  /* .cc:83 */
        float code_phase_step_chips; /* .cc:84 */
        int32_t n_taps;              /* 1..GSH_MAX_TAPS */
        int32_t reserved;
        float shifts_chips[GSH_MAX_TAPS];
    } gsh_corr16_job;                /* 72 bytes, POD */
    int gsh_bank16_create(int device, int n_code_slots, int max_code_length, gsh_bank16_t** out);
    void gsh_bank16_destroy(gsh_bank16_t* b);
    int gsh_bank16_set_code(gsh_bank16_t* b, int slot, const int16_t* code_iq, int code_length);
    /* the IF stream as complex int16: _host copies it to the device, _device borrows device memory (4-byte aligned) */
    int gsh_bank16_set_stream_host(gsh_bank16_t* b, const int16_t* iq, uint64_t n_samples);
    int gsh_bank16_set_stream_device(gsh_bank16_t* b, const void* device_iq, uint64_t n_samples);
    /* one synchronous batch; out_iq: n_jobs * GSH_MAX_TAPS complex int16 (job-major, tap-minor; taps >= n_taps are zero).  The two carrier phasors of
     * every job are formed on the host with the C library, by the expressions of cpu_multicorrelator_16sc.cc:89-93. */
    int gsh_bank16_correlate(gsh_bank16_t* b, const gsh_corr16_job* jobs, int n_jobs, int16_t* out_iq);
    /* the same in pieces (upload once, launch many, read once); gsh_bank16_launch is asynchronous on the bank's stream */
    int gsh_bank16_upload_jobs(gsh_bank16_t* b, const gsh_corr16_job* jobs, int n_jobs);
    int gsh_bank16_launch(gsh_bank16_t* b);
    int gsh_bank16_read_outputs(gsh_bank16_t* b, int16_t* out_iq, int n_jobs);
    /* HIP-event timing of `reps` back-to-back launches (both kernels) of the uploaded job table: average milliseconds per launch */
    int gsh_bank16_time_launches(gsh_bank16_t* b, int reps, float* avg_ms);

    /* ================================================================ SAMPLE STREAM (device-resident ring)
     * gsh_stream_*: the IF sample stream of one RF front-end kept in device memory, addressed by ABSOLUTE sample index
     * (sample 0 = the first sample ever pushed), so that every channel's correlation window refers to bytes that crossed
     * PCIe / xGMI once.  In the reference every tracking / acquisition block reads the same GNU Radio buffer
     * (gnss_flowgraph.cc:1227-1231); this is that buffer's device-side twin.  Raw front-end formats are converted on the
     * device with the arithmetic of the reference's data_type_adapter blocks (ibyte_to_complex.cc:45-51,
     * ishort_to_complex.cc:45-51: integer -> float cast, no scaling; inverted_spectrum -> conjugate).
     * The ring keeps the last `capacity_samples`; any window of up to `max_window_samples` is contiguous in device
     * memory (the first max_window samples are mirrored behind the end), so the correlator kernels never wrap. */
    typedef struct gsh_stream gsh_stream_t;
    enum gsh_item_type
    {
        GSH_ITEM_GR_COMPLEX = 0, /* interleaved float32 I,Q (gr_complex), 8 bytes per sample */
        GSH_ITEM_SHORT = 1,      /* interleaved int16 I,Q (item_type ishort / cshort), 4 bytes per sample */
        GSH_ITEM_BYTE = 2        /* interleaved int8 I,Q (item_type ibyte / cbyte), 2 bytes per sample */
    };
    int gsh_stream_create(int device, uint64_t capacity_samples, uint32_t max_window_samples, gsh_stream_t** out);
    /* Destroying a ring that tracking handles are bound to (gsh_trk_set_stream_ring) tells those handles -- a live residency on it is wound down first, then the
     * memory goes -- but it is NOT synchronised against other threads' calls on those handles or against their destruction: the caller keeps gsh_stream_destroy
     * from racing with gsh_trk_* calls on handles bound to the ring (Hip_Tracking_Runtime does, under its handle mutex). */
    void gsh_stream_destroy(gsh_stream_t* s);
    /* append n samples held in host memory; *first_index (may be NULL) receives the absolute index of items[0].
     * Synchronous: the samples are resident (and any older ones they displace are gone) on return. */
    int gsh_stream_push(gsh_stream_t* s, const void* items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    /* the same with the items already in device memory (e.g. a block received over RCCL); the conversion is queued on
     * `hip_stream` (a hipStream_t cast to void*, NULL = the ring's own stream and synchronous) */
    int gsh_stream_push_device(gsh_stream_t* s, const void* device_items, uint64_t n, int item_type, int inverted_spectrum, void* hip_stream,
        uint64_t* first_index);
    /* [*oldest, *next): the absolute sample indices currently resident */
    /* Asynchronous ingest: the host-to-device copy and the conversion are queued on the ring's own stream and the call returns at once, so
     * the next block travels over PCIe while the correlators (which wait on the ring's event, not on the host) work on the previous one
     * (the reference's flowgraph streams continuously, gnss_flowgraph.cc:1227-1231).  `items` must stay valid and unmodified until
     * gsh_stream_wait() returns or two further pushes have been issued; pinned (page-locked) host memory makes the copy a true DMA.
     * Two device staging buffers alternate.  The caller keeps the ring from lapping its readers: a push may only overwrite samples no
     * queued launch still reads (capacity >= everything in flight). */
    int gsh_stream_push_async(gsh_stream_t* s, const void* items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_wait(gsh_stream_t* s);  /* host waits for every queued push */
    /* Asynchronous ingest out of memory the caller wants back at once (a GNU Radio input buffer): the items are copied into page-locked
     * staging memory owned by the ring (four buffers in rotation), from where the copy to the device and the conversion are queued on the
     * ring's stream; `items` may be reused as soon as the call returns.  Readers wait on the ring's events as for every other push. */
    int gsh_stream_push_staged(gsh_stream_t* s, const void* items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    /* The same for items that already lie in page-locked host memory (gsh_host_register, or memory the caller allocated page-locked): no staging
     * copy on the host -- the DMA engine reads `items` directly -- and the call returns when that DMA has finished (the conversion into the ring
     * stays queued), so `items` may be re-used on return.  This is the path for a GNU Radio input buffer: the scheduler re-uses the same buffer
     * for the whole run, so registering it once makes every later push a true DMA. */
    int gsh_stream_push_pinned(gsh_stream_t* s, const void* items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    /* the same in two halves: _async queues the DMA and the conversion and returns at once; gsh_stream_wait_copied blocks until every DMA queued
     * so far has read its source (`items` of every earlier _async call may be re-used then).  wait_copied touches none of the ring's bookkeeping and
     * may be called WITHOUT the serialisation the other entry points need -- a caller that guards the ring with a lock queues under the lock and
     * waits outside it, so that launches which read the ring are queued while the DMA runs. */
    int gsh_stream_push_pinned_async(gsh_stream_t* s, const void* items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_wait_copied(gsh_stream_t* s);
    /* ... and for a caller that gets its memory back piece by piece (a GNU Radio block returns input to the scheduler only up to what it consumes): blocks
     * until every push that covers samples below end_index has been read out of the caller's memory (and has reached the ring); pushes queued behind
     * those may still be in flight.  *complete_upto (may be NULL): the index up to which the ring is now known to be complete.  Any thread. */
    int gsh_stream_wait_copied_upto(gsh_stream_t* s, uint64_t end_index, uint64_t* complete_upto);
    /* page-lock / release a range of host memory for DMA (hipHostRegister / hipHostUnregister behind the ABI: host code above it has no HIP headers).
     * The range must be mapped; registering pages twice fails with GSH_ERR_HIP. */
    int gsh_host_register(int device, void* ptr, size_t bytes);
    int gsh_host_unregister(void* ptr);
    /* position an (idle) ring: the next pushed sample gets absolute index next_index and nothing older is resident -- a channel that
     * starts hours into a run does not have to fill the ring from index 0 */
    int gsh_stream_seek(gsh_stream_t* s, uint64_t next_index);
    /* ---- one block, N GPUs: replication of the IF sample block into N device rings over RCCL / xGMI.
     * Channels / PRNs shard over the GPUs of a node; they all read the same stream (gnss_flowgraph.cc:1227-1231), so every block enters ONE
     * GPU -- rank 0, the ingest GPU -- in the front-end's raw item format and is replicated to the others, each converting it to complex64
     * into its own ring.  GSH_GROUP_BROADCAST: ncclBroadcast.  GSH_GROUP_SCATTER_ALLGATHER: rank 0 sends a different 1/N to every peer over
     * all its xGMI links at once, then an all-gather completes the block (xGMI is point to point: every link carries block/N twice instead
     * of one link carrying the whole block per hop).  The rings are ordinary gsh_stream_t: banks, loops and acquisition handles bind to
     * them as usual and wait on their events; nothing here synchronises the host.  A push is queued on the rings' own streams; consecutive
     * pushes alternate between two staging buffers.  Ring capacity must cover what is in flight (see gsh_stream_push_async). */
    typedef struct gsh_stream_group gsh_stream_group_t;
#define GSH_GROUP_BROADCAST 0
#define GSH_GROUP_SCATTER_ALLGATHER 1
/* OR'ed into `mode`: a group of ONE rank normally needs no exchange and never touches RCCL; with this flag it builds its communicator
 * (ncclCommInitAll / ncclCommInitRank with one rank) and sends every block through the mode's collectives all the same -- ncclBroadcast, or
 * the grouped ncclSend / ncclRecv to itself + ncclAllGather -- so that the dlopen, the hand-declared signatures and the stream ordering can be
 * exercised on a single-GPU box.  The environment variable GSH_GROUP_FORCE_RCCL=1 sets it for every group of one.  No effect on world > 1. */
#define GSH_GROUP_FORCE_RCCL 0x100
    /* one process drives all n_devices GPUs (ncclCommInitAll); local ring i belongs to devices[i], rank i */
    int gsh_stream_group_create(const int* devices, int n_devices, uint64_t capacity_samples, uint32_t max_window_samples, int mode, gsh_stream_group_t** out);
    /* one process per GPU: id128 = 128 bytes from gsh_comm_unique_id() on one rank, handed to every rank by whoever launched them
     * (environment, file, MPI, torch.distributed's store ... -- control plane only) */
    int gsh_comm_unique_id(void* id128);
    int gsh_stream_group_create_rank(int device, int rank, int world, const void* id128, uint64_t capacity_samples, uint32_t max_window_samples, int mode,
        gsh_stream_group_t** out);
    void gsh_stream_group_destroy(gsh_stream_group_t* g);
    int gsh_stream_group_size(const gsh_stream_group_t* g);                       /* local rings */
    gsh_stream_t* gsh_stream_group_ring(gsh_stream_group_t* g, int local_index);  /* owned by the group */
    /* every rank calls it for every block (a collective); the process that owns rank 0 supplies the block (host memory, or -- _device --
     * memory on rank 0's GPU), the others pass NULL */
    int gsh_stream_group_push(gsh_stream_group_t* g, const void* host_items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_group_push_device(gsh_stream_group_t* g, const void* device_items, uint64_t n, int item_type, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_group_wait(gsh_stream_group_t* g);
    /* what the group has done with RCCL so far: *rccl_ranks = ranks of the communicator(s) the group created (0: none -- a group of one without
     * GSH_GROUP_FORCE_RCCL), *rccl_version = ncclGetVersion's code (0 when RCCL was never loaded), *collectives = RCCL collective / point-to-point
     * calls this group has issued (broadcasts, sends, receives, all-gathers).  Any pointer may be NULL. */
    int gsh_stream_group_rccl_info(const gsh_stream_group_t* g, int32_t* rccl_ranks, int32_t* rccl_version, uint64_t* collectives);
    /* the exchange plan of ONE rank for one block of `bytes` raw bytes: the list of collective / point-to-point operations gsh_stream_group_push issues
     * for it, in order -- the single place where chunk sizes, offsets and peers are decided (the push walks this very list).  Operations of the same
     * `phase` go out between one ncclGroupStart / ncclGroupEnd.  Buffers: STAGE = the rank's staging buffer of *padded_bytes (the block, zero-extended to
     * world x chunk, chunk a multiple of 16), PIECE = its chunk-sized scratch.  Needs no GPU: a launcher can size its messages from it, the CPU suite
     * executes it over torch.distributed / gloo (tests/test_sharding_gloo.py).  ops may be NULL (count only). */
#define GSH_GROUP_OP_BROADCAST 0 /* ncclBroadcast(src, dst, bytes, root = peer) */
#define GSH_GROUP_OP_SEND 1      /* ncclSend(src, bytes, peer) */
#define GSH_GROUP_OP_RECV 2      /* ncclRecv(dst, bytes, peer) */
#define GSH_GROUP_OP_ALLGATHER 3 /* ncclAllGather(src, dst, bytes per rank) */
#define GSH_GROUP_BUF_NONE 0
#define GSH_GROUP_BUF_STAGE 1
#define GSH_GROUP_BUF_PIECE 2
    typedef struct
    {
        int32_t op;
        int32_t peer;
        int32_t phase;
        int32_t src_buf, dst_buf;
        uint64_t src_offset, dst_offset;
        uint64_t bytes;
    } gsh_group_op_t;
    int gsh_stream_group_plan(uint64_t bytes, int world, int rank, int mode, gsh_group_op_t* ops, int max_ops, int* n_ops, uint64_t* padded_bytes);
    /* the collective library in use: file name of the loaded librccl (the system's, or what the environment variable GSH_RCCL_LIBRARY names -- a site's own
     * build, or the test-only stand-in tests/host/libfake_rccl.so with which the N > 1 paths run on a one-GPU box).  GSH_RCCL_LIBRARY is read whenever a
     * group or an id is made; it must not change while a group made with the other library is alive. */
    int gsh_comm_library(char* path, int capacity);
    int gsh_stream_range(gsh_stream_t* s, uint64_t* oldest, uint64_t* next);
    /* copy resident samples [index, index + n) back to the host as complex64 (tests, dumps) */
    int gsh_stream_read(gsh_stream_t* s, uint64_t index, uint64_t n, float* out_iq);
    /* stand-alone conversion of n device-resident items to complex64 (device_dst 8-byte aligned), asynchronous on hip_stream */
    int gsh_convert_samples_device(int device, const void* device_items, int item_type, int inverted_spectrum, void* device_dst, uint64_t n,
        void* hip_stream);
    /* ---- packed 2-bit / 4-bit front-end samples, unpacked on the device with the arithmetic of the reference's unpack blocks
     * (src/algorithms/signal_source/gnuradio_blocks/unpack_*.cc) followed by the GNU Radio conversion the signal source puts behind them.
     * Paths below: adapters/ = src/algorithms/signal_source/adapters/, blocks/ = src/algorithms/signal_source/gnuradio_blocks/.
     *   GSH_PACKED_TWO_BIT       Two_Bit_Packed_File_Signal_Source (adapters/two_bit_packed_file_signal_source.cc:38-145): blocks/unpack_2bit_samples.cc
     *                            (2s + 1 of each signed 2-bit field), then char_to_float (real) or interleaved_char_to_complex (iq / qi).
     *   GSH_PACKED_TWO_BIT_CPX   Two_Bit_Cpx_File_Signal_Source (adapters/two_bit_cpx_file_signal_source.cc:72-81): blocks/unpack_byte_2bit_cpx_samples.cc,
     *                            then interleaved_short_to_complex(false, true).  Complex, 2 samples per byte.
     *   GSH_PACKED_FOUR_BIT_CPX  Four_Bit_Cpx_File_Signal_Source (adapters/four_bit_cpx_file_signal_source.cc:38-55,118-121): blocks/unpack_byte_4bit_samples.cc,
     *                            then interleaved_short_to_complex(false, qi).  Complex, 1 sample per byte.
     *   GSH_PACKED_NSR           Nsr_File_Signal_Source (adapters/nsr_file_signal_source.cc:69-76): blocks/unpack_byte_2bit_samples.cc, real float -2..1,
     *                            4 samples per byte.
     *   GSH_PACKED_NTLAB         NTLab_File_Signal_Source (adapters/ntlab_file_signal_source.cc:41-45,88,100-127): blocks/unpack_ntlab_2bit_samples.cc,
     *                            sign / magnitude +-1 / +-3, one real stream per RF channel; RF_channels = 4 only (1 and 2 are refused: the
     *                            reference block reads past its input there, blocks/unpack_ntlab_2bit_samples.cc:38,57-77).
     *   GSH_PACKED_GSS6450_2BIT  Spir_GSS6450_File_Signal_Source (adapters/spir_gss6450_file_signal_source.cc:46-55,69-98,183-233) with adc_bits 2 / 4:
     *   GSH_PACKED_GSS6450_4BIT  32-bit little-endian words dealt round-robin over total_channels RF bands (deinterleave of 4-byte items: word k
     *                            belongs to band k mod total_channels), every word byte-reversed first when `endian` is set (endian_swap(4)), then
     *                            blocks/unpack_spir_gss6450_samples.cc:39-122: 8 (2-bit) or 4 (4-bit) complex samples per word, sample 0 in the top
     *                            nibble / byte, I in the low half of the field and Q in the high half, two's complement, no 2s + 1.  Complex; a
     *                            packed buffer starts at a frame boundary (band 0's word).  GNU Radio's deinterleave and endian_swap are restated
     *                            from their documented behaviour.
     *   GSH_PACKED_LABSAT_2BIT   Labsat_Signal_Source, LabSat 2 / LabSat 3 files with one RF channel (blocks/labsat23_source.cc:363-583 parse_header,
     *   GSH_PACKED_LABSAT_4BIT   :586-658 decode_samples_one_channel): 16-bit little-endian items.  2 bits per sample: 8 complex samples per item, sample i
     *                            has I = bit 15 - 2i, Q = bit 14 - 2i, value 2 b - 1.  4 bits: 4 samples per item, I sign = bit 15 - 4i, Q sign = bit
     *                            14 - 4i, I magnitude = bit 13 - 4i, Q magnitude = bit 12 - 4i; (sign, magnitude) 00 -> +1, 01 -> +2, 11 -> -1, 10 -> -2.
     *   GSH_PACKED_LS3W_1BIT     Labsat_Signal_Source, LabSat 3 Wideband (.ls3w) with QUA = 1 / 2 / 3 bits each for I and Q and rf_channels = CHN (1..3)
     *   GSH_PACKED_LS3W_2BIT     RF channels: a run of 64-bit little-endian registers of spr samples of EVERY channel (blocks/labsat23_source.cc:954-1034
     *   GSH_PACKED_LS3W_3BIT     number_of_samples_per_ls3w_register; without / with digital I/O recorded):
     *                                QUA 1: CHN 1 32 / 30, CHN 2 16 / 15, CHN 3 10 / 10
     *                                QUA 2: CHN 1 16 / 15, CHN 2  8 /  7, CHN 3  5 /  5
     *                                QUA 3: CHN 1 10 / 10, CHN 2  5 /  5, CHN 3  3 /  3
     *                            With SFT = 2 QUA CHN, spare = 64 - spr SFT bits (0, 4, 8 or 10) at the TOP of the register are not samples.  Sample i
     *                            of channel c starts o = spare + i SFT + 2 QUA c bits below the top (:944-948,1037-1053): the I code is bits 63 - o ..
     *                            63 - o - QUA + 1, most significant first, the Q code the next QUA bits.  Value (generate_mapping, :43-62), half =
     *                            2^(QUA-1): code < half -> (code + 1) / half, else (code - 2^QUA) / half; every value is a multiple of 0.25.
     *                            DEVIATION: the reference as compiled cannot be used as the yardstick here.  Its extract_bits (:67-74) indexes
     *                            bs[64 - start - i + 1], bit 65 - start - i: outside the 64-bit std::bitset for offsets 0 and 1 (undefined behaviour)
     *                            and elsewhere two bits above the position that the surrounding code implies (:1039 "Earlier samples are written in the
     *                            MSBs", the spare bits counted from the top, the LabSat 4 path taking "48 MSBs" with offsets 0 and 24).  This library
     *                            reads bit 63 - start - i.  Not covered: two-channel LabSat 2 / 3 files (refused by the reference, :496-500) and
     *                            throttling.  (The host's file handling -- the _0000.LS3 sequence, the .ini files, seconds_to_skip -- is the Python
     *                            reader LabSatRecording.)
     *   GSH_PACKED_LS4_1BIT      Labsat_Signal_Source, LabSat 4 (.ls4) with QUA = 1 / 2 / 4 / 8 / 12 bits each for I and Q (blocks/labsat23_source.cc:716;
     *   GSH_PACKED_LS4_2BIT      :92-121 write_samples_ls4, :1262-1301 read_ls4_data / parse_ls4_data).  A LAYOUT is (QUA, regs[3]): regs[s] is the number
     *   GSH_PACKED_LS4_4BIT      of 64-bit little-endian registers of channel slot s (A, B, C) per round, BUF_SIZE_s / 8 of the .ini (:836-857), 0 for a
     *   GSH_PACKED_LS4_8BIT      slot that is not recorded.  The file is a run of ROUNDS: a round is the buffers of the recorded slots in the order A, B,
     *   GSH_PACKED_LS4_12BIT     C, 8 x (regs[0] + regs[1] + regs[2]) bytes, and the buffers may differ in size (bandwidth divisors).  A packed block is
     *                            a whole number of rounds and starts at a round boundary.  Inside one slot's buffer the registers form ONE bit stream,
     *                            register 0 first, every register from its most significant bit down: sample j of the round starts at bit 2 QUA j, its
     *                            I code is the first QUA bits, most significant first, its Q code the next QUA.  For QUA <= 8 a register holds 32 / QUA
     *                            whole samples; at QUA 12 three registers hold 8 samples and samples 2 and 5 of such a triple straddle two registers
     *                            (:92-121).  So slot s has S_s = regs[s] 32 / QUA samples per round, and its sample k lies in round k / S_s at j = k % S_s.
     *                            Value: generate_mapping as for LS3W, half = 2^(QUA-1): code < half -> (code + 1) / half, else (code - 2^QUA) / half;
     *                            every value is a multiple of 1 / half, exact in float32.  The reference requires BUF_SIZE_s BW_DIV_s to be equal over
     *                            the slots (:866-888) and advances slot s by regs_per_output (div_selected / div_s) per output (:908-919,1262-1269), so
     *                            every buffer of a round is used up at the same output: the format is defined by the layout alone and the descriptor
     *                            carries no bandwidth divisor.  Descriptor: item_size 8, sample_type IQ, rf_channels = the slots described (1..3),
     *                            channel = the selected slot (its regs > 0), and the three register counts in the fields that every other register
     *                            family requires to be 0: big_endian_bytes = regs[A], big_endian_items = regs[B], reserved = regs[C] (0 .. 2^20 each, 0
     *                            for a slot at or above rf_channels).  Sample counts are samples of the selected slot: whole registers (QUA <= 8) or
     *                            whole triples (QUA 12); a count may end inside a round, and gsh_packed_bytes returns the bytes of the rounds touched.
     *                            Multi-band as LS3W: one pass over the rounds writes up to three slots, which must hold EQUAL regs (the reference refuses
     *                            to select channels of different bandwidth together, :898-906).  DEVIATIONS: bit i of a field at offset `start` is bit
     *                            63 - start - i, as for LS3W; QUA 12 with regs[s] not a multiple of 3 is refused (the reference reads past the buffer
     *                            there, :106-120 with data_index % data.size()).
     *   GSH_PACKED_SPIR_1BIT     Spir_File_Signal_Source (adapters/spir_file_signal_source.cc:50-58): blocks/unpack_intspir_1bit_samples.cc:36-68 with one
     *                            channel: one complex sample per 32-bit little-endian int, I = bit 0, Q = bit 1, +32767 when set and -32767 when clear.
     * The eleven families above are complex (sample_type IQ), take big_endian_bytes = big_endian_items = 0 (LS4: its register counts instead), and their
     * blocks are whole items / registers whose base is aligned to the item (2, 8, 8 and 4 bytes).  The LS3W and LS4 families are multi-band, as GSS6450.
     * The real families (TWO_BIT with sample_type real, NSR, NTLAB) are IF samples: they enter a ring through a packed FIR (gsh_fir_create_packed)
     * and gsh_stream_push_device, never directly.  Sample counts are samples of ONE RF channel and must be whole input items (the reference blocks
     * are sync_interpolators: they consume whole items).  Zero-initialise the descriptor and set what applies. */
#define GSH_PACKED_TWO_BIT 1
#define GSH_PACKED_TWO_BIT_CPX 2
#define GSH_PACKED_FOUR_BIT_CPX 3
#define GSH_PACKED_NSR 4
#define GSH_PACKED_NTLAB 5
#define GSH_PACKED_GSS6450_2BIT 6
#define GSH_PACKED_GSS6450_4BIT 7
#define GSH_PACKED_LABSAT_2BIT 8
#define GSH_PACKED_LABSAT_4BIT 9
#define GSH_PACKED_LS3W_1BIT 10
#define GSH_PACKED_LS3W_2BIT 11
#define GSH_PACKED_LS3W_3BIT 12
#define GSH_PACKED_SPIR_1BIT 13
#define GSH_PACKED_LS4_1BIT 14
#define GSH_PACKED_LS4_2BIT 15
#define GSH_PACKED_LS4_4BIT 16
#define GSH_PACKED_LS4_8BIT 17
#define GSH_PACKED_LS4_12BIT 18
#define GSH_PACKED_REAL 0 /* sample_type "real" */
#define GSH_PACKED_IQ 1   /* sample_type "iq" */
#define GSH_PACKED_QI 2   /* sample_type "qi" */
    typedef struct
    {
        int32_t family;           /* GSH_PACKED_TWO_BIT .. GSH_PACKED_LS4_12BIT (the SignalSource.implementation) */
        int32_t sample_type;      /* TWO_BIT: "sample_type", default real (two_bit_packed_file_signal_source.cc:39); FOUR_BIT_CPX: iq / qi, default iq
                                   * (four_bit_cpx_file_signal_source.cc:38); REAL for NSR and NTLAB; IQ for TWO_BIT_CPX */
        int32_t item_size;        /* TWO_BIT: 1 ("item_type" byte, the default of FileSourceBase) or 2 (short); GSS6450: 4 (the 32-bit word); LABSAT: 2;
                                   * LS3W, LS4: 8 (the register); SPIR: 4; every other family: 1 */
        int32_t big_endian_bytes; /* TWO_BIT: "big_endian_bytes", default false (two_bit_packed_file_signal_source.cc:41): sample order within a byte reversed;
                                   * LS4: regs[A], the registers of slot A per round (BUF_SIZE_A / 8) */
        int32_t big_endian_items; /* TWO_BIT: "big_endian_items", default true (:40): with item_size 2 the two bytes of an item swap first; little-endian
                                   * short items are read as bytes (:63-77).  GSS6450: "endian", default false (spir_gss6450_file_signal_source.cc:51): the
                                   * four bytes of every word are reversed before unpacking.  LS4: regs[B], the registers of slot B per round */
        int32_t rf_channels;      /* NTLAB: "RF_channels", default 4 (ntlab_file_signal_source.cc:41-42), 4 only; GSS6450: "total_channels", 1..8 (0 reads as
                                   * 1); LS3W: CHN, 1..3; LS4: the channel slots described, 1..3; every other family: 0 or 1 */
        int32_t channel;          /* NTLAB: the RF channel unpacked by gsh_unpack_device / the packed FIR (0..3); GSS6450: the band the single-channel calls
                                   * take, "sel_ch" - 1; LS3W: "selected_channel" - 1 (0..2); LS4: the selected slot (0..2, recorded); every other family: 0 */
        int32_t reserved;         /* 0; LS3W: a flags word, bit 0 = digital I/O was recorded ("digital_io_enabled"), every other bit 0;
                                   * LS4: regs[C], the registers of slot C per round */
    } gsh_packed_format;
    /* packed bytes that hold n_samples samples per RF channel; GSH_ERR_INVALID for a bad descriptor or a count that is not whole items.  No GPU. */
    int gsh_packed_bytes(const gsh_packed_format* fmt, uint64_t n_samples, uint64_t* bytes);
    /* the host build of the decoder every device path shares: samples [first_sample, first_sample + n_samples) of fmt->channel in the packed
     * buffer `bytes` (host memory) -> out_iq, two floats (I, Q; Q = 0 for a real family) per sample.  No GPU (tests, host-side tools). */
    int gsh_packed_decode_host(const gsh_packed_format* fmt, const void* bytes, uint64_t first_sample, uint64_t n_samples, float* out_iq);
    /* samples [first_sample, first_sample + n_samples) of the packed buffer d_src (sample 0 = the first of its first byte) -> d_dst: complex64 for
     * the complex families (conjugated when inverted_spectrum), float32 of fmt->channel for the real ones (inverted_spectrum must be 0).
     * first_sample may fall inside a byte or a register, and n_samples need not end at one; d_src aligned to the item of a LABSAT / LS3W / LS4 / SPIR family;
     * d_dst 8-byte aligned (complex) or 4-byte aligned (real).  Asynchronous on hip_stream. */
    int gsh_unpack_device(int device, const gsh_packed_format* fmt, const void* d_src, uint64_t first_sample, uint64_t n_samples, int inverted_spectrum,
        void* d_dst, void* hip_stream);
    /* the same for several bands of a multi-band family (GSS6450, LS3W, LS4) in ONE pass over the packed block: samples [first_sample, first_sample + n_samples)
     * of band channels[i] -> complex64 at d_dst[i] (8-byte aligned), i < n_channels <= rf_channels.  fmt->channel is not consulted.  GSH_ERR_INVALID
     * for a family without several bands, a band out of range or named twice, a null or misaligned destination.  d_src is 4-byte aligned (GSS6450) or 8-byte aligned (LS3W, LS4).  The LS4 slots of one call hold equal register counts.
     * Asynchronous on hip_stream. */
    int gsh_unpack_device_multi(int device, const gsh_packed_format* fmt, const void* d_src, uint64_t first_sample, uint64_t n_samples,
        int inverted_spectrum, const int32_t* channels, int n_channels, void* const* d_dst, void* hip_stream);
    /* the push entry points above for packed complex samples: the packed bytes cross PCIe, the unpack writes complex64 straight into the ring.
     * Same rules as gsh_stream_push / _device / _pinned_async (gsh_stream_wait_copied and _upto cover the _pinned_async form).  A real family is
     * refused (GSH_ERR_INVALID): IF samples go through gsh_fir_create_packed. */
    int gsh_stream_push_packed(gsh_stream_t* s, const gsh_packed_format* fmt, const void* bytes, uint64_t n_samples, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_push_packed_device(gsh_stream_t* s, const gsh_packed_format* fmt, const void* device_bytes, uint64_t n_samples, int inverted_spectrum,
        void* hip_stream, uint64_t* first_index);
    int gsh_stream_push_packed_pinned_async(gsh_stream_t* s, const gsh_packed_format* fmt, const void* bytes, uint64_t n_samples, int inverted_spectrum,
        uint64_t* first_index);
    /* One push of a multi-band packed block (GSS6450, LS3W, LS4) into n_rings rings: band channels[i] goes to rings[i].  The block crosses PCIe once and
     * one pass over it writes every ring; afterwards each ring is, bit for bit and index for index, what the single-ring call of the same name
     * with fmt->channel = channels[i] would have left (resident range, mirror, push event, live words), and gsh_stream_wait / _wait_copied /
     * _wait_copied_upto work on every ring of the call.  Rings may differ in capacity, window and next index; they lie on one device.  n_samples
     * counts samples per band.  first_index: n_rings entries, or NULL.  All or nothing: on a refusal (GSH_ERR_INVALID for a ring or band named
     * twice, a band out of range, rings on different devices, a partial word, a single-band family; GSH_ERR_STATE for a live tracking channel
     * whose samples the push would overwrite) no ring advances.  The device form works on hip_stream (NULL: the first ring's own stream,
     * synchronous). */
    int gsh_stream_push_packed_multi(gsh_stream_t* const* rings, const int32_t* channels, int n_rings, const gsh_packed_format* fmt, const void* bytes,
        uint64_t n_samples, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_push_packed_multi_device(gsh_stream_t* const* rings, const int32_t* channels, int n_rings, const gsh_packed_format* fmt,
        const void* device_bytes, uint64_t n_samples, int inverted_spectrum, void* hip_stream, uint64_t* first_index);
    int gsh_stream_push_packed_multi_pinned_async(gsh_stream_t* const* rings, const int32_t* channels, int n_rings, const gsh_packed_format* fmt,
        const void* bytes, uint64_t n_samples, int inverted_spectrum, uint64_t* first_index);
    /* gsh_stream_group_push / _device for packed complex samples: rank 0 stages the packed bytes, the group replicates exactly those (padded as
     * gsh_stream_group_plan pads them), every rank unpacks into its own ring */
    int gsh_stream_group_push_packed(gsh_stream_group_t* g, const gsh_packed_format* fmt, const void* host_bytes, uint64_t n_samples, int inverted_spectrum,
        uint64_t* first_index);
    int gsh_stream_group_push_packed_device(gsh_stream_group_t* g, const gsh_packed_format* fmt, const void* device_bytes, uint64_t n_samples,
        int inverted_spectrum, uint64_t* first_index);
    /* ---- ION GNSS SDR metadata standard (ION_GSMS) recordings: the device half of ION_GSMS_Signal_Source (adapters/ion_gsms_signal_source.cc,
     * gnuradio_blocks/ion_gsms.cc, libs/ion_gsms_chunk_data.{h,cc}, libs/ion_gsms_chunk_unpacking_ctx.h, libs/ion_gsms_stream_encodings.h; "libs/" below).
     * The general layout of which the GSH_PACKED_* families are special cases; it does not fit gsh_packed_format, so it has a layout object of its own.
     * BIT STREAM.  A block of a recording is a run of chunk CYCLES; one cycle is the chunks in order, cycle_bytes = sum of size_word x count_words
     * (<= GSH_ION_MAX_CYCLE_BYTES).  Within one chunk the words in ascending order, each from its most significant bit down, form one bit stream (chunk
     * shift Left, libs/ion_gsms_chunk_unpacking_ctx.h:46-49,86-89).  A word is little-endian in memory unless big_endian: stream byte b of a little-endian
     * chunk of W-byte words is memory byte (b / W) W + W - 1 - b % W.  Head padding is skipped first (libs/ion_gsms_chunk_data.cc:149-153), pad = 8 x
     * size_word x count_words - sum of packed_bits >= 0; then the streams of the chunk in order, packed_bits each, selected or not (:156-167).
     * A stream's packed_bits are rate_factor samples (:58-59,179-180), each one FIELD when real and two when complex, in the order of `format`; a field
     * is w = packed_bits / rate_factor bits, halved when complex (:60-65,182-187); the divisions must be exact and 1 <= quantization <= w <= 16.  With
     * alignment 0 the code is the whole field (q = w); with alignment 1 / 2 it is the top / low q = quantization bits and the rest is ignored.  A
     * field may straddle words.  Sample k of a stream lies in cycle k / rate_factor.
     * VALUES.  The code c has q bits, most significant first; g is the Gray-decoded c (g = c ^ c>>1 ^ c>>2 ...):
     *   OB c - 2^(q-1)      OBA 2c - (2^q - 1)      TC c, or c - 2^q when its top bit is set      TCA 2 TC + 1
     *   SM sign = top bit, m = the rest: +-m      SMA +-(2m + 1)      MS sign = low bit, m = c >> 1: +-m      MSA +-(2m + 1)
     *   OG OB(g)      OGA OBA(g)      SIGN (q = 1): 0 -> +1, 1 -> -1
     * These equal the reference's tables at 2..5 bits (libs/ion_gsms_stream_encodings.h:105-163) for every encoding but MS at 3, 4 and 5 bits (below).
     * Outputs are float32 and exact: `negate` is applied to the integer value (a zero stays +0), then the conjugation of inverted_spectrum.
     * DEVIATIONS: the definition is the layout as the reference's code plainly intends it, not the reference as compiled --
     *   - its word type is signed: a field whose leading bit is set is extracted with an arithmetic shift and then indexes the look-up tables below
     *     their start (libs/ion_gsms_chunk_unpacking_ctx.h:164-168, libs/ion_gsms_chunk_data.cc:252-266); here fields are unsigned;
     *   - its masks are `1 << n` computed in int, also for 64-bit words (ctx.h:149,166); here no shift count reaches the operand's width;
     *   - a field that straddles words is not assembled there (ctx.h:143-161 ORs its two parts into the output at the wrong positions: 12-bit TC
     *     across 8-bit words AB CD EF gives (-1, -1)); here it is one bit string, (-1348, -529);
     *   - endianness is a TODO there (chunk_data.cc:141: the host's, little-endian); big_endian is honoured here;
     *   - the MS tables at 3, 4 and 5 bits repeat the 2-bit row (stream_encodings.h:125,140,155); here MS is regular, as the neighbouring MSA tables are;
     *   - SIGN passes the raw bit through there (chunk_data.cc:266-269); here it follows the sign convention of SM: 0 -> +1, 1 -> -1;
     *   - fields of 6 bits and more are passed through undecoded there (:266-269); here every encoding is defined at every width.
     * NOT BUILT: chunk shift Right (starts one word past the buffer there, ctx.h:50-57) and lump shift Right (writes items count .. 1 there,
     * chunk_data.cc:219-230): GSH_ERR_UNSUPPORTED; encoding FP: GSH_ERR_UNSUPPORTED; fields over 16 bits; streams of unequal rate in one call. */
#define GSH_ION_MAX_CHUNKS 16
#define GSH_ION_MAX_STREAMS 64     /* described per chunk cycle */
#define GSH_ION_MAX_SELECTED 8     /* per call, as the multi-ring frame */
#define GSH_ION_MAX_CYCLE_BYTES 4096
/* encodings, the reference's numbering (libs/ion_gsms_stream_encodings.h:37-48) */
#define GSH_ION_SIGN 0
#define GSH_ION_OB 1
#define GSH_ION_SM 2
#define GSH_ION_MS 3
#define GSH_ION_TC 4
#define GSH_ION_OG 5
#define GSH_ION_OBA 6
#define GSH_ION_SMA 7
#define GSH_ION_MSA 8
#define GSH_ION_TCA 9
#define GSH_ION_OGA 10
#define GSH_ION_FP 11 /* GSH_ERR_UNSUPPORTED */
    typedef struct
    {
        int32_t size_word;   /* 1, 2, 4, 8 bytes */
        int32_t count_words; /* >= 1 */
        int32_t big_endian;  /* 0: little-endian words */
        int32_t shift;       /* 0 Left; 1 Right -> GSH_ERR_UNSUPPORTED */
        int32_t padding;     /* 0 none / tail, 1 head */
        int32_t n_streams;   /* streams of this chunk, lumps flattened in file order */
    } gsh_ion_chunk;
    typedef struct
    {
        int32_t packed_bits, rate_factor, quantization, encoding;
        int32_t format;     /* GSH_PACKED_REAL / _IQ / _QI */
        int32_t alignment;  /* 0 undefined: the code is the whole field; 1 left: its top `quantization` bits; 2 right: its low bits */
        int32_t lump_shift; /* 0 Left / undefined; 1 Right -> GSH_ERR_UNSUPPORTED */
        int32_t negate;     /* bit 0: negate I (or the real value), bit 1: negate Q */
    } gsh_ion_stream;
    typedef struct gsh_ion_layout gsh_ion_layout_t;
    /* `streams` lists the streams of every chunk in order: chunks[0].n_streams of them, then chunks[1].n_streams ...; n_streams is their total.
     * GSH_ERR_INVALID for a descriptor that breaks a rule or a limit above, GSH_ERR_UNSUPPORTED for a Right shift or FP.  No GPU. */
    int gsh_ion_layout_create(const gsh_ion_chunk* chunks, int n_chunks, const gsh_ion_stream* streams, int n_streams, gsh_ion_layout_t** out);
    void gsh_ion_layout_destroy(gsh_ion_layout_t* layout);
    int gsh_ion_layout_info(const gsh_ion_layout_t* layout, uint32_t* cycle_bytes, int32_t* n_streams);
    /* samples of `stream` per cycle (rate_factor), whether it is complex, and the bits of one field (w) */
    int gsh_ion_stream_info(const gsh_ion_layout_t* layout, int stream, int32_t* samples_per_cycle, int32_t* is_complex, int32_t* field_bits);
    /* the bytes of the cycles that samples [0, n_samples) of `stream` touch */
    int gsh_ion_bytes(const gsh_ion_layout_t* layout, int stream, uint64_t n_samples, uint64_t* bytes);
    /* the host build of the decoder the kernel shares (csrc/ion_gsms.h): samples [first_sample, first_sample + n_samples) of `stream` in the block
     * `bytes` (host memory, cycle 0 at its first byte) -> out: one float per sample for a real stream, two (I, Q) for a complex one.  No GPU. */
    int gsh_ion_decode_host(const gsh_ion_layout_t* layout, int stream, const void* bytes, uint64_t first_sample, uint64_t n_samples, float* out);
    /* one pass over the device-resident block d_src (the start of a cycle, aligned to the largest size_word of the layout) writes samples
     * [first_sample, first_sample + n_samples) of streams[i] to d_dst[i], i < n_streams <= GSH_ION_MAX_SELECTED: complex64 (8-byte aligned, conjugated
     * when inverted_spectrum) when the streams are complex, float32 (4-byte aligned; inverted_spectrum must be 0) when they are real.  The streams of
     * one call have equal samples per cycle and are all complex or all real (GSH_ERR_INVALID otherwise, as the equal slots of LS4); none is named
     * twice.  first_sample may fall inside a cycle and n_samples need not end at one.  Real streams are IF samples: they reach a ring through
     * gsh_fir_process_device with the floats of this call.  Asynchronous on hip_stream. */
    int gsh_ion_unpack_device(int device, const gsh_ion_layout_t* layout, const void* d_src, uint64_t first_sample, uint64_t n_samples,
        int inverted_spectrum, const int32_t* streams, int n_streams, void* const* d_dst, void* hip_stream);
    /* One push of a block of whole cycles into n_rings rings: complex stream streams[i] goes to rings[i].  The block crosses PCIe once and one pass
     * over it writes every ring; afterwards each ring is, bit for bit and index for index, what gsh_stream_push of the host-decoded samples
     * (gsh_ion_decode_host, gr_complex, the same inverted_spectrum) would have left, and gsh_stream_wait / _wait_copied / _wait_copied_upto work on
     * every ring of the call.  n_samples counts samples per stream and must be whole cycles.  first_index: n_rings entries, or NULL.  All or nothing,
     * as gsh_stream_push_packed_multi: GSH_ERR_INVALID for a real stream, streams of unequal rate, a stream or ring named twice, a partial cycle,
     * rings on different devices, a push above a capacity; GSH_ERR_STATE for a live tracking channel whose samples the push would overwrite; then
     * no ring advances.  The device form takes a block aligned to the largest size_word and works on hip_stream (NULL: the first ring's own
     * stream, synchronous). */
    int gsh_stream_push_ion(gsh_stream_t* const* rings, const int32_t* streams, int n_rings, const gsh_ion_layout_t* layout, const void* bytes,
        uint64_t n_samples, int inverted_spectrum, uint64_t* first_index);
    int gsh_stream_push_ion_device(gsh_stream_t* const* rings, const int32_t* streams, int n_rings, const gsh_ion_layout_t* layout,
        const void* device_bytes, uint64_t n_samples, int inverted_spectrum, void* hip_stream, uint64_t* first_index);
    int gsh_stream_push_ion_pinned_async(gsh_stream_t* const* rings, const int32_t* streams, int n_rings, const gsh_ion_layout_t* layout,
        const void* bytes, uint64_t n_samples, int inverted_spectrum, uint64_t* first_index);
    /* ---- antenna array front end: the spatial filter of Array_Signal_Conditioner (Beamformer_Filter, gnss_block_factory.cc:819-839;
     * src/algorithms/input_filter/gnuradio_blocks/beamformer.{h,cc}) for up to 8 antennas, several beams at once, each beam straight into its own
     * ring, and the array covariance the weights are computed from.
     * Arithmetic (the definition): every item becomes a complex float by the integer -> float cast of the ring pushes, (I, Q) per first_is_q,
     * conjugated when inverted_spectrum.  Then for beam b (beamformer.cc:53-61): sum = (0, 0); for a = 0 .. A-1 in that order
     *   p.re = x.re w.re - x.im w.im,  p.im = x.re w.im + x.im w.re,  sum += p
     * in float32 with one rounding per operation, w = weight [b][a].  The reference block has 8 inputs, one output and weights fixed at (1, 0)
     * (beamformer.h:52; its "dynamically reloadable weights" have no setter); here the antennas, the beams and the weights are the caller's.
     * A call uses the weights as they stand when it is made (they travel as kernel arguments): gsh_beam_set_weights between two pushes takes
     * effect exactly at the push boundary.
     * `items` / `device_items` hold n_antennas pointers for GSH_ARRAY_PLANAR and one pointer for GSH_ARRAY_INTERLEAVED; device pointers are
     * aligned to the item (2 / 4 / 8 bytes), 16-byte aligned interleaved frames of whole 16-byte words are read with 16-byte loads. */
#define GSH_ARRAY_MAX_ANTENNAS 8 /* GNSS_SDR_BEAMFORMER_CHANNELS, beamformer.h:37 */
#define GSH_ARRAY_MAX_BEAMS 8
#define GSH_ARRAY_PLANAR 0      /* one buffer per antenna: the block's input_items[a] (beamformer.cc:59; Multichannel_File_Signal_Source) */
#define GSH_ARRAY_INTERLEAVED 1 /* one buffer of sample-major frames, antenna a of sample k is item k*A + a: the wire layout of
                                   Custom_UDP_Signal_Source for cbyte / ishort / cfloat (gr_complex_ip_packet_source.cc:395-488) */
    typedef struct
    {
        int32_t n_antennas; /* 1..8 */
        int32_t item_type;  /* enum gsh_item_type */
        int32_t layout;     /* GSH_ARRAY_PLANAR / _INTERLEAVED */
        int32_t first_is_q; /* 0: the first value of a pair is I; 1: it is Q (Custom_UDP's IQ_swap = false, gr_complex_ip_packet_source.cc:406-413) */
    } gsh_array_format;
    typedef struct gsh_beam gsh_beam_t;
    /* GSH_ERR_INVALID (before any device is touched) for a null pointer, n_antennas or n_beams outside 1..8, an unknown item type or layout */
    int gsh_beam_create(int device, const gsh_array_format* fmt, int n_beams /* 1..8 */, gsh_beam_t** out);
    void gsh_beam_destroy(gsh_beam_t* b);
    /* n_beams x n_antennas complex64, row-major; default every weight (1, 0), beamformer.h:52 */
    int gsh_beam_set_weights(gsh_beam_t* b, const float* w_iq);
    int gsh_beam_get_weights(const gsh_beam_t* b, float* w_iq);
    /* n samples of every antenna -> beam r at device_out[r] (n complex64, 8-byte aligned), r < n_beams; asynchronous on hip_stream (NULL: the
     * handle's own stream, synchronous) */
    int gsh_beam_process_device(gsh_beam_t* b, const void* const* device_items, uint64_t n, int inverted_spectrum, void* const* device_out, void* hip_stream);
    /* One push of an array block into n_beams rings: beam r goes to rings[r].  The raw block crosses PCIe once and one pass over it writes every
     * ring; afterwards ring r holds, bit for bit and index for index, what gsh_stream_push(rings[r], beam_r, n, GSH_ITEM_GR_COMPLEX, 0, ...) of the
     * host-computed beam would have left (resident range, mirror, push event and history, live words), and gsh_stream_wait / gsh_stream_read work
     * on every ring of the call.  Rings may differ in capacity, window and next index; they lie on the handle's device.  first_index: n_beams
     * entries, or NULL.  All or nothing, as gsh_stream_push_packed_multi: GSH_ERR_INVALID for a null pointer, a ring named twice, a ring on
     * another device, n above a ring's capacity; GSH_ERR_STATE for a live tracking channel whose samples the push would overwrite on any ring;
     * after a refusal no ring has advanced.  The device form works on hip_stream (NULL: the first ring's own stream, synchronous). */
    int gsh_beam_push(gsh_beam_t* b, gsh_stream_t* const* rings, const void* const* items, uint64_t n, int inverted_spectrum, uint64_t* first_index);
    int gsh_beam_push_device(gsh_beam_t* b, gsh_stream_t* const* rings, const void* const* device_items, uint64_t n, int inverted_spectrum, void* hip_stream,
        uint64_t* first_index);
    /* r_iq: n_antennas x n_antennas complex128, row-major, R[i][j] = sum_n x_i[n] conj(x_j[n]) -- a sum, the caller divides -- of x as the
     * beamformer sees it (after first_is_q and inverted_spectrum).  Products (exact: two float32 factors) and sums in FP64; the upper triangle
     * is computed, the lower is its conjugate.  Per-work-group partials added in a fixed order, no floating-point atomics: the same data give
     * the same bits on every run.  Synchronous. */
    int gsh_beam_covariance(gsh_beam_t* b, const void* const* items, uint64_t n, int inverted_spectrum, double* r_iq);
    int gsh_beam_covariance_device(gsh_beam_t* b, const void* const* device_items, uint64_t n, int inverted_spectrum, double* r_iq);
    /* average time of one beam pass over a zero-filled block of n samples in the handle's format, HIP events, as the other gsh_*_time_* calls */
    int gsh_beam_time_process(gsh_beam_t* b, uint64_t n, int reps, float* avg_ms);
    /* Adaptive mode: the weights of every beam come from the covariance of the blocks themselves, on the device.  On an adaptive handle
     * gsh_beam_process_device, gsh_beam_push and gsh_beam_push_device queue, on the stream the call works on,
     *   covariance partials -> final sums (R_block: gsh_beam_covariance_device of the block, bit for bit) -> accumulate and solve -> beam pass
     * with no read-back and no host synchronisation beyond what the fixed-weight call of the same name does.  The raw block is read twice on the
     * device and crosses PCIe once.  Arithmetic (the definition; csrc/array_weights.h, FP64, one rounding per operation, no square root, every
     * sum in ascending index order):
     *   R_acc <- forgetting * R_acc + R_block                 per real number of the upper triangle; the diagonal's imaginary parts are 0
     *   delta  = loading_rel * (sum_i Re R_acc[i][i]) / A + loading_abs,   M = R_acc + delta I
     *   M = L D L^H                                           square-root-free Cholesky, column by column, no pivoting
     *   per beam, c its constraint vector:  L y = c,  z = y / D,  L^H u = z,  d = sum_i conj(c_i) u_i,  v = u conj(d) / |d|^2
     *   w = conj(v), each part rounded once to float32        (the block's convention y = sum_a x_a w_a)
     * c = the steering vector s gives the MVDR weights R^-1 s / (s^H R^-1 s); c = the unit vector of a reference element gives power inversion
     * (that element's weight is exactly (1, 0)).  The weights a block is formed with come from the covariance through that block.
     * A call FAILS when a pivot D[j] is not > 0, |d|^2 is not > 0 or a number on the way is not finite: R_acc is updated all the same, `failures`
     * counts it and every beam keeps the weights it had before the call -- the caller's fixed weights until the first call that succeeds.
     * gsh_adaptive_beam_set takes effect at the next call, at its first sample; setting the mode starts from R_acc = 0 and both counters 0;
     * NULL clears it: the caller's fixed weights (kept meanwhile; gsh_beam_get_weights returns them throughout) are in force again.
     * GSH_ERR_INVALID, before any device is touched, for a null handle, forgetting outside [0, 1], a negative loading, a number that is not
     * finite, an all-zero constraint vector of a beam the handle forms.  Refusals of the pushes are as on a fixed-weight handle and leave R_acc,
     * weights and counters as they were.  Consecutive adaptive calls on different streams are ordered by the handle (an event recorded at the
     * end of a chain, waited for at the start of the next).  gsh_beam_covariance* is unchanged on an adaptive handle and does not touch R_acc
     * (the chain has scratch memory of its own); gsh_beam_time_process times the whole chain on copies of the state. */
    typedef struct gsh_beam_adapt
    {
        double forgetting;  /* lambda in [0, 1]: R_acc <- lambda R_acc + R_block (0: every block on its own) */
        double loading_rel; /* >= 0 */
        double loading_abs; /* >= 0; delta = loading_rel * (sum_i Re R_acc[i][i]) / A + loading_abs, added to the diagonal */
        double constraint_iq[GSH_ARRAY_MAX_BEAMS][GSH_ARRAY_MAX_ANTENNAS][2]; /* per beam the constraint vector c (entries a < n_antennas) */
    } gsh_beam_adapt;
    struct gsh_beam_adapt_state
    {
        uint64_t blocks;   /* adaptive calls completed since the mode was set (failed ones included) */
        uint64_t failures; /* those of them that failed */
        double delta;      /* the loading of the last call */
        double r_acc_iq[GSH_ARRAY_MAX_ANTENNAS * GSH_ARRAY_MAX_ANTENNAS * 2]; /* the first A x A complex128, row-major, as gsh_beam_covariance */
        float w_iq[GSH_ARRAY_MAX_BEAMS * GSH_ARRAY_MAX_ANTENNAS * 2];         /* the weights in force: the first n_beams x A complex64, row-major */
    };
    /* (the gsh_beam_* prefix is the fixed-weight entry points' list; the two calls of the adaptive mode carry a prefix of their own) */
    int gsh_adaptive_beam_set(gsh_beam_t* b, const gsh_beam_adapt* conf); /* NULL: back to the caller's fixed weights */
    /* synchronous: waits for the adaptive calls queued so far.  GSH_ERR_STATE on a handle that is not adaptive. */
    int gsh_adaptive_beam_state(gsh_beam_t* b, struct gsh_beam_adapt_state* out);
    /* Direct (nearest-neighbour) resampler, the arithmetic of direct_resampler_conditioner_cc (src/algorithms/resampler/gnuradio_blocks/
     * direct_resampler_conditioner_cc.cc:39-129; used by the signal conditioner and the acquisition decimator, gnss_flowgraph.cc:1165-1209):
     * 32-bit phase accumulator, a sample is copied on every wrap.  Stateless form: outputs are numbered from the start of the stream,
     * output j reads input ceil(j 2^32 / phase_step) (decimation) or floor((j + 1) phase_step / 2^32) (interpolation) -- what the reference's
     * loop produces, however the stream is cut into blocks.  device_src[0] is absolute input sample in0 (n_in samples, complex64), device_dst[0]
     * receives absolute output out0; *n_out = how many outputs this block feeds (<= max_out), *n_in_consumed (may be NULL) = input samples the
     * reference block would have consumed by then.  Asynchronous on hip_stream. */
    int gsh_direct_resample_device(int device, const void* device_src, uint64_t in0, uint64_t n_in, double fs_in, double fs_out, uint64_t out0,
        void* device_dst, uint64_t max_out, uint64_t* n_out, uint64_t* n_in_consumed, void* hip_stream);
    /* Frequency-translating decimating FIR filter: what the input-filter adapters instantiate (src/algorithms/input_filter/adapters/
     * freq_xlating_fir_filter.cc:115-161: gr::filter::freq_xlating_fir_filter_{ccf,fcf,scf}::make(decimation, taps, IF, sampling_frequency);
     * fir_filter.cc: fir_filter_ccf = the same with IF 0, decimation 1).  y[m] = sum_k taps[k] x[mD - k] exp(-j 2 pi IF (mD - k) / fs), zero
     * history before the stream starts.  The taps are the adapter's (pm_remez / firdes, computed once on the host).  input_kind: 0 complex64
     * (ccf), 1 real float32 (fcf), 2 real int16, 3 real int8 (scf after byte_to_short).  The handle carries the filter history, so a stream may
     * be fed in blocks of any size: *n_out outputs are written per call (every output whose newest input has arrived). */
    typedef struct gsh_fir gsh_fir_t;
    int gsh_fir_create(int device, const float* taps, int n_taps, int decimation, double center_freq_hz, double sampling_freq_hz, int input_kind,
        gsh_fir_t** out);
    void gsh_fir_destroy(gsh_fir_t* f);
    int gsh_fir_process_device(gsh_fir_t* f, const void* device_in, uint64_t n_in, void* device_out, uint64_t max_out, uint64_t* n_out, void* hip_stream);
    /* the same filter fed packed front-end bytes (gsh_packed_format): gsh_fir_process_device's device_in is the packed block and n_in counts
     * samples of fmt->channel, a whole number of input items per call.  Output and history are those of gsh_fir_create fed the unpacked samples
     * (real families: input_kind 1 with the floats of gsh_unpack_device; complex families: input_kind 0, not conjugated). */
    int gsh_fir_create_packed(int device, const float* taps, int n_taps, int decimation, double center_freq_hz, double sampling_freq_hz,
        const gsh_packed_format* fmt, gsh_fir_t** out);
    /* ---- signal conditioner: the chain every receiver puts between its source and its channels (Signal_Conditioner,
     * src/algorithms/conditioner/adapters/signal_conditioner.cc:60-87: DataTypeAdapter -> InputFilter -> Resampler), one handle and one call per
     * block, one pass over the raw block straight into a ring.  Ring sample j of the conditioner's output (j counts from the handle's creation) is
     *   ring[base + j] = sum_{k<K} taps[k] rot(x[m(j) D - k]),
     * x the block's samples decoded as the adapters decode them (ibyte_to_complex.cc:45-51, ishort_to_complex.cc:45-51, the packed sources
     * above; conjugated first when inverted_spectrum), rot and the sum those of gsh_fir_process_device (freq_xlating_fir_filter.cc:115-161,
     * fir_filter.cc), m(j) the input index of gsh_direct_resample_device (direct_resampler_conditioner_cc.cc:39-129), `base` the ring's next index
     * when it was bound.  Invariant: after any sequence of pushes the ring holds, index for index and bit for bit, what gsh_convert_samples_device
     * / gsh_unpack_device -> gsh_fir_process_device -> gsh_direct_resample_device give for the concatenated input in one call per stage; where the
     * stream is cut into pushes does not matter.  Only the filter outputs the resampler keeps are formed.  The handle owns its device staging
     * and the converted history (n_taps - 1 samples) between pushes; all counts are integers computed on the host, a push reads nothing back.
     * Pulse_Blanking_Filter is an optional stage between the filter and the resampler (gsh_cond_set_blanking below).
     * So are the notch filters, in this chain's own cut-invariant form with all state on the device (gsh_cond_set_notch below).
     * Not stages of this chain (they stay loose calls): Notch_Filter, Notch_Filter_Lite (gsh_notch_*: a one-sample advance and a state the host
     * shadows); a fan-out of several filters into several rings; stream groups; the cshort / cbyte outputs of the xlating adapter
     * (freq_xlating_fir_filter.cc:136-160). */
#define GSH_COND_INPUT_ITEMS 0  /* complex items of an enum gsh_item_type (item_type) */
#define GSH_COND_INPUT_REAL 1   /* real items: item_type 1 float32, 2 int16, 3 int8 (the input_kind of gsh_fir_create); needs a filter */
#define GSH_COND_INPUT_PACKED 2 /* packed front-end bytes (packed); a real family needs a filter */
    typedef struct
    {
        int32_t input;             /* GSH_COND_INPUT_* */
        int32_t item_type;         /* see GSH_COND_INPUT_ITEMS / _REAL; unused for packed input */
        int32_t inverted_spectrum; /* conjugate the decoded sample before the filter (complex input only) */
        int32_t n_taps;            /* 0: InputFilter Pass_Through; else 1..1024 as gsh_fir_create */
        const float* taps;         /* n_taps real taps (copied by gsh_cond_create) */
        int32_t decimation;        /* 1..64; 0 reads as 1 */
        int32_t reserved;          /* 0 */
        double center_freq_hz;     /* IF */
        double sampling_freq_hz;   /* of the filter's input; positive when n_taps > 0 */
        double fs_in, fs_out;      /* Direct_Resampler: sample_freq_in (the rate after the filter) / sample_freq_out; both 0: Pass_Through */
        gsh_packed_format packed;  /* GSH_COND_INPUT_PACKED */
    } gsh_cond_conf;
    typedef struct gsh_cond gsh_cond_t;
    /* GSH_ERR_INVALID with a message, before any device is touched, for: a null pointer, an unknown input or item type, real input without a
     * filter (the ring holds complex samples), inverted_spectrum on real input, taps / decimation / sampling frequency outside gsh_fir_create's
     * limits, one of fs_in / fs_out zero or negative, a ratio the 32-bit phase accumulator cannot hold (as gsh_direct_resample_device), a bad
     * packed format */
    int gsh_cond_create(int device, const gsh_cond_conf* conf, gsh_cond_t** out);
    void gsh_cond_destroy(gsh_cond_t* h);
    /* the same checks and the bookkeeping alone, no GPU: *n_out_total = ring samples the conditioner has produced once n_in_total input samples
     * have arrived (every filter output whose newest input is there, every resampler output whose filter output is) */
    int gsh_cond_plan(const gsh_cond_conf* conf, uint64_t n_in_total, uint64_t* n_out_total);
    /* the ring the pushes write (on the handle's device; it outlives the handle's use): the conditioner's NEXT output goes to the ring's next
     * index as it stands now.  NULL detaches. */
    int gsh_cond_bind(gsh_cond_t* h, gsh_stream_t* ring);
    /* One block of n_in input samples (packed input: a whole number of input items) through the chain into the bound ring.  *first_out = ring
     * index of the block's first output, *n_out = how many it completed (0 is not an error: a block shorter than the decimation); either may be
     * NULL.  gsh_cond_push: host memory, synchronous.  _push_device: the block lies in device memory (aligned to its item), the work is queued on
     * hip_stream (NULL: the ring's own stream, synchronous).  _push_pinned_async: page-locked host memory (gsh_host_register), returns at once;
     * the block must stay untouched until gsh_stream_wait_copied / gsh_stream_wait_copied_upto(ring, *first_out + *n_out) covers the push (a
     * push with *n_out = 0: until the next one is covered).
     * All or nothing; a refusal advances nothing and rotates no history: GSH_ERR_INVALID for more outputs than the ring's capacity, a partial
     * packed item, no bound ring; GSH_ERR_STATE when the ring's next index is no longer where the conditioner left it (someone else pushed or
     * sought) or a live tracking channel would be overrun. */
    int gsh_cond_push(gsh_cond_t* h, const void* items, uint64_t n_in, uint64_t* first_out, uint64_t* n_out);
    int gsh_cond_push_device(gsh_cond_t* h, const void* device_items, uint64_t n_in, void* hip_stream, uint64_t* first_out, uint64_t* n_out);
    int gsh_cond_push_pinned_async(gsh_cond_t* h, const void* items, uint64_t n_in, uint64_t* first_out, uint64_t* n_out);
    /* input samples taken and ring samples produced since the handle was created */
    int gsh_cond_position(const gsh_cond_t* h, uint64_t* n_in_total, uint64_t* n_out_total);
    /* average HIP-event time of the device work of one push of device_block (n_in samples, device memory) from the handle's present state: the
     * fused launch into a scratch destination and the history update.  Neither the ring nor the handle's position or history changes. */
    int gsh_cond_time_push(gsh_cond_t* h, const void* device_block, uint64_t n_in, int reps, float* avg_ms);
    /* ---- pulse blanking as a stage of the conditioner's push (Pulse_Blanking_Filter: pulse_blanking_filter.cc:73-125, an optional xlating
     * filter with decimation 1 in front of pulse_blanking_cc; here behind whatever filter the conf names).  With y the filter-output stream of the
     * chain above (the decoded samples themselves when n_taps = 0): y is tiled into segments of `length` samples from y[0] on; the energy and the
     * decision of a segment are those of gsh_pb_process_device over the whole stream (pulse_blanking_cc.cc:63-95), the state lives in device
     * memory and is carried from push to push; z[k] = (0, 0) where the segment of k was blanked, else y[k]; the resampler gathers from z with the
     * same m(j).  Only whole segments are emitted and a trailing partial one waits for the next push (it is never flushed): after N inputs and
     * M = ceil(N / D) filter outputs, M' = floor(M / length) * length are mitigated and the ring has every j with m(j) < M'.
     * Invariant: the ring holds, bit for bit, what the loose chain gives with gsh_pb_process_device between the filter and the resampler, one call
     * per stage over the concatenated input, and gsh_cond_blanking_state equals gsh_pb_get_state of that run.  One difference in timing, not in
     * content: gsh_pb_process_device, like the block, leaves a segment that ends exactly on the last offered item for its next call; the
     * conditioner emits it. */
    typedef struct
    {
        float pfa;                /* in (0, 1) */
        int32_t length;           /* 1..4096 samples per segment */
        int32_t n_segments_est;   /* >= 0 */
        int32_t n_segments_reset; /* >= 0 */
    } gsh_cond_blanking;
    struct gsh_cond_blanking_state /* a struct tag: the entry point that fills it has the same name */
    {
        float thres;                  /* gsh_pb_threshold */
        float noise_power_estimation; /* as gsh_pb_get_state */
        int32_t n_segments;
        int32_t last_filtered;
        uint64_t n_decided;           /* segments decided since the handle was created */
        uint64_t n_blanked;           /* ... and those of them that were blanked */
    };
    /* Allowed until the handle's first push (GSH_ERR_STATE afterwards); GSH_ERR_INVALID with a message for values outside gsh_pb_create's ranges,
     * before anything is allocated.  NULL turns the stage off again.  The push entry points, _position, _bind and _time_push keep their rules; a
     * push that completes no segment returns *n_out = 0. */
    int gsh_cond_set_blanking(gsh_cond_t* h, const gsh_cond_blanking* blanking);
    /* gsh_cond_plan for a chain with the stage (NULL: without it) */
    int gsh_cond_plan_blanked(const gsh_cond_conf* conf, const gsh_cond_blanking* blanking, uint64_t n_in_total, uint64_t* n_out_total);
    /* waits for the handle's queued pushes, then reads the state.  GSH_ERR_STATE on a handle without the stage. */
    int gsh_cond_blanking_state(gsh_cond_t* h, struct gsh_cond_blanking_state* state);
    /* ---- the notch filters as a stage of the conditioner's push (Notch_Filter: notch_cc.cc:72-118; Notch_Filter_Lite: notch_lite_cc.cc:81-136),
     * between the filter and the resampler like the blanking stage.
     * Streams.  With y[0], y[1], ... the filter-output stream of the chain above (the decoded samples themselves when n_taps = 0), the stage forms
     * the notch output stream w[k], k = 0, 1, ...: w[k] is the mitigated y[k + 1] with y[k] as its previous sample -- the blocks' one-sample
     * advance (notch_cc.cc:72 `in++`, NotchLite's history item); y[0] is only ever a "sample in front".
     * Segments.  w is tiled into segments of `length` samples from w[0] on; segment s needs y[1 + s L .. (s + 1) L].  After M >= 1 filter outputs
     * S = floor((M - 1) / L) segments are decided and W' = S L notch outputs exist (the block's loop condition (index_out + length_) <
     * noutput_items over the whole stream); the resampler gathers from w with the same m(j), and the ring has every j with m(j) < W'.  A trailing
     * partial segment waits for the next push; it is never flushed.
     * Per segment the state machine, the energy, the spectral noise floor, NotchLite's z0 and the per-sample map out = a + b out_prev are those of
     * gsh_notch_process_device (one text, csrc/notch_filter.h); the energy sum's rotation is keyed to the segment's absolute index, so its bits are
     * those of one call over the whole stream.
     * The recurrence is evaluated as gsh_notch_process_device evaluates it within a call: chunks of 128 notch outputs, aligned to the absolute index
     * (chunk c = w[128 c .. 128 c + 127]), one composite (B, A) per chunk, a sequential carry chain over the chunks, each chunk replayed from its
     * carry.  The carry handed from push to push is the composite carry at the start of the open chunk, never a replayed output; a chunk that the
     * push's last decided segment cuts is replayed from its carry up to that segment now, and the next push forms it again from its start and writes
     * only the new outputs.  Between pushes the handle therefore keeps, in device memory: the filter outputs from y[128 c0] on, c0 = floor(W' / 128)
     * (at most 128 + length + 1 samples), the modes (NotchLite: and coefficients) of the decided segments that overlap the open chunk (at most 65),
     * the carry of chunk c0, and the state-machine state.
     * Invariant: the ring after any sequence of pushes equals, index for index and bit for bit, what the loose chain gives for the concatenated
     * input with one call per stage: gsh_convert_samples_device / gsh_unpack_device -> gsh_fir_process_device -> one gsh_notch_process_device over
     * all M filter outputs -> gsh_direct_resample_device.  Where the pushes cut the stream does not matter.  gsh_cond_notch_state equals
     * gsh_notch_get_state after that one call in noise_pow_est, n_segments, filter_state, n_segments_coeff and, for NotchLite, z0.  (The loose call's
     * last_out and Notch's per-sample z0 depend on where its last chunk falls: they are not reported.  Several loose calls over the same stream do
     * not give these bits: each starts its chunks anew and hands on a replayed output.)
     * A push reads nothing back: no shadow state, no retry.  Whether the noise-floor values (a length-point DFT per segment) are formed is decided
     * on the device from the state at the start of the push, by the condition gsh_notch_process_device evaluates on its shadow; the decision never
     * lacks a value it needs, and the bits do not depend on it.
     * One mitigation stage per handle: gsh_cond_set_notch while blanking is on, and gsh_cond_set_blanking (not NULL) while the notch stage is on,
     * return GSH_ERR_STATE. */
    typedef struct
    {
        float pfa;                /* in (0, 1) */
        float p_c_factor;         /* finite */
        int32_t length;           /* 2..1024 samples per segment */
        int32_t n_segments_est;   /* >= 0 */
        int32_t n_segments_reset; /* >= 0 */
        int32_t n_segments_coeff; /* 0: Notch; >= 1: NotchLite, one coefficient per that many filtered segments */
    } gsh_cond_notch;
    struct gsh_cond_notch_state /* a struct tag: the entry point that fills it has the same name */
    {
        float thres;              /* gsh_notch_threshold */
        float noise_pow_est;      /* as gsh_notch_get_state */
        int32_t n_segments;
        int32_t filter_state;
        int32_t n_segments_coeff;
        int32_t reserved;         /* 0 */
        float z0[2];              /* NotchLite's coefficient; (0, 0) for Notch */
        uint64_t n_decided;       /* segments decided since the handle was created */
        uint64_t n_filtered;      /* ... and those of them that went through the recurrence */
    };
    /* Allowed until the handle's first push (GSH_ERR_STATE afterwards, and while the blanking stage is on); GSH_ERR_INVALID with a message for
     * values outside gsh_notch_create's ranges, before any device is touched.  NULL turns the stage off again.  The push entry points, _position,
     * _bind and _time_push keep their rules (at most 2^32 filter outputs per push, as with blanking; _time_push changes neither the ring nor any
     * carried state); a push that completes no segment returns *n_out = 0. */
    int gsh_cond_set_notch(gsh_cond_t* h, const gsh_cond_notch* notch);
    /* gsh_cond_plan for a chain with the stage (NULL: without it); no GPU */
    int gsh_cond_plan_notched(const gsh_cond_conf* conf, const gsh_cond_notch* notch, uint64_t n_in_total, uint64_t* n_out_total);
    /* waits for the handle's queued pushes, then reads the state.  GSH_ERR_STATE on a handle without the stage. */
    int gsh_cond_notch_state(gsh_cond_t* h, struct gsh_cond_notch_state* state);
    /* ---- signal generator: synthetic GNSS scenarios made on the device (Signal_Generator: src/algorithms/signal_generator/adapters/
     * signal_generator.cc over gnuradio_blocks/signal_generator_c.h / .cc = sg.cc), into a caller's device buffer or straight into a ring.
     * Table-driven.  A generator holds n_sats <= GSH_GEN_MAX_SATS satellites; a satellite is two complex64 tables A and B of `period` samples
     * (B may be NULL), a delay_samples in [0, period), two periodic sign sequences sA, sB of 1..GSH_GEN_MAX_SIGNS bytes +-1, and a carrier.
     * Sample n -- the ABSOLUTE index since the generator's start -- is, in float32, satellites in ascending order, every operation rounded once:
     *   out[n] = sum_sat (sA[p mod len_a] A[n mod period] + sB[p mod len_b] B[n mod period]) exp(+j (start_phase + 2 pi f n / fs)) + noise[n]
     *   p = (n + period - delay_samples) / period   (the sign boundaries passed: one lies at every n = delay_samples mod period, where the
     *       reference may change its data bit inside a code period, sg.cc:362-383, :426-450)      f = doppler_hz + carrier_offset_hz
     * which covers the reference's three combinations: GPS / GLONASS (sg.cc:366, :399: A = scaled sampled code, sA = data bits, no B; GLONASS'
     * FDMA offset, sg.cc:388, is carrier_offset_hz), Galileo E1 / E6 (sg.cc:518, :492: A = data component, B = minus the pilot with its secondary
     * code, sB = +1) and Galileo E5a / E5b (sg.cc:428-448: A = (Re, 0), B = (0, Im), sA = data bit x I secondary code, sB = Q secondary code,
     * an entry per code period).  The tables are the host's: generate_codes() (sg.cc:164-323) with its chip shift and its C/N0 scaling
     * sqrt(10^(CN0/10) / BW_BB) (sg.cc:184), halved power for two-component signals (sg.cc:230); the kernel knows amplitudes only.
     * Carrier: the phase of sample n is evaluated from n (128-bit fixed-point revolutions per sample, exact for every 64-bit index) -- the
     * reference accumulates a float32 phase per sample and a float32 start phase per vector (sg.cc:350-354); a stated deviation.
     * Noise (off: nothing is added): complex white Gaussian of unit variance per component (sg.cc:540-546), Philox4x32-10 keyed by the seed with
     * the absolute sample index as its counter, then Box-Muller.  Table entry, sign, phase and noise of sample n depend on n alone: the stream is
     * the same bit for bit however it is cut into calls and wherever a ring wraps.  The data bits the reference draws from a random_device are
     * the caller's sign sequence. */
#define GSH_GEN_MAX_SATS 32
#define GSH_GEN_MAX_SIGNS 1024
    typedef struct gsh_gen gsh_gen_t;
    /* GSH_ERR_INVALID before any device is touched: null out, fs_sps not positive and finite, n_sats outside 1..GSH_GEN_MAX_SATS */
    int gsh_gen_create(int device, double fs_sps, int32_t n_sats, gsh_gen_t** out);
    void gsh_gen_destroy(gsh_gen_t* g);
    /* tables as interleaved (I, Q) float32, copied.  GSH_ERR_INVALID before anything is touched: null handle, table A or sign sequence, `sat`
     * outside the handle's satellites, period below 1 (or above 2^30), delay_samples outside [0, period), a sign byte other than +-1, a sequence
     * length outside 1..GSH_GEN_MAX_SIGNS, a Doppler, start phase, carrier offset or table value that is not finite.  With table_b NULL signs_b /
     * len_b are not read.  gsh_gen_check_satellite: the same checks alone, without a handle or a GPU. */
    int gsh_gen_set_satellite(gsh_gen_t* g, int32_t sat, const float* table_a, const float* table_b, uint32_t period, uint32_t delay_samples,
        const int8_t* signs_a, int32_t len_a, const int8_t* signs_b, int32_t len_b, double doppler_hz, double start_phase_rad, double carrier_offset_hz);
    int gsh_gen_check_satellite(double fs_sps, const float* table_a, const float* table_b, uint32_t period, uint32_t delay_samples, const int8_t* signs_a,
        int32_t len_a, const int8_t* signs_b, int32_t len_b, double doppler_hz, double start_phase_rad, double carrier_offset_hz);
    int gsh_gen_set_noise(gsh_gen_t* g, int32_t enabled, uint64_t seed);
    /* the next sample to produce (below 2^63) */
    int gsh_gen_seek(gsh_gen_t* g, uint64_t sample_index);
    int gsh_gen_position(const gsh_gen_t* g, uint64_t* sample_index);
    /* the next n samples as complex64 at device_out (device memory, 8-byte aligned); synchronous.  GSH_ERR_STATE while a satellite is unset. */
    int gsh_gen_generate_device(gsh_gen_t* g, uint64_t n, void* device_out);
    /* the next n samples straight into the ring, which afterwards is what a push of those samples from the host would have left (resident range,
     * mirror, push event and history, live words); *first_index (may be NULL) = the ring index of the first.  Synchronous.  All or nothing, the
     * ring and the generator's position stay as they were: GSH_ERR_INVALID for a null ring, a ring on another device, n above the ring's
     * capacity; GSH_ERR_STATE for an unset satellite or a live tracking channel whose samples the push would overwrite. */
    int gsh_gen_push(gsh_gen_t* g, gsh_stream_t* ring, uint64_t n, uint64_t* first_index);
    /* average HIP-event time of generating n samples (at most 2^30) from the present position into a scratch buffer; the position stays */
    int gsh_gen_time_generate(gsh_gen_t* g, uint64_t n, int reps, float* avg_ms);
    /* the noise's word stage on the host (csrc/signal_generator.h, the text the kernel runs): the four Philox4x32-10 words of counter
     * (sample_index low, high, 0, 0) under key (seed low, high); I and Q of the sample come from words 0 and 1 */
    void gsh_gen_philox_words(uint64_t seed, uint64_t sample_index, uint32_t out[4]);
    /* bind a bank to a ring: from now on gsh_corr_job.sample_offset is an ABSOLUTE sample index; a job whose window is not
     * fully resident (or longer than max_window_samples) fails with GSH_ERR_INVALID.  NULL detaches.
     * Residency is checked when the job table is staged (gsh_bank_correlate / gsh_bank_upload_jobs): a table uploaded once and
     * launched repeatedly (gsh_bank_launch) keeps pointing at the ring positions it was translated to, so the caller must not push
     * past those windows in between.  The handles are not internally synchronised: one thread at a time per handle, and pushes
     * into a ring are serialised against the calls that read it (Hip_Correlator_Runtime does both for a receiver). */
    int gsh_bank_set_stream_ring(gsh_bank_t* b, gsh_stream_t* s);

    /* ================================================================ TRACKING LOOP (closed on the device)
     * gsh_trk_*: the steady-state loop of dll_pll_veml_tracking (trk.cc state 2, :1975-2001), one code period per
     * iteration:  do_correlation_step (trk.cc:1232-1257) -> run_dll_pll (:1260-1324: Costas / four-quadrant PLL
     * discriminator, fll_diff_atan, Tracking_FLL_PLL_filter, E-L or VEMLP DLL discriminator, Tracking_loop_filter,
     * carrier aiding) -> update_tracking_vars (:1409-1483) -> consume d_current_prn_length_samples (:2287),
     * with the initial conditions of start_tracking (:796-866) and the pull-in state (:1949-1973).
     * All of it runs on the GPU: one work-group per channel iterates over the code periods of a device-resident IF
     * stream and leaves one record per period, so n_epochs periods cost one launch instead of n_epochs host round
     * trips.  With enable_lock_detectors the C/N0 estimator, the carrier lock detector, their smoothers and the loss-of-lock
     * counters (cn0_and_tracking_lock_status, trk.cc:1167-1224; T/lock_detectors.cc, T/exponential_smoother.cc) run on the device
     * too, between the correlation and run_dll_pll as state 2 orders them (:2008-2018).  Not modelled here (the host block
     * keeps them): the experimental Doppler correction (:1326-1346).  Symbol synchronisation, narrow tracking, extended integration,
     * the histogram bit synchroniser and high dynamics are switched on by the corresponding gsh_trk_conf fields.
     * T/ = src/algorithms/tracking/libs/.
     */
    typedef struct gsh_trk gsh_trk_t;

    typedef struct gsh_trk_conf
    {
        double fs_in;                    /* Dll_Pll_Conf::fs_in */
        double code_chip_rate;           /* d_code_chip_rate [chips/s] */
        double signal_carrier_freq;      /* d_signal_carrier_freq [Hz] (carrier aiding, trk.cc:1320-1323) */
        double cfo_frequency_hz;         /* d_cfo_frequency_hz, trk.cc:1423 */
        uint32_t code_length_chips;      /* d_code_length_chips */
        uint32_t code_samples_per_chip;  /* d_code_samples_per_chip: 1, or 2 for the E1 sinBOC replica (trk.cc:289) */
        uint32_t vector_length;          /* samples per correlation, trk.cc:1243 */
        int32_t veml;                    /* 0: E/P/L, 1: VE/E/P/L/VL (trk.cc:609-650) */
        int32_t track_pilot;             /* also correlate the data-component code, 1 tap (trk.cc:1246-1256) */
        float early_late_space_chips;
        float very_early_late_space_chips;
        float pll_bw_hz, dll_bw_hz, fll_bw_hz;
        int32_t pll_filter_order;        /* 2 or 3 (T/tracking_FLL_PLL_filter.cc:23-54) */
        int32_t dll_filter_order;        /* 1..3 (T/tracking_loop_filter.cc:101-196) */
        int32_t enable_fll_pull_in, enable_fll_steady_state, carrier_aiding;
        int32_t cloop;                   /* d_cloop: 1 = Costas two-quadrant arctangent, 0 = four-quadrant */
        uint32_t pull_in_time_s;         /* Dll_Pll_Conf::pull_in_time_s, trk.cc:1912-1915 */
        float spc, slope, y_intercept;   /* dll_nc_e_minus_l_normalized parameters (trk.cc:1986, dll_pll_conf.h:55-57) */
        int32_t enable_lock_detectors;   /* 0: the loop never declares loss of lock (the host block runs the detectors) */
        int32_t cn0_samples;             /* Dll_Pll_Conf::cn0_samples, 1..GSH_MAX_CN0_SAMPLES (flag default 20) */
        int32_t cn0_min;                 /* [dB-Hz] (25) */
        int32_t max_code_lock_fail;      /* (50) */
        int32_t max_carrier_lock_fail;   /* (5000) */
        int32_t cn0_smoother_samples;    /* (200) divided by the code period in ms, trk.cc:683-686 */
        int32_t carrier_lock_test_smoother_samples; /* (25) */
        float cn0_smoother_alpha;        /* (0.002) */
        float carrier_lock_test_smoother_alpha;     /* (0.002) */
        double carrier_lock_th;          /* (0.7) */
        /* symbol synchronisation and the narrow-tracking state (trk.cc:2026-2104 and state 4, :2197-2252); 0 = the loop stays in state 2.
         * Per-signal values as the block's constructor sets them (trk.cc:196-300): GPS L1 C/A symbols_per_bit 20, secondary_code = the
         * 160-symbol telemetry preamble (GPS_CA_PREAMBLE_SYMBOLS_STR), has_secondary 0; Galileo E1 pilot symbols_per_bit 1,
         * secondary_code = the 25-chip E1C code, has_secondary 1; GPS L5 the NH codes.  extend_correlation_symbols > 1 adds the coherent
         * integration of trk.cc:2114-2149, 2156-2195: after synchronisation the loop filters are re-parameterised (dll_bw_narrow_hz and
         * pll_bw_narrow_hz over the stretched update interval, filter memories kept), the correlator spacing narrows, and the loop closes
         * once every extend_correlation_symbols periods on the accumulated correlators.  use_histogram_bit_sync adds the
         * HistogramBitSynchronizer of T/bit_synchronizer.cc in front of the preamble search, as the block configures it for signals
         * without a secondary code and more than one symbol per bit (trk.cc:1387-1406, 2046-2072). */
        int32_t enable_symbol_sync;
        int32_t symbols_per_bit;         /* d_symbols_per_bit */
        int32_t has_secondary;           /* d_secondary: in state 4 the correlators are multiplied by the secondary code chip */
        int32_t secondary_code_length;   /* d_secondary_code_length, <= GSH_MAX_SECONDARY */
        int32_t data_secondary_code_length; /* d_data_secondary_code_length */
        int32_t extend_correlation_symbols; /* Dll_Pll_Conf::extend_correlation_symbols (1) */
        uint8_t secondary_code[320];     /* characters '0' / '1' (d_secondary_code_string) */
        uint8_t data_secondary_code[320];
        float pll_bw_narrow_hz;          /* (5.0)  dll_pll_conf.h:49 */
        float dll_bw_narrow_hz;          /* (0.75) */
        float early_late_space_narrow_chips;      /* (0.15) */
        float very_early_late_space_narrow_chips; /* (0.5) */
        int32_t use_histogram_bit_sync;  /* d_use_histogram_bit_sync */
        int32_t bs_min_events_for_lock;  /* (10) dll_pll_conf.h:76 */
        int32_t bs_stable_best_required; /* (3) */
        int32_t bs_use_phase_dot_detector; /* (1) */
        float bs_min_prompt_mag;         /* (0.0) */
        int32_t enable_bit_sync_time_limit; /* 1: the fail-safe of trk.cc:2000-2007 -- a channel still in state 2 (no secondary code / bit synchronisation yet)
                                               more than bit_synchronization_time_limit_s whole seconds after the acquisition stamp is declared lost.  The
                                               adapters switch it on (the reference has no switch); needs enable_lock_detectors and enable_symbol_sync */
        double bs_dominance_ratio;       /* (0.6) */
        int32_t high_dyn;                /* Dll_Pll_Conf::high_dyn: the high-dynamics resampler + rotator (trk.cc:669-675) fed with the rate-of-change
                                            estimates of both NCO steps (trk.cc:1425-1443, 1458-1480) */
        uint32_t smoother_length;        /* (10) periods per average, <= GSH_MAX_SMOOTHER */
        uint32_t bit_synchronization_time_limit_s; /* (20) Dll_Pll_Conf::bit_synchronization_time_limit_s */
        int32_t enable_doppler_correction; /* Dll_Pll_Conf::enable_doppler_correction (false): the experimental one-shot re-initialisation of the carrier loop
                                              when the filtered code error averages more than 1 chip/s over 1000 loop updates after pull-in (trk.cc:1326-1346) */
    } gsh_trk_conf;
#define GSH_MAX_BITSYNC_BINS 64
#define GSH_MAX_SMOOTHER 32
#define GSH_MAX_CN0_SAMPLES 64
#define GSH_MAX_SECONDARY 320  /* the longest pattern the reference correlates: the 300-symbol GLONASS GNAV preamble */

    typedef struct gsh_trk_epoch         /* what log_data dumps per period (trk.cc:1599-1702), POD */
    {
        uint64_t sample_counter;         /* first sample of the correlated window */
        int32_t prn_length_samples;      /* d_current_prn_length_samples: samples consumed after this period */
        int32_t flags;                   /* bit 0: d_pull_in_transitory was set; bit 1: loss of lock declared in this period
                                            (trk.cc:1208-1221, "events" message 3): the channel stops, the record carries the
                                            correlator outputs and the detector values only, prn_length_samples = 0 */
        float corr[10];                  /* E,P,L or VE,E,P,L,VL as interleaved complex64 */
        float prompt_data[2];            /* d_Prompt_Data (track_pilot) */
        float rem_carr_phase_rad;
        float cn0_db_hz;                 /* d_CN0_SNV_dB_Hz (0 until cn0_samples periods have passed, or with the detectors off) */
        double carrier_doppler_hz, code_freq_chips, carr_phase_error_hz, carr_freq_error_hz, carr_error_filt_hz;
        double code_error_chips, code_error_filt_chips, rem_code_phase_samples, acc_carrier_phase_rad;
        double carrier_lock_test;        /* d_carrier_lock_test */
        int32_t state;                   /* d_state the period ran in: 2 wide tracking / symbol search, 3 coherent integration (no loop update:
                                            the loop fields of the record are 0), 4 narrow tracking (0 with symbol sync off) */
        int32_t symbol_flags;            /* bit 0: Flag_valid_symbol_output (a telemetry symbol leaves the block, trk.cc:2212-2236);
                                            bit 1: Flag_PLL_180_deg_phase_locked (trk.cc:1148-1156) */
        float p_data_accu[2];            /* d_P_data_accu: Prompt_I / Prompt_Q of the symbol when bit 0 is set, else the running sum */
        double carrier_phase_rate_step_rad; /* d_carrier_phase_rate_step_rad [rad/sample^2] after this period (0 outside high_dyn) */
        double code_phase_rate_step_chips;  /* d_code_phase_rate_step_chips [chips/sample^2] */
        float accu[10];                  /* d_VE_accu .. d_VL_accu as run_dll_pll / log_data saw them (E,P,L in slots 0..2 without veml): the period's
                                            outputs in state 2, the secondary-code-wiped running sums in states 3 / 4 (trk.cc:1486-1512, 1624-1636) */
    } gsh_trk_epoch;

    int gsh_trk_create(int device, const gsh_trk_conf* conf, int n_channels, int max_code_length, gsh_trk_t** out);
    void gsh_trk_destroy(gsh_trk_t* t);
    /* IF sample stream shared by every channel: _host copies, _device borrows 16-byte aligned device memory */
    int gsh_trk_set_stream_host(gsh_trk_t* t, const float* iq, uint64_t n_samples);
    int gsh_trk_set_stream_device(gsh_trk_t* t, const void* device_iq, uint64_t n_samples);
    /* follow a live sample ring: start_sample / sample_counter are absolute sample indices; every gsh_trk_run works through the
     * periods whose windows are resident at the time of the call and stops at the newest sample, the next call (after more pushes)
     * continues.  A channel whose next window has already been overwritten (it fell more than the ring's capacity behind) stops. */
    int gsh_trk_set_stream_ring(gsh_trk_t* t, gsh_stream_t* s);
    /* start_tracking (trk.cc:796-866) for one channel: local replica(s) (code_length floats = chips x samples per
     * chip; data_code NULL unless track_pilot), Acq_doppler_hz, Acq_samplestamp_samples, and the first sample of the
     * first code period, i.e. the stream position after the pull-in alignment of trk.cc:1949-1973 */
    int gsh_trk_start(gsh_trk_t* t, int channel, const float* code, const float* data_code, int code_length, uint64_t start_sample,
        uint64_t acq_sample_stamp, double acq_carrier_doppler_hz);
    /* the same with d_acc_carrier_phase_rad preset (the pull-in alignment subtracts step * samples_offset from it, trk.cc:1966) */
    int gsh_trk_start_ex(gsh_trk_t* t, int channel, const float* code, const float* data_code, int code_length, uint64_t start_sample,
        uint64_t acq_sample_stamp, double acq_carrier_doppler_hz, double initial_acc_carrier_phase_rad);
    /* The pull-in arithmetic of dll_pll_veml_tracking::general_work, state 1 (trk.cc:1949-1978), host only: with the block's read pointer at
     * absolute sample nitems_read and the acquisition's Acq_delay_samples / Acq_samplestamp_samples / Acq_doppler_hz, how many samples
     * to skip so that the next sample is a code start (samples_offset -> consume_each), the nominal first block length
     * (d_current_prn_length_samples = round(T_prn_mod_samples)), and d_acc_carrier_phase_rad after the skip.
     * start_sample for gsh_trk_start_ex is nitems_read + samples_offset. */
    int gsh_trk_pull_in(const gsh_trk_conf* conf, uint64_t nitems_read, double acq_delay_samples, uint64_t acq_sample_stamp, double acq_carrier_doppler_hz,
        int32_t* samples_offset, int32_t* first_prn_length_samples, double* acc_carrier_phase_rad);
    /* The pull-in transitory (d_pull_in_transitory, trk.cc:1073, 1910-1917) is a latch that EVERY general_work call looks at -- the pull-in call (state 1) included:
     *   pull_in_time_s < (nitems_read(0) - d_acq_sample_stamp) / (int)fs_in        in unsigned 64-bit arithmetic.
     * A tracking block whose read pointer is still BEHIND the acquisition's sample stamp at that call (it runs only when two code periods of input are there, the
     * acquisition block consumes whatever it is offered: tracking behind acquisition is the normal order of things in a flowgraph) wraps that difference round to
     * ~2^64 and the transitory is over before the first period: bit synchronisation starts at once and the lock detectors count from the first test.  Returns 1 when
     * that is the case for the pull-in call at read pointer nitems_read (host only) -> GSH_TRK_START_PULL_IN_OVER for gsh_trk_start_flags. */
    int gsh_trk_pull_in_over(const gsh_trk_conf* conf, uint64_t nitems_read, uint64_t acq_sample_stamp);
#define GSH_TRK_START_PULL_IN_OVER 1u
    /* gsh_trk_start_ex + flags (GSH_TRK_START_PULL_IN_OVER: the channel starts with the pull-in transitory already over, see above) */
    int gsh_trk_start_flags(gsh_trk_t* t, int channel, const float* code, const float* data_code, int code_length, uint64_t start_sample,
        uint64_t acq_sample_stamp, double acq_carrier_doppler_hz, double initial_acc_carrier_phase_rad, uint32_t flags);
    /* stop_tracking / clear_tracking_vars for one channel: the loop no longer advances it (its state stays readable) */
    int gsh_trk_stop(gsh_trk_t* t, int channel);
    /* n_epochs code periods of every started channel in ONE launch; the loop state stays on the device, so a later
     * call continues where this one stopped.  records: n_channels * n_epochs (channel-major) or NULL;
     * epochs_done[n_channels]: periods completed (a channel stops when its window would leave the stream). */
    int gsh_trk_run(gsh_trk_t* t, int n_epochs, gsh_trk_epoch* records, int32_t* epochs_done);
    /* Cooperating work-groups (round 6): `work_groups_per_channel` work-groups on different compute units share every window of a channel in LAUNCHED runs
     * (gsh_trk_run / _run_begin / _time_run; standard correlator only) -- each correlates its segment of the window, the channel's main work-group adds the partial
     * sums in a fixed order and runs the loop.  For few channels on a large device; MEASURED at 32 channels, 25 Msps: 7.29 us per period with one work-group,
     * 6.75 - 7.4 with two, 7.2 - 7.8 with four, ~9 with eight -- two hand-overs through L2 per period (~0.7 us each) eat most of what the shorter
     * correlation saves, so this is an option, not the default.  The sums are
     * formed in another order than with one work-group per channel, so records agree with that form to rounding (same bars against the oracle), not bit for bit;
     * live residencies always run one work-group per channel.  Needs (ceil(n_channels / 8) x 8 x work_groups_per_channel) compute units free at once; a partner
     * that does not get to run within 0.2 s ends the run with GSH_ERR_STATE instead of hanging the device.  1 = off (default).
     * Where it pays is the LONG window: BASELINE config 4 (50 channels, 128 000 samples, 5 + 1 taps) 36.5 us per period with one work-group, 22.0 with two,
     * 16.1 with four.  0 = choose by the window's length in trips and the compute units the channels leave free (2 for 25 000-sample E/P/L windows, 4 for config 4). */
    int gsh_trk_set_split(gsh_trk_t* t, int work_groups_per_channel);
    /* the same in two halves, for a caller that serialises launches against pushes into the ring itself (Hip_Tracking_Runtime): _begin queues
     * the launch on the loop's stream -- the kernel writes its results into page-locked host memory itself (GSH_TRK_HOST_RECORDS=0 in the environment:
     * into device memory, with two copies queued behind it) -- and returns at once; it is the only part
     * that looks at the ring's bookkeeping (newest sample, reader fences), so the ring's lock is needed around it alone and the next block of
     * samples can travel while the kernel runs; _end waits for the stream and hands the results over.  One launch in flight per handle. */
    int gsh_trk_run_begin(gsh_trk_t* t, int n_epochs, int want_records);
    int gsh_trk_run_end(gsh_trk_t* t, gsh_trk_epoch* records, int32_t* epochs_done);
    /* ---- live mode: the loop follows the ring as it fills, without a launch per batch of periods.
     * In the reference every channel's block is called once per code period (trk.cc:1898-2001) off one shared buffer
     * (src/core/receiver/gnss_flowgraph.cc:1227-1231); at that cadence a launch per call is all host time.  gsh_trk_live_begin queues a RESIDENCY of the loop
     * kernel instead: every started channel correlates its next window as soon as the ring (gsh_trk_set_stream_ring) holds it -- pushes announce
     * themselves to the resident kernel through the ring, no event, no host --, and leaves one record per period in a ring of records in page-locked
     * host memory that gsh_trk_live_take reads without a lock or a device call.  A residency ends by itself when nothing new has arrived for
     * idle_timeout_us (1000), after residency_us (20000: anything that waits for the whole device gets its turn), when the host asks (gsh_trk_live_quiesce)
     * or when no channel has work; up to two may be queued, the second takes over when the first ends.  Loop arithmetic, records and trajectories are
     * those of gsh_trk_run, bit for bit.
     * Threads: _begin, _in_flight, _quiesce, start, stop, run*: one at a time per handle (the caller's lock).  _take: any thread, at most one per
     * CHANNEL at a time, concurrently with everything except start / stop of that channel and gsh_trk_destroy.
     * Pushes into the ring never overwrite samples a live channel has not correlated yet: they fail with GSH_ERR_STATE instead (an event cannot order
     * a push behind a kernel that is waiting for that push); the caller keeps its pushes below lowest next window + ring capacity. */
    int gsh_trk_live_configure(gsh_trk_t* t, uint32_t idle_timeout_us, uint32_t residency_us);
    int gsh_trk_live_begin(gsh_trk_t* t);
    int gsh_trk_live_in_flight(gsh_trk_t* t, int32_t* residencies);  /* queued or running */
    /* up to max_records finished periods of one channel, oldest first, whose samples lie below limit_end (sample_counter + max(vector_length,
     * prn_length_samples) <= limit_end; UINT64_MAX: no limit).  A record with flags bit 1 (loss of lock) ends the take and is the channel's last.
     * *pending: records finished and not taken; *next_window: first sample of the window behind the last record taken; *active: the device still
     * advances the channel; *resident: the channel's work-group is inside a running residency right now (0: it has left -- idle, time budget, quit --
     * or none has started yet: a caller that waits for a record then knows to ask for one, without a device call). */
    int gsh_trk_live_take(gsh_trk_t* t, int channel, uint64_t limit_end, int max_records, gsh_trk_epoch* out, int32_t* n_out, int32_t* pending,
        uint64_t* next_window, int32_t* active, int32_t* resident);
    /* tell the residencies in flight to leave, wait for them; records not yet taken stay where they are.  Needed before start / stop / run. */
    int gsh_trk_live_quiesce(gsh_trk_t* t);
    /* where every channel stands after the last completed run (host copy, refreshed by gsh_trk_run / _run_end and by start / stop):
     * next_window[ch] = absolute index of the first sample of the channel's next correlation window, active[ch] != 0 while the loop advances it */
    int gsh_trk_positions(gsh_trk_t* t, uint64_t* next_window, int32_t* active);
    /* HIP-event milliseconds of one gsh_trk_run-sized launch, averaged over reps (each rep restarts from the state at
     * entry; the state is restored afterwards) */
    int gsh_trk_time_run(gsh_trk_t* t, int n_epochs, int reps, float* avg_ms);
    /* ---- Kalman-filter loop: the reference's second tracking family, kf_tracking (kf.cc = src/algorithms/tracking/gnuradio_blocks/kf_tracking.cc,
     * Kf_Conf = T/kf_conf.{h,cc}, adapter gps_l1_ca_kf_tracking).  It drives the same correlator and the same state machine as dll_pll_veml_tracking --
     * pull-in, state 2, secondary-code / bit synchronisation, states 3 and 4, lock detectors, C/N0 -- and differs in run_Kf (kf.cc:1143-1218) in place of
     * run_dll_pll, in its update_tracking_vars (:1251-1327) and in init_kf / update_kf_narrow_integration_time / update_kf_cn0 (:871-969): a four-state
     * filter x = [code phase (chips), carrier phase (rad), Doppler (Hz), Doppler rate (Hz/s)] fed with the code and the carrier discriminator
     * (csrc/kalman_step.h: the arithmetic, FP64, with the order of every sum written out).  gsh_trk_set_kalman switches a handle to that loop (NULL: back
     * to DLL/PLL); only while no channel is started.  GSH_ERR_INVALID: high_dyn (the smoother that overwrites the Doppler rate, kf.cc:1269-1291, is not
     * modelled), enable_doppler_correction (kf_tracking has none), a split other than 1, enable_symbol_sync without enable_lock_detectors (state 4 rebuilds
     * R from the C/N0 estimate, kf.cc:1973), a standard deviation that is negative or not finite.  GSH_ERR_STATE: a channel is active, a run or a live
     * residency is in flight.  On a Kalman handle gsh_trk_set_split(!= 1) and gsh_trk_live_begin return GSH_ERR_INVALID (launched runs of one work-group per
     * channel only); start*, run, run_begin / _end, time_run (which saves and restores the filters too), positions, stop and the stream setters work unchanged.
     * IGNORED in Kalman mode: pll_bw_hz, pll_bw_narrow_hz, dll_bw_hz, dll_bw_narrow_hz, fll_bw_hz, pll_filter_order, dll_filter_order (still range-checked by
     * gsh_trk_create), enable_fll_pull_in, enable_fll_steady_state, carrier_aiding and cfo_frequency_hz (kf.cc:1265 has no offset term).  Note Kf_Conf's own
     * defaults: early_late_space_chips 0.25, bit_synchronization_time_limit_s = pull_in_time_s + 60 (kf_conf.cc:49, 110).
     * gsh_trk_epoch keeps its layout and carries what kf_tracking::log_data logs (kf.cc:1443-1539): carrier_doppler_hz = x[2], code_freq_chips =
     * d_code_freq_kf_chips_s, carr_phase_error_hz = carrier discriminator / 2 pi, carr_error_filt_hz = x[2], carr_freq_error_hz = x[3] (Doppler rate, Hz/s),
     * code_error_chips = code discriminator, code_error_filt_chips = d_code_error_kf_chips (all 0 in a state-3 period, as in the DLL/PLL loop); everything
     * else as there.  The reference's KF dump file (96 bytes per period) differs from the 108-byte DLL/PLL dump gsh_trk_write_dump writes: not provided. */
    typedef struct gsh_trk_kf_conf            /* Kf_Conf, kf_conf.h:40-55; defaults kf_conf.cc:39-48 */
    {
        double code_disc_sd_chips, carrier_disc_sd_rads;                       /* R   (0.2, 0.3) */
        double code_phase_sd_chips, carrier_phase_sd_rad, carrier_freq_sd_hz, carrier_freq_rate_sd_hz_s;   /* Q   (0.15, 0.25, 0.6, 0.01) */
        double init_code_phase_sd_chips, init_carrier_phase_sd_rad, init_carrier_freq_sd_hz, init_carrier_freq_rate_sd_hz_s; /* P0  (0.5, 0.7, 5, 1) */
    } gsh_trk_kf_conf;
    int gsh_trk_set_kalman(gsh_trk_t* t, const gsh_trk_kf_conf* kf);
    /* the channel's filter after the last completed run: x[4], P[16] row-major, the diagonal of R (each may be NULL) */
    int gsh_trk_kf_state(gsh_trk_t* t, int channel, double x[4], double P[16], double R[2]);
    /* write (append != 0: append) the records of one channel as a tracking dump file in the block's own binary layout
     * (log_data, trk.cc:1599-1702: 19 floats, the PRN start sample as uint64 and as double, PRN, TOW [ms] as uint64, week number =
     * 108 bytes per logged period -- the layout save_matfile (trk.cc:1705-1716) and utils/matlab/libs/dll_pll_veml_read_tracking_dump.m
     * parse).  Host-only.  Logged are the periods the block logs: every period of state 2, the symbol periods of states 3 / 4
     * (trk.cc:2024, 2166, 2218); periods flagged as loss of lock are skipped, as the reference skips log_data there.  tow_ms / wn: one
     * value per record (d_tow_from_telemetry_ms / d_wn_from_telemetry of that call, trk.cc:1921-1935) or NULL for zeros. */
    int gsh_trk_write_dump(const char* path, int append, const gsh_trk_conf* conf, uint32_t prn, const gsh_trk_epoch* records, int n_records,
        const uint64_t* tow_ms, const uint32_t* wn);

    /* ================================================================ ACQUISITION
     * gsh_acq_*: the arithmetic of class pcps_acquisition (acq.h:93-251) without its
     * GNU Radio shell: set_local_code (acq.cc:218-251), update_grid_doppler_wipeoffs
     * (acq.cc:284-291), doppler_grid (acq.cc:522-560), both statistics (acq.cc:409-519).
     * One handle searches n_prn local codes against the same input block in one go
     * (the reference runs one block per channel, each recomputing the D forward FFTs).
     */
    typedef struct gsh_acq gsh_acq_t;

    typedef struct gsh_acq_conf
    {
        int64_t fs_in;              /* Acq_Conf::fs_in (resampled_fs when the resampler is on), acq.cc:277 */
        uint32_t fft_size;          /* d_fft_size, acq.cc:111.  Any length: on-chip plans for the common ones, a four-step split for prime factors
                                       <= 61, and for the rest (plain searches) a zero-padded power-of-two form of the same circular correlation */
        uint32_t effective_fft_size; /* d_effective_fft_size, acq.cc:112 */
        uint32_t consumed_samples;  /* d_consumed_samples, acq.cc:110 */
        uint32_t num_doppler_bins;  /* d_num_doppler_bins, acq.cc:113; 0 = ceil(2*doppler_max/doppler_step) */
        int32_t doppler_max;        /* Acq_Conf::doppler_max */
        int32_t doppler_step;       /* Acq_Conf::doppler_step */
        int32_t doppler_center;     /* set_doppler_center, acq.cc:737-746 */
        int32_t doppler_bias;       /* GLONASS FDMA offset, acq.cc:254-272; 0 otherwise */
        uint32_t samples_per_chip;  /* Acq_Conf::samples_per_chip, acq_conf.cc:122 */
        float samples_per_code;     /* Acq_Conf::samples_per_code, acq_conf.cc:123 */
        int32_t bit_transition_flag; /* acq.cc:230-235,544 */
        int32_t use_cfar;           /* d_use_CFAR_algorithm_flag: 1 = max_to_input_power, 0 = first_vs_second_peak */
        uint32_t max_prn;           /* how many local codes this handle can hold */
        int32_t no_grid;            /* 0: the |.|^2 grid d_magnitude_grid (acq.cc:137) is kept in device memory, as the
                                       reference keeps it (needed by accumulate != 0, i.e. max_dwells > 1, and by
                                       gsh_acq_read_grid, i.e. dump).  1: the caller promises neither; lengths with an
                                       on-chip plan then never write the grid (statistics are formed on chip) */
        int32_t transform_path;     /* 0: automatic (whole transform on one CU when the length has a plan, else the
                                       four-step path through HBM); 1: force the four-step path (A/B testing) */
        uint32_t num_doppler_bins_step2; /* Acq_Conf::num_doppler_bins_step2 (acq_conf.h:62, key second_nbins); 0 = the handle
                                       never runs the fine-Doppler step (make_two_steps = false); must be <= num_doppler_bins */
        float doppler_step2;        /* Acq_Conf::doppler_step2 (acq_conf.h:50, key second_doppler_step) */
        uint32_t fold;              /* 0 or 1: off.  > 1 (QuickSync, pcps_quicksync_acquisition_cc.cc:243-263): the input block is
                                       fold * fft_size samples (= consumed_samples); after the Doppler wipe-off its `fold` segments
                                       are added into one fft_size-long block before the forward transform.  The block passes
                                       folding_factor^2; set_local_code takes the code already folded to fft_size (:137-152) */
    } gsh_acq_conf;

    typedef struct gsh_acq_result
    {
        uint32_t index_time;        /* AcquisitionResult::index_time  (lowest index on ties) */
        uint32_t index_doppler;     /* winning Doppler bin (first bin on ties, acq.cc:420) */
        int32_t doppler_hz;         /* AcquisitionResult::doppler, acq.cc:431 */
        float acq_delay_samples;    /* fmod((float)index_time, samples_per_code), acq.cc:582 */
        float peak;                 /* grid maximum */
        float input_power;          /* d_input_power (CFAR only), acq.cc:430 */
        float second_peak;          /* peak-ratio statistic only, acq.cc:511-513 */
        float test_statistics;      /* acq.cc:439-445 or :516 */
    } gsh_acq_result;

    int gsh_acq_create(int device, const gsh_acq_conf* conf, gsh_acq_t** out);
    void gsh_acq_destroy(gsh_acq_t* a);
    /* acq.cc:218-251: place the time-domain replica per the padding rules, FFT, conjugate.
     * `code_iq` holds consumed_samples complex samples (fft_size/2 when bit_transition_flag). */
    int gsh_acq_set_local_code(gsh_acq_t* a, uint32_t prn_slot, const float* code_iq);
    /* acq.cc:737-746 */
    int gsh_acq_set_doppler_center(gsh_acq_t* a, int32_t doppler_center);
    /* acq.cc:252-272 (is_fdma): GLONASS L1 / L2 satellites sit on their own FDMA carrier, DFRQ{1,2}_GLO * channel number away from
     * the band centre; the offset is re-derived whenever the PRN changes and enters only the wipe-off frequency (acq.cc:289), never
     * the reported Doppler.  Applies to every prn slot of the handle: search GLONASS satellites one frequency channel per handle. */
    int gsh_acq_set_doppler_bias(gsh_acq_t* a, int32_t doppler_bias);
    /* The other PCPS detectors on the same engine:
     * pcps_tong_acquisition_cc.cc:243-249 scales every |y|^2 by 1 / (fft_norm^2 * input_power) BEFORE adding it to its
     * d_grid_data; `weight` is that factor, applied (one float multiply per cell) to every magnitude that is added to or
     * stored in the grid by the dwells that follow.  Default 1 (the multiply is then exact).  Needs no_grid == 0 when != 1. */
    int gsh_acq_set_grid_weight(gsh_acq_t* a, float weight);
    /* mean |x|^2 of the consumed_samples block most recently handed to the handle -- d_input_power of
     * pcps_tong_acquisition_cc.cc:208-210 and galileo_pcps_8ms_acquisition_cc.cc:190-192.  Per-sample terms are the
     * reference's float values; they are summed in double (the reference's float VOLK accumulator has no defined lane
     * order), so the value agrees with the reference to float rounding of the sum (~1e-7 relative), not bit for bit. */
    int gsh_acq_input_power(gsh_acq_t* a, float* mean_power);
    /* The Tong weight of a block depends on that block's own power, so the block must be resident before its dwell is
     * queued: stage_input[_device] copies consumed_samples complex64 samples into the handle (what gsh_acq_dwell[_device]
     * do first), dwell_resident then runs the dwell of gsh_acq_dwell over the resident block. */
    int gsh_acq_stage_input(gsh_acq_t* a, const float* in_iq);
    int gsh_acq_stage_input_device(gsh_acq_t* a, const void* device_in_iq);
    int gsh_acq_dwell_resident(gsh_acq_t* a, uint32_t n_prn, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    /* per-Doppler-bin maximum and its (lowest) time index of prn_slot's grid after the last full dwell -- magt / indext of
     * the per-bin loops of galileo_pcps_8ms_acquisition_cc.cc:226-262, which compares two local codes bin by bin.
     * num_doppler_bins entries each. */
    int gsh_acq_read_row_peaks(gsh_acq_t* a, uint32_t prn_slot, float* row_peak, uint32_t* row_index_time);
    /* Non-coherent I + Q combination of galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:357-492 after a dwell over the block's local
     * codes held in four slots of this handle: data component "A" (1,1,1) in slot_ia, pilot "A" in slot_qa (-1: data only,
     * d_both_signal_components false), and for coherent times above one code period the "B" combinations with the first period
     * inverted in slot_ib / slot_qb (-1: d_sampled_ms == 1).  Per Doppler bin the component's A or B row is kept as the block keeps it
     * (row maxima / N^4 compared with >=, :403, :410 -- the Q-B candidate ranked by the I-B row at Q-B's arg-max, as :393 is written),
     * the two kept magnitude rows are ADDED cell by cell on the device (:419-431) and the maximum of the sum with its lowest index is
     * returned (:487-492), together with the two row maxima the CAF filter works on (:405-427).  num_doppler_bins records.
     * Needs the stored grid (no_grid = 0). */
    typedef struct gsh_acq_pair_peak
    {
        float peak;           /* d_magnitudeI[indext] after the addition, unnormalised */
        uint32_t index_time;  /* indext */
        float caf_i;          /* d_CAF_vector_I[doppler_index] */
        float caf_q;          /* d_CAF_vector_Q[doppler_index] (0 without a pilot slot) */
        uint32_t i_slot;      /* the slots whose rows were added */
        uint32_t q_slot;      /* 0xFFFFFFFF: none */
    } gsh_acq_pair_peak;
    int gsh_acq_noncoherent_pair_peaks(gsh_acq_t* a, int32_t slot_ia, int32_t slot_qa, int32_t slot_ib, int32_t slot_qb, gsh_acq_pair_peak* out);
    /* QuickSync's de-ambiguation (pcps_quicksync_acquisition_cc.cc:295-323): time-domain correlation of the resident block,
     * wiped off at Doppler bin `doppler_index`, with the UNfolded code (code_len complex64 samples, host memory) at n_delays
     * (<= 100) candidate delays: out[c] = sum_j x[delays[c] + j] w[delays[c] + j] code[j].  Float products as the reference forms
     * them, summed in double (the reference adds sequentially in float: agreement ~1e-6 relative, not bit for bit). */
    int gsh_acq_time_correlate(gsh_acq_t* a, const float* code_iq, uint32_t code_len, uint32_t doppler_index, const uint32_t* delays,
        uint32_t n_delays, float* out_iq);
    /* one acquisition_core pass (acq.cc:648-684) for prn_slot 0..n_prn-1 over the same
     * consumed_samples input block.  `accumulate` != 0 adds to the stored grids
     * (non-coherent dwell number > 1, acq.cc:549-553); `dwell_count` is
     * d_num_noncoherent_integrations_counter after the increment (acq.cc:668), used by the
     * CFAR power normalisation (acq.cc:430). */
    int gsh_acq_dwell(gsh_acq_t* a, const float* in_iq, uint32_t n_prn, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    /* One dwell for an arbitrary subset of the handle's local codes: results[i] belongs to prn_slots[i].  First dwell of a search only
     * (accumulate = 0, dwell count 1) and statistics only: whatever grid the handle stores is indexed by position i for this call, not by slot.
     * This is what lets the channels of a receiver that search the same input block at the same time share one batch -- the D forward transforms
     * are computed once for all of them instead of once per channel (Hip_Acquisition_Runtime; the reference runs one pcps_acquisition block per
     * channel, each recomputing them, acq.cc:522-560). */
    int gsh_acq_dwell_slots(gsh_acq_t* a, const float* in_iq, uint32_t n, const uint32_t* prn_slots, gsh_acq_result* results);
    /* same with the input block already in device memory (16-byte aligned) */
    int gsh_acq_dwell_device(gsh_acq_t* a, const void* device_in_iq, uint32_t n_prn, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    /* Step two of make_two_steps (acq.cc:294-301, 522-560 with d_step_two, 428-437 / 475-482): for each i < n a narrow
     * grid of num_doppler_bins_step2 bins at  center[i] + ((float)d - floor(nbins2/2)) * doppler_step2  (float arithmetic,
     * acq.cc:298-299) for local code prn_slots[i] over one consumed_samples block.  `doppler_center_step_two[i]` is the
     * step-one result's Doppler (acq.cc:619); `input_power_step_one[i]` is d_input_power left by step one -- the CFAR
     * statistic of step two divides by it without recomputing it (acq.cc:428-445); ignored for the peak-ratio statistic.
     * results[i].doppler_hz = (int32_t)(center + ((float)index_doppler - floor(nbins2/2)) * doppler_step2) (acq.cc:436).
     * `accumulate`/`dwell_count` as in gsh_acq_dwell (non-coherent dwells inside step two, acq.cc:545-553). */
    int gsh_acq_dwell_step2(gsh_acq_t* a, const float* in_iq, uint32_t n, const uint32_t* prn_slots, const float* doppler_center_step_two,
        const float* input_power_step_one, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    int gsh_acq_dwell_step2_device(gsh_acq_t* a, const void* device_in_iq, uint32_t n, const uint32_t* prn_slots,
        const float* doppler_center_step_two, const float* input_power_step_one, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    /* item_type = cshort (acq.cc:653-656): `in_iq16` holds consumed_samples interleaved int16 I,Q pairs, converted to
     * complex64 on the device (volk_gnsssdr_16ic_convert_32fc: exact int -> float), then as gsh_acq_dwell */
    int gsh_acq_dwell_cshort(gsh_acq_t* a, const int16_t* in_iq16, uint32_t n_prn, int accumulate, uint32_t dwell_count, gsh_acq_result* results);
    /* the input block is consumed_samples resident samples of a device ring starting at absolute index first_sample (the ring's
     * max_window_samples must cover consumed_samples): what the acquisition block copies out of its input buffer (acq.cc:790-815) */
    int gsh_acq_dwell_ring(gsh_acq_t* a, gsh_stream_t* ring, uint64_t first_sample, uint32_t n_prn, int accumulate, uint32_t dwell_count,
        gsh_acq_result* results);
    /* dump support (acq.cc:555-558): copy |.|^2 grid of one PRN, D rows of effective_fft_size floats */
    int gsh_acq_read_grid(gsh_acq_t* a, uint32_t prn_slot, float* grid);
    /* HIP-event average milliseconds per full dwell batch (n_prn codes), inputs resident */
    int gsh_acq_time_dwells(gsh_acq_t* a, uint32_t n_prn, int reps, float* avg_ms);
    /* the same stream of `reps` dwell batches issued alternately on two HIP streams with per-batch spectra / row /
     * result buffers, so batch k+1's forward transforms and first cells run on the compute units batch k's tail
     * leaves idle: average milliseconds per batch in steady state (throughput; the single-batch latency is what
     * gsh_acq_time_dwells reports).  Statistics only (as no_grid = 1); lengths without an on-chip plan fall back to
     * gsh_acq_time_dwells. */
    int gsh_acq_time_dwells_pipelined(gsh_acq_t* a, uint32_t n_prn, int reps, float* avg_ms);

    /* ---- pulse blanking (input filter in front of the channels) ---------------------------------------------------------------
     * pulse_blanking_cc (src/algorithms/input_filter/gnuradio_blocks/pulse_blanking_cc.cc:33-106; adapter key
     * InputFilter.implementation=Pulse_Blanking_Filter, pulse_blanking_filter.cc: pfa, length, segments_est, segments_reset): the
     * stream is tiled into `length`-sample segments; a segment whose energy over the estimated noise power exceeds the chi-squared
     * (2 * length degrees of freedom) threshold for `pfa` is zeroed.  State (noise estimate, segment counter, last_filtered) lives on
     * the device and carries over between calls. */
    typedef struct gsh_pulse_blanking gsh_pb_t;
    int gsh_pb_create(int device, float pfa, int32_t length, int32_t n_segments_est, int32_t n_segments_reset, gsh_pb_t** out);
    void gsh_pb_destroy(gsh_pb_t* p);
    float gsh_pb_threshold(const gsh_pb_t* p); /* thres_, pulse_blanking_cc.cc:48-49 */
    /* one general_work call (:57-106) over n_items resident complex64 samples: whole segments are filtered while
     * (index + length) < n_items, exactly as the block consumes them; *n_done = samples consumed = samples produced (the caller
     * presents the remainder again, followed by new samples, like the GNU Radio scheduler does).  In-place (out == in) is allowed. */
    int gsh_pb_process_device(gsh_pb_t* p, const void* device_in_iq, uint64_t n_items, void* device_out_iq, uint64_t* n_done);
    int gsh_pb_get_state(gsh_pb_t* p, float* noise_power_estimation, int32_t* n_segments, int32_t* last_filtered);

    /* Notch (src/algorithms/input_filter/gnuradio_blocks/notch_cc.cc:33-140; adapter Notch_Filter: pfa, p_c_factor, length, segments_est,
     * segments_reset) and NotchLite (.../notch_lite_cc.cc:30-150; adapter Notch_Filter_Lite, n_segments_coeff = coeff_rate-derived) -- continuous-wave
     * interference excision: segments of `length` samples whose energy over the estimated noise floor exceeds the chi-squared threshold for `pfa`
     * go through  out[n] = in[n] - z0 in[n-1] + p_c_factor z0 out[n-1];  the others pass unchanged.  n_segments_coeff = 0: Notch (z0 per sample
     * from the phase of in[n] conj(in[n-1])); >= 1: NotchLite (one z0 per that many filtered segments).  The floor estimate (FFT-based spectral
     * noise floor of the first n_segments_est segments after each reset), the segment counter, the filter state and the last output live on the
     * device and carry over between calls. */
    typedef struct gsh_notch gsh_notch_t;
    int gsh_notch_create(int device, float pfa, float p_c_factor, int32_t length, int32_t n_segments_est, int32_t n_segments_reset, int32_t n_segments_coeff,
        gsh_notch_t** out);
    void gsh_notch_destroy(gsh_notch_t* p);
    float gsh_notch_threshold(const gsh_notch_t* p); /* thres_, notch_cc.cc:54-55 */
    /* one general_work call over n_items resident complex64 items, of which item 0 is the sample IN FRONT of the first one processed (notch_cc.cc:71
     * `in++`; NotchLite's set_history(2) item): whole segments are taken while (index + length) < n_items; *n_done = items consumed = samples produced
     * (out[k] is the filtered in[k + 1]); the caller presents the rest again like the GNU Radio scheduler does.  Not in place. */
    int gsh_notch_process_device(gsh_notch_t* p, const void* device_in_iq, uint64_t n_items, void* device_out_iq, uint64_t* n_done);
    int gsh_notch_get_state(gsh_notch_t* p, float* noise_pow_est, int32_t* n_segments, int32_t* filter_state, float* last_out_iq, int32_t* n_segments_coeff,
        float* z0_iq);

    /* Fine-Doppler step of pcps_acquisition_fine_doppler_cc (gnuradio_blocks/pcps_acquisition_fine_doppler_cc.cc:316-389): the
     * n complex64 samples x (host), multiplied element-wise by w when w != NULL (the aligned code replica: code wipe-off, :348), are
     * zero-padded to fft_size, transformed, and the index of the largest |X[k]|^2 (lowest k among equal maxima, :354-358) is returned;
     * `peak` (nullable) receives that |X|^2.  fft_size needs a four-step split (n1 <= 1024, n2 <= 2048, prime factors <= 61):
     * up to ~2 M points, i.e. the block's 80 x samples_per_ms up to 25 Msps. */
    int gsh_spectrum_peak(int device, const float* x_iq, const float* w_iq, uint32_t n, uint32_t fft_size, uint32_t* index, float* peak);

    /* compute_threshold, acq.cc:52-56: 2*gamma_p_inv(2*max_dwells, (1-pfa)^(1/(effective*bins))) */
    float gsh_acq_compute_threshold(float pfa, uint32_t effective_fft_size, uint32_t num_doppler_bins, uint32_t max_dwells);

    /* ---- Galileo telemetry pages (I/NAV on E1B / E5b, F/NAV on E5a, C/NAV on E6) ------------------------------------------------
     * The page decoder of galileo_telemetry_decoder_gs (src/algorithms/telemetry_decoder/gnuradio_blocks/galileo_telemetry_decoder_gs.cc):
     * deinterleaver (:352-361), the NOT gate of G2 (:371-377), Viterbi_Decoder::decode (libs/viterbi_decoder.cc:47-120; K = 7, rate 1/2,
     * generators 121 / 91), CRC-24Q (boost::crc_optimal<24, 0x1864CFBU, 0, 0, false, false> of galileo_{inav,fnav,cnav}_message.cc), and the
     * clipped preamble correlation of the frame synchroniser (:962-972).  The symbols are the p_data_accu[0] of the gsh_trk_epoch records
     * whose symbol_flags bit 0 is set.  Page contents are not decoded here.
     * metric_mode GSH_TLM_METRIC_FULL: both symbols of a pair enter the branch metric and every page starts from state 0 alone -- a
     * maximum-likelihood decoder.  GSH_TLM_METRIC_REFERENCE: the reference as it runs -- only the first symbol of each pair enters
     * (viterbi_decoder.cc:61 copies d_nn - 1 elements) and, but for element 0 (:56), a page starts from the metrics the channel's previous
     * page ended with; those 64 floats per channel live in the handle between pages and launches.  |symbol| <= 1e5 in that mode. */
#define GSH_TLM_METRIC_FULL 0
#define GSH_TLM_METRIC_REFERENCE 1
#define GSH_TLM_MAX_CHANNELS 65536
#define GSH_TLM_JOB_INVERT 1u       /* negate every symbol: the 180 deg lock, galileo_telemetry_decoder_gs.cc:1040-1046 */
#define GSH_TLM_JOB_CRC_CONTINUE 2u /* the CRC register continues from this channel's previous job instead of starting at zero */
#define GSH_TLM_JOB_INAV_AUTO 4u    /* frame type 1 only: the page's first bit chooses the CRC work (galileo_inav_message.cc:146-177) -- 0, an even
                                       part: register from zero, 114 bits, no comparison; 1, an odd part: continue, 82 bits, compare.  crc_bits,
                                       crc_check and GSH_TLM_JOB_CRC_CONTINUE of the job are then ignored */
    typedef struct gsh_tlm gsh_tlm_t;
    typedef struct
    {
        int32_t channel;
        int32_t frame_type;     /* d_frame_type: 1 I/NAV page part (240 symbols, 114 bits), 2 F/NAV (488, 238), 3 C/NAV (984, 486) */
        uint64_t symbol_offset; /* the first symbol after the preamble */
        uint32_t flags;         /* GSH_TLM_JOB_* */
        int32_t crc_bits;       /* bits fed to the CRC from the page's first, 0 for none */
        int32_t crc_check;      /* nonzero: compare the 24 bits that follow with the register */
        int32_t reserved;
    } gsh_tlm_page_job; /* 32 bytes */
    typedef struct
    {
        uint32_t bits[16];     /* the information bits, MSB first: bit t is bit 31 - t % 32 of word t / 32; the rest is 0 */
        uint32_t crc_register; /* after crc_bits bits */
        int32_t crc_ok;        /* 1 / 0, or -1 when nothing was compared */
    } gsh_tlm_page_result; /* 72 bytes */
    int gsh_tlm_create(int device, int n_channels, int metric_mode, gsh_tlm_t** out);
    void gsh_tlm_destroy(gsh_tlm_t* h);
    /* a fresh Viterbi_Decoder and a CRC register of zero for one channel (what a new telemetry block starts with) */
    int gsh_tlm_channel_reset(gsh_tlm_t* h, int channel);
    /* the range checks of a job table, on the host alone: GSH_ERR_INVALID for a window that leaves the n_symbols of the buffer, an unknown
     * frame type or flag, a channel >= n_channels, crc_bits (+ 24 with crc_check) beyond the page.  The decode entry points run it before any launch */
    int gsh_tlm_check_jobs(int n_channels, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs);
    /* galileo_telemetry_decoder_gs.cc:962-972 at every position of a block of n host symbols: corr_out[i] = sum_k pre[k] * (symbols[i + k] < 0 ? -1 : +1)
     * for the preamble of frame_type (10, 12 or 16 symbols); the positions whose window leaves the block, i > n - length, receive 0 */
    int gsh_tlm_preamble_scan(gsh_tlm_t* h, int frame_type, const float* symbols, uint64_t n, int8_t* corr_out);
    /* decode_INAV_word / decode_FNAV_word / decode_CNAV_word up to the CRC verdict (:364-560) for every job of the table.  Jobs of one channel are
     * taken in table order, channels may interleave in any way.  symbols: n_symbols host floats; jobs and results: host arrays of n_jobs */
    int gsh_tlm_decode_pages(gsh_tlm_t* h, const float* symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs, gsh_tlm_page_result* results);
    /* the same over n_symbols floats resident on the handle's device (borrowed for the call) */
    int gsh_tlm_decode_pages_device(gsh_tlm_t* h, const void* device_symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs,
        gsh_tlm_page_result* results);
    /* HIP-event average milliseconds per launch of the job table, inputs resident (the carried state of the channels moves on) */
    int gsh_tlm_time_decode_pages(gsh_tlm_t* h, const float* symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs, int reps, float* avg_ms);

    /* ---- GPS CNAV messages (L2C, L5) ---------------------------------------------------------------------------------------------
     * libswiftcnav's streaming decoder (src/algorithms/telemetry_decoder/libs/libswiftcnav/cnav_msg.c, viterbi27.c, bits.c, edc.c) as the
     * blocks gps_l2c_telemetry_decoder_gs and gps_l5_telemetry_decoder_gs drive it: per channel two sliding-window K = 7 rate 1/2 Viterbi
     * decoders one symbol apart with integer metrics, each with its message-lock machine (preamble 0x8B or its inverse, 300 bits, CRC-24Q
     * over 276).  State lives in the handle from symbol to symbol; results equal the reference bit for bit on every input.  The symbols are
     * the p_data_accu[0] (L2C, Prompt_I) or p_data_accu[1] (L5, Prompt_Q) of the gsh_trk_epoch records whose symbol_flags bit 0 is set.
     * Message contents beyond prn, msg_id, tow and alert are not decoded here. */
#define GSH_CNAV_MAX_CHANNELS 65536
#define GSH_CNAV_QUANTISER_HARD 0 /* (x > 0) * 255: gps_l2c_telemetry_decoder_gs.cc:178, gps_l5_telemetry_decoder_gs.cc:213 */
#define GSH_CNAV_QUANTISER_SOFT 1 /* rint(127.5 + 127.5 * clamp(x / soft_scale, -1, 1)) in float32: the soft input the library accepts */
#define GSH_CNAV_FLAG_PREAMBLE_SEEN 1u /* cnav_v27_part_t, cnav_msg.h:78-86 */
#define GSH_CNAV_FLAG_INVERT 2u
#define GSH_CNAV_FLAG_MESSAGE_LOCK 4u
#define GSH_CNAV_FLAG_CRC_OK 8u
#define GSH_CNAV_FLAG_INIT 16u
    /* the messages n symbols can deliver: the locked decoder releases 32 bits per 64 symbols and holds fewer than 300 between symbols, so two
     * messages can complete within 577 symbols, three within 1 153, and so on, 576 apart at the closest (never below n / 600 + 1) */
#define GSH_CNAV_RESULT_CAPACITY(n) ((n) == 0 ? 1u : ((n) + 575u) / 576u)
    typedef struct gsh_cnav gsh_cnav_t;
    typedef struct
    {
        uint64_t decisions[64];   /* the decision ring: bit n of an entry is new state n's decision (v27_decision_t.w[0] | w[1] << 32) */
        uint32_t old_metrics[64]; /* what v27_t.old_metrics points at: the metrics after the last step */
        uint32_t new_metrics[64]; /* what v27_t.new_metrics points at: those of the step before, which the trace-back ranks */
        uint8_t symbols[128];     /* cnav_v27_part_t.symbols */
        uint32_t decoded[16];     /* cnav_v27_part_t.decoded, MSB first: byte b is bits 31 - 8 * (b % 4) .. of word b / 4 */
        uint32_t decisions_index;
        uint32_t n_symbols;
        uint32_t n_decoded;
        uint32_t flags; /* GSH_CNAV_FLAG_* */
        uint32_t n_crc_fail;
        uint32_t reserved;
    } gsh_cnav_part_state; /* 1240 bytes */
    typedef struct
    {
        gsh_cnav_part_state part[2]; /* part1, part2 of cnav_msg_decoder_t */
    } gsh_cnav_channel_state; /* 2480 bytes */
    typedef struct
    {
        int32_t channel;
        int32_t reserved;
        uint64_t symbol_offset;   /* the channel's new symbols in the call's symbol array */
        uint64_t n_symbols;       /* at most 2^31 */
        uint32_t result_offset;   /* the job's slice of the call's result array */
        uint32_t result_capacity; /* at least GSH_CNAV_RESULT_CAPACITY(n_symbols) */
    } gsh_cnav_job; /* 32 bytes */
    typedef struct
    {
        uint32_t bits[10];     /* the 300 bits, un-inverted, MSB first; the last 20 bits of word 9 are 0 */
        uint32_t symbol_index; /* within the job's span, of the symbol that completed the message */
        uint32_t delay;        /* cnav_msg.c:344: (n_decoded - 300 + 32) * 2 + n_symbols */
        uint32_t tow;          /* bits 20-36 */
        uint8_t prn;           /* bits 8-13 */
        uint8_t msg_id;        /* bits 14-19 */
        uint8_t alert;         /* bit 37 */
        uint8_t part;          /* 1 or 2: which part delivered */
        uint8_t invert;        /* that part's invert flag */
        uint8_t invert_or;     /* part1.invert | part2.invert, from which both blocks set d_flag_PLL_180_deg_phase_locked
                                  (gps_l5_telemetry_decoder_gs.cc:227-234); the idle part's flag can be stale */
        uint8_t reserved[2];
    } gsh_cnav_message; /* 60 bytes */
    /* n_channels decoders, each as after cnav_msg_decoder_init (cnav_msg.c:374-390).  soft_scale > 0 is used by GSH_CNAV_QUANTISER_SOFT only */
    int gsh_cnav_create(int device, int n_channels, int quantiser_mode, float soft_scale, gsh_cnav_t** out);
    void gsh_cnav_destroy(gsh_cnav_t* h);
    /* a fresh cnav_msg_decoder_init for one channel */
    int gsh_cnav_channel_reset(gsh_cnav_t* h, int channel);
    /* the range checks of a job table, on the host alone: GSH_ERR_INVALID for a channel outside 0..n_channels - 1, two jobs of one channel, a
     * symbol span that leaves the n_symbols of the array or exceeds 2^31, a result slice that leaves the n_results of the array or overlaps
     * another job's, a capacity below GSH_CNAV_RESULT_CAPACITY(n_symbols).  The push entry points run it before any launch */
    int gsh_cnav_check_jobs(int n_channels, uint64_t n_symbols, uint32_t n_results, const gsh_cnav_job* jobs, int n_jobs);
    /* cnav_msg_decoder_add_symbol (cnav_msg.c:415-439) for every symbol of every job, symbols as the library takes them (0x00 a certain 0, 0xFF
     * a certain 1).  results: host array of n_results messages, each job writes counts[job] messages from its result_offset; the rest is untouched.
     * A channel whose state was imported (gsh_cnav_channel_set_state) with a message's worth of bits already decoded can deliver more than its
     * capacity: the first result_capacity messages are written, counts[job] holds the number delivered, every channel's state has advanced, and
     * the call returns GSH_ERR_STATE */
    int gsh_cnav_push_u8(gsh_cnav_t* h, const uint8_t* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, gsh_cnav_message* results,
        uint32_t n_results, int32_t* counts);
    /* the same over host floats through the handle's quantiser (gps_l2c_telemetry_decoder_gs.cc:178, gps_l5_telemetry_decoder_gs.cc:213) */
    int gsh_cnav_push_f32(gsh_cnav_t* h, const float* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, gsh_cnav_message* results,
        uint32_t n_results, int32_t* counts);
    /* the same over n_symbols floats resident on the handle's device (borrowed for the call) */
    int gsh_cnav_push_f32_device(gsh_cnav_t* h, const void* device_symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs,
        gsh_cnav_message* results, uint32_t n_results, int32_t* counts);
    /* HIP-event average milliseconds per launch of the job table over uint8 symbols; the channels' states are put back before every launch and
     * at the end, so every repetition does the same work and the handle is left as it was */
    int gsh_cnav_time_push(gsh_cnav_t* h, const uint8_t* symbols, uint64_t n_symbols, const gsh_cnav_job* jobs, int n_jobs, int reps, float* avg_ms);
    /* a channel's whole cnav_msg_decoder_t (cnav_msg.h:67-99): moves a channel between handles or devices without losing lock.  set_state
     * refuses a state whose indices or counts leave their arrays */
    int gsh_cnav_channel_get_state(gsh_cnav_t* h, int channel, gsh_cnav_channel_state* state);
    int gsh_cnav_channel_set_state(gsh_cnav_t* h, int channel, const gsh_cnav_channel_state* state);

#ifdef __cplusplus
}
#endif
#endif /* GNSS_SDR_HIP_H */
