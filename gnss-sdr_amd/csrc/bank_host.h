// Host-side steps the correlator banks share (tracking_api.hip, the host half of multicorrelator_16sc.hip).  No device code; not part of the ABI.
#ifndef GSH_BANK_HOST_H
#define GSH_BANK_HOST_H
#include "gsh_internal.h"
#include <initializer_list>

#define GSH_TRY(expr)                          \
    do                                         \
        {                                      \
            const int rc__ = (expr);           \
            if (rc__ != GSH_OK) return rc__;   \
        }                                      \
    while (0)

namespace gsh
{
// A growable buffer of T in device (PINNED false) or page-locked host memory: a pointer and its capacity in elements.  grow() keeps no contents.  No
// destructor: a handle releases its buffers in its destroy, after hipSetDevice.
template <typename T, bool PINNED>
struct Buf
{
    T* p{nullptr};
    size_t cap{0};

    int release()
    {
        T* old = p;
        p = nullptr;
        cap = 0;
        if (old != nullptr) GSH_HIP(PINNED ? hipHostFree(old) : hipFree(old));
        return GSH_OK;
    }
    int grow(size_t need)
    {
        if (need <= cap) return GSH_OK;
        GSH_TRY(release());
        if (PINNED)
            GSH_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * need, hipHostMallocDefault));
        else
            GSH_HIP(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * need));
        cap = need;
        return GSH_OK;
    }
};
template <typename T>
using DeviceBuf = Buf<T, false>;
template <typename T>
using PinnedBuf = Buf<T, true>;

// release every buffer, in the order given; the first failure is the answer.  Buffers that grow as one block are all released before the first of them is
// allocated again; a destroy walks its members with it.
template <typename... B>
int release_all(B&... bufs)
{
    int rc = GSH_OK;
    for (const int r : {bufs.release()...})
        if (rc == GSH_OK) rc = r;
    return rc;
}

// May a staged batch run on the attached flat stream?  max_end is the largest window end of the batch; sample_base shifts every window.
inline int batch_fits_stream(const void* d_stream, unsigned long long max_end, unsigned long long sample_base, unsigned long long stream_len)
{
    if (d_stream == nullptr) return set_error(GSH_ERR_STATE, "no sample stream attached (gsh_bank_set_stream_*)");
    if (max_end + sample_base > stream_len)
        return set_error(GSH_ERR_INVALID, "a job window ends at sample %llu (sample_base %llu), past the %llu-sample stream", max_end + sample_base, sample_base, stream_len);
    return GSH_OK;
}

// The event-timed loop: `reps` calls of launch() between ev0 and ev1 on st; *avg_ms is the elapsed time per call.  The caller has checked its arguments and
// warmed up; a failing launch() ends the loop with its status.
template <typename Launch>
int time_launches(hipEvent_t ev0, hipEvent_t ev1, hipStream_t st, int reps, float* avg_ms, Launch launch)
{
    GSH_HIP(hipEventRecord(ev0, st));
    for (int i = 0; i < reps; i++) GSH_TRY(launch());
    GSH_HIP(hipEventRecord(ev1, st));
    GSH_HIP(hipEventSynchronize(ev1));
    float ms = 0.0f;
    GSH_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    *avg_ms = ms / static_cast<float>(reps);
    return GSH_OK;
}
}  // namespace gsh

#endif
