// The index arithmetic of the direct resampler (direct_resampler_conditioner_cc.cc:52-59,83-110; see resampler.hip), host side: shared by
// gsh_direct_resample_device and the signal conditioner's bookkeeping (conditioner.hip), so that both number the stream's outputs alike.
#ifndef GSH_RESAMPLE_INDEX_H
#define GSH_RESAMPLE_INDEX_H
#include <cmath>

namespace gsh
{
// phase step exactly as the reference computes it (:52-59); 0 stands for a ratio of one (2^32 does not fit the uint32 cast)
inline unsigned phase_step_of(double fs_in, double fs_out, int* decimating)
{
    const double two_32 = 4294967296.0;
    *decimating = fs_in >= fs_out ? 1 : 0;
    const double v = *decimating ? std::floor(two_32 * fs_out / fs_in) : std::floor(two_32 * fs_in / fs_out);
    if (v >= two_32) return 0u;
    return static_cast<unsigned>(v);
}

// absolute input index feeding absolute output j
inline unsigned long long input_index_of(unsigned long long j, unsigned step, int decimating)
{
    if (step == 0) return j;
    if (decimating) return static_cast<unsigned long long>(((static_cast<unsigned __int128>(j) << 32) + step - 1) / step);
    return static_cast<unsigned long long>((static_cast<unsigned __int128>(j + 1) * step) >> 32);
}
}  // namespace gsh
#endif
