// The batched multicorrelator's E/P/L kernels once more, with work-groups of 128 threads: TWO waves per job (csrc/multicorrelator.hip explains when its launcher
// comes here).  The kernel text is csrc/mcorr_kernels.h, included at this size; mcorr_device.h keeps the two sizes in separate namespaces (mcdev_256 / mcdev_128),
// and the template is named mcorr_kernel_t128<...> so that a profile tells them apart.  Only what mcorr_launch_epl_t128 launches is instantiated: three flavours
// of mcorr_kernel_t128<3, 0, ...> and the walk (tests/test_tracking_kernel_inventory.py).
#define GSH_MC_THREADS 128
#define GSH_MC_VARIANT_128 1
#define mcorr_kernel mcorr_kernel_t128
#include "mcorr_kernels.h"
#include <atomic>
#include <cstdlib>

namespace gsh
{
namespace
{
// Work-groups of mcorr_walk_kernel_t128 the current device holds at once (occupancy x compute units, with the most LDS the half-chip flavour ever asks for):
// asked once per device.  0: the runtime could not say -- no walk.
int walk_capacity()
{
    constexpr int MAX_DEVICES = 64;
    static std::atomic<int> cached[MAX_DEVICES];  // 0: not asked yet; -1: asked, no answer
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return 0;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v == 0)
        {
            const size_t lds_most = mcorr_lds_bytes_half(MC_HALF_MAX_CODE_LEN, MC_WAVES);
            int per_cu = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mcorr_walk_kernel_t128, MC_THREADS, lds_most) != hipSuccess
                || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu <= 0 || cus <= 0)
                {
                    (void)hipGetLastError();
                    v = -1;
                }
            else
                v = per_cu * cus;
            cached[dev].store(v, std::memory_order_relaxed);
        }
    return v > 0 ? v : 0;
}

// Grid of the walk for a launch that would take mcorr_kernel_t128<3, 0, false, false, false, true, true>; 0: that kernel itself, one work-group per job.
// GSH_MC_WALK (read once; A/B runs and tests): 0 never walks; a positive number is the grid, whatever the size of the launch; unset, the grid is one resident
// round of work-groups once the launch holds at least two of them (below that a chip that is not full wants one work-group per job).
int walk_grid(const McorrArgs& a)
{
    static const int forced = [] {
        const char* e = std::getenv("GSH_MC_WALK");
        return (e != nullptr && e[0] != '\0') ? std::atoi(e) : -1;
    }();
    if (forced == 0 || a.splits != 1 || a.n_launch <= 0) return 0;
    if (forced > 0) return forced;
    const int g = walk_capacity();
    return (g > 0 && static_cast<long long>(a.n_launch) >= 2LL * g) ? g : 0;
}

std::atomic<unsigned long long> walk_launches{0};  // launches of this process that took the walk (gsh_mcorr_walk_launches)
}  // namespace

int mcorr_launch_epl_t128(const McorrArgs& a, size_t lds, size_t lds_half, hipStream_t stream)
{
    const dim3 grid(static_cast<unsigned>(a.n_launch) * static_cast<unsigned>(a.splits));
    const dim3 block(MC_THREADS);
    if (a.pair && a.packed == 1)
        {
            if (a.half && lds_half > 0 && a.code_images != nullptr)
                {
                    const int walk = walk_grid(a);
                    if (walk > 0)
                        {
                            hipLaunchKernelGGL(mcorr_walk_kernel_t128, dim3(static_cast<unsigned>(walk)), block, lds_half, stream, a);
                            walk_launches.fetch_add(1, std::memory_order_relaxed);
                        }
                    else
                        hipLaunchKernelGGL((mcorr_kernel_t128<3, 0, false, false, false, true, true>), grid, block, lds_half, stream, a);
                }
            else
                hipLaunchKernelGGL((mcorr_kernel_t128<3, 0, false, false, false, true>), grid, block, lds, stream, a);
        }
    else
        hipLaunchKernelGGL((mcorr_kernel_t128<3, 0, false>), grid, block, lds, stream, a);
    GSH_HIP(hipGetLastError());
    return GSH_OK;
}
}  // namespace gsh

extern "C"
{
    int gsh_mcorr_walk_capacity(void) { return gsh::walk_capacity(); }
    uint64_t gsh_mcorr_walk_launches(void) { return gsh::walk_launches.load(std::memory_order_relaxed); }
}
