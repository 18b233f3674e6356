// The ION_GSMS layout object (gsh_ion_layout_t) and its device unpack, for the other translation units of the library (the ring pushes of
// sample_stream.hip).  The decoder and the descriptor's rules are in ion_gsms.h.
#ifndef GSH_ION_LAYOUT_H
#define GSH_ION_LAYOUT_H
#include "gsh_internal.h"
#include "ion_gsms.h"

struct gsh_ion_layout
{
    gsh::IonLayout l;
};

namespace gsh
{
// the streams of one call: 1 .. GSH_ION_MAX_SELECTED of them, each described, none named twice, equal samples per cycle, all complex or all real
// (*cplx, *rate: what they share); GSH_ERR_INVALID otherwise
int ion_check_streams(const gsh_ion_layout* layout, const int32_t* streams, int n_streams, int* cplx, int* rate);
// samples [first, first + n) of each selected stream of the block at d_src (cycle 0 at its first byte, aligned to the layout's largest word) ->
// d_dst[i]: complex64 (conjugated when conj) or float32; the caller has validated the selection (ion_check_streams) and the pointers
int ion_unpack(const gsh_ion_layout* layout, const void* d_src, unsigned long long first, unsigned long long n, int conj, const int32_t* streams,
    int n_streams, void* const* d_dst, hipStream_t s);
}  // namespace gsh
#endif
