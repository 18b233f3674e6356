// Host build of gnss-sdr_amd/csrc/cnav_stream.h for tests/test_cnav_stream_host.py: one channel walked on one thread with the functions as they
// are, the way cnav_stream_kernel walks it with 64 lanes.  The channel state belongs to the caller, as it belongs to the handle in the library.
#include "cnav_stream.h"
#include "gnss_sdr_hip.h"

extern "C"
{
    int gsh_test_cnav_sizes(int* job_bytes, int* message_bytes, int* state_bytes)
    {
        *job_bytes = static_cast<int>(sizeof(gsh_cnav_job));
        *message_bytes = static_cast<int>(sizeof(gsh_cnav_message));
        *state_bytes = static_cast<int>(sizeof(gsh_cnav_channel_state));
        return gsh::CNAV_STATES;
    }

    void gsh_test_cnav_init(gsh_cnav_channel_state* state) { gsh::cnav_channel_init(*state); }

    int gsh_test_cnav_state_valid(const gsh_cnav_channel_state* state) { return gsh::cnav_state_valid(*state) ? 1 : 0; }

    // the messages delivered; only the first `capacity` are written
    uint32_t gsh_test_cnav_push(gsh_cnav_channel_state* state, const uint8_t* symbols, uint32_t n, gsh_cnav_message* out, uint32_t capacity)
    {
        return gsh::cnav_channel_push(*state, symbols, n, out, capacity);
    }

    void gsh_test_cnav_quantise(const float* x, uint32_t n, int mode, float scale, uint8_t* out)
    {
        for (uint32_t i = 0; i < n; i++) out[i] = static_cast<uint8_t>(gsh::cnav_quantise(x[i], mode, scale));
    }

    uint32_t gsh_test_cnav_acs(uint32_t n, uint32_t old_lo, uint32_t old_hi, uint32_t sym0, uint32_t sym1, uint32_t* decision)
    {
        return gsh::cnav_acs(n, old_lo, old_hi, sym0, sym1, *decision);
    }
}
