// GPU test of Hip_Sample_Ring::push_packed (gnss-sdr_amd/host/hip_correlator_runtime.{h,cc}) and of the group push of packed samples beneath it.
// One complex family, Two_Bit_Cpx_File_Signal_Source (two_bit_cpx_file_signal_source.cc:72-81: unpack_byte_2bit_cpx_samples, then
// interleaved_short_to_complex(false, true)), pushed in ragged whole-byte blocks that wrap a ring of odd capacity:
//   * a plain ring: every resident sample equals a ring fed the host-unpacked int16 pairs through push_ishort;
//   * a group of one forced through RCCL (GSH_GROUP_FORCE_RCCL, the block crosses ncclSend / ncclRecv / ncclAllGather as packed bytes): the same;
//   * with GSH_RCCL_LIBRARY naming the test stand-in (tests/host/libfake_rccl.so): Hip_Sample_Ring over three ranks on one device (its group branch).
// Prints "PACKED RING OK".  Built by __graft_entry__.build(); run by tests/test_packed_ingest_gpu.py.
#include "hip_correlator_runtime.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>

namespace
{
int fails = 0;
#define EXPECT(cond, ...)                                        \
    do                                                           \
        {                                                        \
            if (!(cond))                                         \
                {                                                \
                    if (fails++ < 20)                            \
                        {                                        \
                            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                            std::printf(__VA_ARGS__);            \
                            std::printf("\n");                   \
                        }                                        \
                }                                                \
        }                                                        \
    while (0)

// the reference chain on the host: unpack_byte_2bit_cpx_samples.cc:77-89 (bits 5:4, 7:6, 1:0, 3:2 as 2 s + 1), then the I/Q swap of
// interleaved_short_to_complex(false, true) -- as int16 pairs for push_ishort
int s2(int v) { return (v & 1) - (v & 2); }
std::vector<int16_t> host_unpack(const std::vector<uint8_t>& b)
{
    std::vector<int16_t> iq;
    for (uint8_t c : b)
        {
            const int16_t u[4] = {int16_t(2 * s2(c >> 4) + 1), int16_t(2 * s2(c >> 6) + 1), int16_t(2 * s2(c) + 1), int16_t(2 * s2(c >> 2) + 1)};
            iq.insert(iq.end(), {u[1], u[0], u[3], u[2]});
        }
    return iq;
}

bool same_ring(gsh_stream_t* a, gsh_stream_t* b, uint32_t win, const char* what)
{
    uint64_t lo = 0, hi = 0, lo2 = 0, hi2 = 0;
    gsh_stream_range(a, &lo, &hi);
    gsh_stream_range(b, &lo2, &hi2);
    EXPECT(lo == lo2 && hi == hi2, "%s: ranges [%llu, %llu) vs [%llu, %llu)", what, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)lo2,
        (unsigned long long)hi2);
    const uint64_t n = std::min<uint64_t>(hi - lo, win);
    std::vector<float> x(2 * n), y(2 * n);
    for (uint64_t start : {lo, hi - n})
        {
            EXPECT(gsh_stream_read(a, start, n, x.data()) == GSH_OK && gsh_stream_read(b, start, n, y.data()) == GSH_OK, "%s: read: %s", what, gsh_last_error());
            EXPECT(std::memcmp(x.data(), y.data(), x.size() * sizeof(float)) == 0, "%s: ring contents differ at window %llu", what, (unsigned long long)start);
        }
    return fails == 0;
}
}  // namespace

int main()
{
    const uint64_t cap = 40001;  // not a multiple of 4: the wrap falls inside a packed byte
    const uint32_t win = 9000;
    gsh_packed_format fmt{};
    fmt.family = GSH_PACKED_TWO_BIT_CPX;
    fmt.sample_type = GSH_PACKED_IQ;
    fmt.item_size = 1;
    std::mt19937 rng(7);
    std::vector<std::vector<uint8_t>> blocks;
    for (uint64_t bytes : {4500u, 1u, 4095u, 10000u, 0u, 389u, 16666u, 2048u})
        {
            std::vector<uint8_t> b(bytes);
            for (auto& v : b) v = static_cast<uint8_t>(rng());
            blocks.push_back(b);
        }

    Hip_Sample_Ring plain(0, cap, win), ref(0, cap, win);
    EXPECT(plain.ok() && ref.ok(), "ring: %s", plain.last_error().c_str());
    gsh_stream_group_t* g = nullptr;
    const int dev = 0;
    EXPECT(gsh_stream_group_create(&dev, 1, cap, win, GSH_GROUP_SCATTER_ALLGATHER | GSH_GROUP_FORCE_RCCL, &g) == GSH_OK, "group: %s", gsh_last_error());
    const char* stub = std::getenv("GSH_RCCL_LIBRARY");
    Hip_Sample_Ring* multi = nullptr;
    if (stub != nullptr && *stub != '\0')
        {
            multi = new Hip_Sample_Ring(std::vector<int>{0, 0, 0}, cap, win);
            EXPECT(multi->ok(), "three-rank ring: %s", multi->last_error().c_str());
        }
    if (fails) return 1;
    uint64_t total = 0;
    for (const auto& b : blocks)
        {
            const uint64_t n = 2 * b.size();
            const std::vector<int16_t> iq = host_unpack(b);
            const uint64_t f0 = plain.push_packed(fmt, b.data(), n);
            const uint64_t f1 = ref.push_ishort(iq.data(), n);
            uint64_t f2 = 0;
            EXPECT(gsh_stream_group_push_packed(g, &fmt, b.data(), n, 0, &f2) == GSH_OK && gsh_stream_group_wait(g) == GSH_OK, "group push: %s", gsh_last_error());
            EXPECT(f0 == total && f1 == total && f2 == total, "first index %llu / %llu / %llu, expected %llu", (unsigned long long)f0, (unsigned long long)f1,
                (unsigned long long)f2, (unsigned long long)total);
            if (multi != nullptr) EXPECT(multi->push_packed(fmt, b.data(), n) == total, "three-rank push: %s", multi->last_error().c_str());
            total += n;
            same_ring(plain.handle(), ref.handle(), win, "plain ring vs push_ishort");
            same_ring(gsh_stream_group_ring(g, 0), ref.handle(), win, "RCCL group of one vs push_ishort");
            if (multi != nullptr) same_ring(multi->handle_for(0), ref.handle(), win, "three-rank ring (rank 0) vs push_ishort");
            if (fails) break;
        }
    // a partial item is refused and leaves the ring as it was
    uint8_t one = 0x5a;
    EXPECT(plain.push_packed(fmt, &one, 1) == UINT64_MAX, "a partial item was accepted");
    EXPECT(plain.next_index() == total, "a refused push moved the ring");
    int32_t ranks = 0;
    uint64_t calls = 0;
    gsh_stream_group_rccl_info(g, &ranks, nullptr, &calls);
    EXPECT(ranks == 1 && calls == 3 * 7, "RCCL group of one: %d ranks, %llu calls (expected 1, 21)", ranks, (unsigned long long)calls);
    gsh_stream_group_destroy(g);
    delete multi;
    if (fails)
        {
            std::printf("PACKED RING FAILED (%d)\n", fails);
            return 1;
        }
    std::printf("PACKED RING OK: %llu samples of Two_Bit_Cpx in %zu blocks, plain ring + RCCL group of one%s equal push_ishort of the host-unpacked pairs\n",
        (unsigned long long)total, blocks.size(), multi ? " + three stub ranks" : "");
    return 0;
}
