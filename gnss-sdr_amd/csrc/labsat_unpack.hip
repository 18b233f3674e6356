// LabSat 2 / 3, LabSat 3 Wideband and SPIR 1-bit captures -> complex64 (ring positions): the device half of the reference's Labsat_Signal_Source and
// Spir_File_Signal_Source for the register families of packed_registers.h (the decoder, the layout and the reference lines are there).
// Store-bound: a sample costs 4 bytes in at the most (SPIR), 0.53 .. 2 for the LabSat families, and 8 out per RF channel.  So lanes map to OUTPUT samples:
// a lane decodes two adjacent samples and writes them with one 16-byte store (two 8-byte stores where the destination is not 16-byte aligned), a wave
// writes one contiguous run of 1 KiB of ONE destination per store instruction, and the 2 .. 32 lanes whose samples lie in one register load the same
// 8 bytes.  One pass over the registers of a LabSat 3 Wideband block writes up to 3 RF channels, each to a destination of its own, out of that one load.
// A block may start and end inside a register (a ring split at its capacity boundary does): every sample, whole register or not, goes through
// register_decode.  The host splits `first` into a register and an offset inside it and cuts the block into launches of fewer than REG_DIV_LIMIT
// samples, so a lane divides by spr (3, 5, 7, 10, 15, 30 ...) with one 32-bit multiply (register_div) and never in 64 bits.
// LabSat 4 -- rounds of one buffer per channel, 24-bit samples across registers -- has a kernel of its own below, unpack_ls4_kernel, of the same shape.
#include "packed_unpack.h"

namespace gsh
{
namespace
{
constexpr int RG_THREADS = 256;
constexpr int RG_MAX = 3;  // RF channels of a LabSat 3 Wideband register
struct RegisterArgs
{
    const void* src;    // register 0 of the launch: the one that holds its first sample; aligned to the register size
    unsigned off, n;    // the first sample's number inside that register (< spr); samples to write: off + n < REG_DIV_LIMIT
    float qsign;
    int n_sel;
    int ch[RG_MAX];
    float2* dst[RG_MAX];  // dst[i][0] is the launch's first sample of channel ch[i]
};

// REG: the register as it lies in memory (unsigned short, unsigned, unsigned long long)
template <typename REG>
__global__ __launch_bounds__(RG_THREADS) void unpack_register_kernel(RegisterArgs a, PackedCode c)
{
    const unsigned j = 2u * (blockIdx.x * RG_THREADS + threadIdx.x);  // the lane's outputs j, j + 1
    if (j >= a.n) return;
    const bool two = j + 1u < a.n;
    const unsigned spr = static_cast<unsigned>(c.spr);
    const unsigned t = a.off + j;
    const unsigned r0 = register_div(t, c.spr_magic);
    const unsigned i0 = t - r0 * spr;
    const bool wrap = i0 + 1u == spr;  // the second sample opens the next register
    const unsigned i1 = wrap ? 0u : i0 + 1u;
    const REG* src = static_cast<const REG*>(a.src);
    const unsigned long long w0 = src[r0];
    const unsigned long long w1 = (two && wrap) ? static_cast<unsigned long long>(src[r0 + 1u]) : w0;  // (never a register behind the block's last sample)
#pragma unroll
    for (int i = 0; i < RG_MAX; i++)
        if (i < a.n_sel)
            {
                const float2 x0 = register_decode(c, w0, static_cast<int>(i0), a.ch[i]);
                float2* d = a.dst[i] + j;
                if (!two)
                    {
                        d[0] = make_float2(x0.x, a.qsign * x0.y);
                        continue;
                    }
                const float2 x1 = register_decode(c, w1, static_cast<int>(i1), a.ch[i]);
                if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                    *reinterpret_cast<float4*>(d) = make_float4(x0.x, a.qsign * x0.y, x1.x, a.qsign * x1.y);
                else
                    {
                        d[0] = make_float2(x0.x, a.qsign * x0.y);
                        d[1] = make_float2(x1.x, a.qsign * x1.y);
                    }
            }
}
// LabSat 4 (packed_registers.h): the same shape of kernel over ROUNDS, S the samples of a selected slot per round.  Two ways to a lane's round:
//   small rounds (by_round 0): output sample t of the launch, counted from the start of the launch's first round, lies in round t / S at j = t % S --
//     one 32-bit multiply (register_div; the launcher keeps t S below 2^32, where it is exact);
//   large rounds (by_round 1): blockIdx.y is the round and the lanes of the x dimension walk its S samples: no division, and one launch takes up to
//     65 535 whole rounds.  (S is even, so a lane's pair never leaves the round.)
// From j the way is shifts: register 2 QUA j / 64 of the slot's buffer at bit 2 QUA j % 64.  The lane's two samples are 4 QUA adjacent bits of the slot's
// bit stream, one field in one register or across two (ls4_field64): one load, at most two, per slot.  The selected slots of one call hold the same
// number of registers per round, so the lane's position is the same in each and only the buffer's place in the round differs.
struct Ls4Args
{
    const unsigned long long* src;  // register 0 of the round that holds the launch's first sample
    unsigned off, n;                // by_round 0: the first sample's number inside that round (< S); samples to write
    unsigned s, s_magic;            // S and register_div_magic(S); magic 0: off + n <= S, the launch stays inside one round
    unsigned round, bits;           // registers per round; 2 QUA
    int qua, by_round;
    float scale, qsign;
    int n_sel;
    unsigned base[RG_MAX];          // where the buffer of selected slot i starts in the round (registers)
    float2* dst[RG_MAX];            // dst[i][0] is the launch's first sample of that slot
};

// 2 * bits (<= 48) adjacent bits that start `o` below the top of lo and may run on into the top of hi
__device__ __forceinline__ unsigned long long ls4_field64(unsigned long long lo, unsigned long long hi, unsigned o, unsigned nbits)
{
    const unsigned end = o + nbits;
    const unsigned long long v = end <= 64u ? lo >> (64u - end) : (lo << (end - 64u)) | (hi >> (128u - end));
    return v & ((1ull << nbits) - 1ull);
}

__global__ __launch_bounds__(RG_THREADS) void unpack_ls4_kernel(Ls4Args a)
{
    const unsigned j = 2u * (blockIdx.x * RG_THREADS + threadIdx.x);  // the lane's outputs j, j + 1 (by_round: of its round)
    unsigned round0, j0;
    unsigned long long out;  // the first of them in dst
    bool two;
    if (a.by_round)
        {
            if (j >= a.s) return;
            round0 = blockIdx.y;
            j0 = j;
            two = true;  // (S is even)
            out = static_cast<unsigned long long>(round0) * a.s + j;
        }
    else
        {
            if (j >= a.n) return;
            two = j + 1u < a.n;
            const unsigned t = a.off + j;
            round0 = a.s_magic ? register_div(t, a.s_magic) : 0u;
            j0 = t - round0 * a.s;
            out = j;
        }
    const bool pair = two && j0 + 1u < a.s;  // both samples in this round: one field of 4 QUA bits
    const unsigned b0 = j0 * a.bits, o0 = b0 & 63u;
    const unsigned long long r0 = static_cast<unsigned long long>(round0) * a.round + (b0 >> 6);
    // a second register only where the lane's bits run into it: it holds bits of a sample the lane writes, so it is never one behind the block's last
    // sample (and inside the buffer: at QUA 12 regs is a multiple of 3, a triple ends with a sample)
    const bool more = o0 + (pair ? 2u * a.bits : a.bits) > 64u;
#pragma unroll
    for (int i = 0; i < RG_MAX; i++)
        if (i < a.n_sel)
            {
                const unsigned long long* p = a.src + a.base[i];
                const unsigned long long lo = p[r0];
                const unsigned long long hi = more ? p[r0 + 1ull] : 0ull;
                float2* d = a.dst[i] + out;
                if (pair)
                    {
                        const unsigned long long v = ls4_field64(lo, hi, o0, 2u * a.bits);
                        const float2 x0 = ls4_value(static_cast<unsigned>(v >> a.bits), a.qua, a.scale);
                        const float2 x1 = ls4_value(static_cast<unsigned>(v) & ((1u << a.bits) - 1u), a.qua, a.scale);
                        if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0)
                            *reinterpret_cast<float4*>(d) = make_float4(x0.x, a.qsign * x0.y, x1.x, a.qsign * x1.y);
                        else
                            {
                                d[0] = make_float2(x0.x, a.qsign * x0.y);
                                d[1] = make_float2(x1.x, a.qsign * x1.y);
                            }
                        continue;
                    }
                const float2 x0 = ls4_value(ls4_field(lo, hi, o0, a.bits), a.qua, a.scale);
                d[0] = make_float2(x0.x, a.qsign * x0.y);
                if (two)  // the second sample opens the next round: the top of its first register
                    {
                        const unsigned long long w = p[static_cast<unsigned long long>(round0 + 1u) * a.round];
                        const float2 x1 = ls4_value(ls4_field(w, 0ull, 0u, a.bits), a.qua, a.scale);
                        d[1] = make_float2(x1.x, a.qsign * x1.y);
                    }
            }
}

constexpr int LS4_MAX_REGS = 1 << 20;        // registers of one slot per round (BUF_SIZE of 8 MiB): keeps 2 QUA j of a round in 32 bits
constexpr unsigned LS4_DIVIDE_BELOW = 1024;   // S up to here: lanes divide by S (a launch takes 2^32 / S >= 4 Mi samples); above: a grid row per round

int ls4_code(const gsh_packed_format* f, PackedCode* out)
{
    static const int quas[5] = {1, 2, 4, 8, 12};
    const int qua = quas[f->family - GSH_PACKED_LS4_1BIT];
    const int regs[3] = {f->big_endian_bytes, f->big_endian_items, f->reserved};  // (the fields every other register family keeps 0)
    GSH_REQUIRE(f->item_size == 8, "item_size %d: the LabSat 4 families read 8-byte little-endian registers (item_size 8)", f->item_size);
    GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ, "sample_type %d: LabSat 4 samples are complex, sample_type must be GSH_PACKED_IQ", f->sample_type);
    GSH_REQUIRE(f->rf_channels >= 1 && f->rf_channels <= 3, "rf_channels %d: a LabSat 4 layout describes 1..3 channel slots (A, B, C)", f->rf_channels);
    PackedCode c{};
    c.family = f->family;
    c.cplx = 1;
    c.item_bytes = 1;
    c.rbytes = 8;
    c.ls4 = 1;
    c.qua = qua;
    c.frame_bits = 2 * qua;
    c.nch = f->rf_channels;
    c.spr = qua == 12 ? 8 : 32 / qua;
    c.spr_magic = register_div_magic(c.spr);
    c.ls4_scale = 1.0f / static_cast<float>(1 << (qua - 1));
    for (int s = 0; s < 3; s++)
        {
            GSH_REQUIRE(regs[s] >= 0 && regs[s] <= LS4_MAX_REGS, "register count %d of slot %c outside 0..%d (BUF_SIZE_%c / 8 of the LabSat 4 recording)", regs[s],
                'A' + s, LS4_MAX_REGS, 'A' + s);
            GSH_REQUIRE(s < f->rf_channels || regs[s] == 0, "register count %d of slot %c, but rf_channels %d describes no such slot", regs[s], 'A' + s,
                f->rf_channels);
            GSH_REQUIRE(qua != 12 || regs[s] % 3 == 0, "QUA 12 with %d registers in slot %c: not a multiple of 3, a 24-bit sample would run past the buffer",
                regs[s], 'A' + s);
            c.ls4_off[s] = c.ls4_round;
            c.ls4_regs[s] = static_cast<unsigned>(regs[s]);
            c.ls4_round += static_cast<unsigned>(regs[s]);
        }
    GSH_REQUIRE(f->channel >= 0 && f->channel < f->rf_channels, "channel %d outside 0..%d (selected_channel - 1 of %d channel slots)", f->channel,
        f->rf_channels - 1, f->rf_channels);
    GSH_REQUIRE(regs[f->channel] > 0, "channel %d (slot %c) is not recorded: its register count is 0", f->channel, 'A' + f->channel);
    c.channel = f->channel;
    c.ls4_base = c.ls4_off[f->channel];
    c.ls4_s = c.ls4_regs[f->channel] * 32u / static_cast<unsigned>(qua);  // (QUA 12: regs / 3 triples of 8)
    *out = c;
    return GSH_OK;
}

int unpack_ls4(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s)
{
    int rc = ls4_check_channels(c, channels, n_sel);
    if (rc != GSH_OK) return rc;
    const unsigned long long S = static_cast<unsigned long long>(c.ls4_regs[channels[0]]) * 32ull / static_cast<unsigned long long>(c.qua);
    Ls4Args a{};
    a.s = static_cast<unsigned>(S);
    a.round = c.ls4_round;
    a.bits = static_cast<unsigned>(c.frame_bits);
    a.qua = c.qua;
    a.scale = c.ls4_scale;
    a.qsign = conj ? -1.0f : 1.0f;
    a.n_sel = n_sel;
    for (int i = 0; i < n_sel; i++) a.base[i] = c.ls4_off[channels[i]];
    // samples [at, at + len) by division: len is such that (off + len) S < 2^32, where register_div by S is exact (its e <= S), and below REG_DIV_LIMIT
    auto divided = [&](unsigned long long done, unsigned long long len, bool one_round) {
        const unsigned long long at = first + done, round = at / S;
        a.by_round = 0;
        a.s_magic = one_round ? 0u : register_div_magic(static_cast<int>(S));
        a.src = static_cast<const unsigned long long*>(d_src) + round * c.ls4_round;
        a.off = static_cast<unsigned>(at - round * S);
        a.n = static_cast<unsigned>(len);
        for (int i = 0; i < n_sel; i++) a.dst[i] = d_dst[i] + done;
        const unsigned blocks = static_cast<unsigned>((len + 2ull * RG_THREADS - 1ull) / (2ull * RG_THREADS));
        unpack_ls4_kernel<<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a);
        return hipGetLastError();
    };
    if (S <= LS4_DIVIDE_BELOW)
        {
            // whole rounds a launch (S is even: the pairing into 16-byte stores carries over)
            const unsigned long long bound = std::min<unsigned long long>(REG_DIV_LIMIT, (1ull << 32) / S);
            const unsigned long long chunk = ((bound - 1ull) / S - 1ull) * S;
            for (unsigned long long done = 0; done < n; done += chunk) GSH_HIP(divided(done, std::min(n - done, chunk), false));
            return GSH_OK;
        }
    // large rounds: what lies in front of the first round boundary and behind the last one as launches of their own (less than a round each: no
    // division), the whole rounds between them a grid row each
    const unsigned long long head = std::min(n, (S - first % S) % S), rounds = (n - head) / S, tail = n - head - rounds * S;
    if (head) GSH_HIP(divided(0, head, true));
    for (unsigned long long r = 0; r < rounds; r += 65535ull)
        {
            const unsigned long long rows = std::min(rounds - r, 65535ull), done = head + r * S;
            a.by_round = 1;
            a.src = static_cast<const unsigned long long*>(d_src) + (first + done) / S * c.ls4_round;
            a.off = 0;
            a.n = 0;
            for (int i = 0; i < n_sel; i++) a.dst[i] = d_dst[i] + done;
            const unsigned blocks = static_cast<unsigned>((S + 2ull * RG_THREADS - 1ull) / (2ull * RG_THREADS));
            unpack_ls4_kernel<<<dim3(blocks, static_cast<unsigned>(rows)), dim3(RG_THREADS), 0, s>>>(a);
            GSH_HIP(hipGetLastError());
        }
    if (tail) GSH_HIP(divided(head + rounds * S, tail, true));
    return GSH_OK;
}
}  // namespace

int ls4_check_channels(const PackedCode& c, const int* channels, int n_sel)
{
    if (!c.ls4) return GSH_OK;
    for (int i = 0; i < n_sel; i++)
        {
            GSH_REQUIRE(channels[i] >= 0 && channels[i] < c.nch, "band %d outside 0..%d", channels[i], c.nch - 1);
            GSH_REQUIRE(c.ls4_regs[channels[i]] > 0, "channel %d (slot %c) is not recorded: its register count is 0", channels[i], 'A' + channels[i]);
            GSH_REQUIRE(c.ls4_regs[channels[i]] == c.ls4_regs[channels[0]],
                "channels %d and %d hold %u and %u registers per round: the channels of one call must have the same bandwidth (select them in separate calls)",
                channels[0], channels[i], c.ls4_regs[channels[0]], c.ls4_regs[channels[i]]);
        }
    return GSH_OK;
}

int register_code(const gsh_packed_format* f, PackedCode* out)
{
    if (packed_ls4(f->family)) return ls4_code(f, out);
    const bool ls3w = packed_ls3w(f->family);
    const char* name = ls3w ? "LabSat 3 Wideband" : f->family == GSH_PACKED_SPIR_1BIT ? "SPIR" : "LabSat 2 / 3";
    const int item = ls3w ? 8 : f->family == GSH_PACKED_SPIR_1BIT ? 4 : 2;
    if (ls3w)
        GSH_REQUIRE((f->reserved & ~1) == 0, "reserved %d: bit 0 (digital I/O recorded) is the only flag of the LabSat 3 Wideband families", f->reserved);
    else
        GSH_REQUIRE(f->reserved == 0, "gsh_packed_format.reserved must be 0");
    GSH_REQUIRE(f->item_size == item, "item_size %d: the %s families read %d-byte little-endian %s (item_size %d)", f->item_size, name, item,
        ls3w ? "registers" : "items", item);
    GSH_REQUIRE(f->sample_type == GSH_PACKED_IQ, "sample_type %d: %s samples are complex, sample_type must be GSH_PACKED_IQ", f->sample_type, name);
    GSH_REQUIRE(f->big_endian_bytes == 0 && f->big_endian_items == 0, "big_endian_bytes %d / big_endian_items %d: the %s families are little-endian, both must be 0",
        f->big_endian_bytes, f->big_endian_items, name);
    PackedCode c{};
    c.family = f->family;
    c.cplx = 1;
    c.item_bytes = 1;
    c.nch = 1;
    c.rbytes = item;
    if (ls3w)
        {
            GSH_REQUIRE(f->rf_channels >= 1 && f->rf_channels <= 3, "rf_channels %d: a LabSat 3 Wideband recording has CHN = 1..3 RF channels", f->rf_channels);
            GSH_REQUIRE(f->channel >= 0 && f->channel < f->rf_channels, "channel %d outside 0..%d (selected_channel - 1 of %d RF channels)", f->channel,
                f->rf_channels - 1, f->rf_channels);
            c.qua = f->family - GSH_PACKED_LS3W_1BIT + 1;
            c.nch = f->rf_channels;
            c.channel = f->channel;
            c.frame_bits = 2 * c.qua * c.nch;
            c.spr = ls3w_samples_per_register(c.qua, c.nch, f->reserved & 1);
            c.spare = 64 - c.spr * c.frame_bits;
        }
    else
        {
            GSH_REQUIRE((f->rf_channels == 0 || f->rf_channels == 1) && f->channel == 0, "rf_channels %d / channel %d: the %s families carry one RF channel",
                f->rf_channels, f->channel, name);
            c.spr = f->family == GSH_PACKED_LABSAT_2BIT ? 8 : f->family == GSH_PACKED_LABSAT_4BIT ? 4 : 1;
            c.qua = f->family == GSH_PACKED_LABSAT_4BIT ? 2 : 1;
            c.frame_bits = 2 * c.qua;
        }
    c.spr_magic = register_div_magic(c.spr);
    *out = c;
    return GSH_OK;
}

int unpack_registers(const void* d_src, const PackedCode& c, unsigned long long first, unsigned long long n, int conj, const int* channels, int n_sel,
    float2* const* d_dst, hipStream_t s)
{
    if (n == 0) return GSH_OK;
    GSH_REQUIRE(c.rbytes != 0 && n_sel >= 1 && n_sel <= RG_MAX && n_sel <= c.nch, "%d bands of packed family %d", n_sel, c.family);
    GSH_REQUIRE((reinterpret_cast<uintptr_t>(d_src) & static_cast<uintptr_t>(c.rbytes - 1)) == 0, "packed %d-bit %s must be %d-byte aligned", 8 * c.rbytes,
        c.rbytes == 8 ? "registers" : "items", c.rbytes);
    if (c.ls4) return unpack_ls4(d_src, c, first, n, conj, channels, n_sel, d_dst, s);
    const unsigned long long spr = static_cast<unsigned long long>(c.spr);
    // launches of whole registers' worth of samples, an even count (the pairing of a destination's samples into 16-byte stores carries over), below the
    // bound of the lanes' 32-bit division
    const unsigned long long chunk = (static_cast<unsigned long long>(REG_DIV_LIMIT) / 2ull - 64ull) / (2ull * spr) * (2ull * spr);
    for (unsigned long long done = 0; done < n; done += chunk)
        {
            const unsigned long long at = first + done, len = n - done < chunk ? n - done : chunk;
            const unsigned long long r = at / spr;
            RegisterArgs a{};
            a.src = static_cast<const unsigned char*>(d_src) + r * static_cast<unsigned long long>(c.rbytes);
            a.off = static_cast<unsigned>(at - r * spr);
            a.n = static_cast<unsigned>(len);
            a.qsign = conj ? -1.0f : 1.0f;
            a.n_sel = n_sel;
            for (int i = 0; i < n_sel; i++)
                {
                    a.ch[i] = channels[i];
                    a.dst[i] = d_dst[i] + done;
                }
            const unsigned blocks = static_cast<unsigned>((len + 2ull * RG_THREADS - 1ull) / (2ull * RG_THREADS));
            if (c.rbytes == 8)
                unpack_register_kernel<unsigned long long><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            else if (c.rbytes == 4)
                unpack_register_kernel<unsigned><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            else
                unpack_register_kernel<unsigned short><<<dim3(blocks), dim3(RG_THREADS), 0, s>>>(a, c);
            GSH_HIP(hipGetLastError());
        }
    return GSH_OK;
}
}  // namespace gsh
