#!/usr/bin/env python3
"""Mint tests/golden/cnav.npz from the REFERENCE ITSELF: libswiftcnav (src/algorithms/telemetry_decoder/libs/libswiftcnav/: cnav_msg.c, viterbi27.c,
bits.c, edc.c), plain C without dependencies, compiled in a temporary directory from where it lies in the reference tree with a small driver of this
script's own.  No stand-in is needed.  Run in the build container only:

    python tests/golden/make_golden_cnav.py <path to the reference tree> [--time]

The driver feeds cnav_msg_decoder_add_symbol one symbol at a time.  For every case <name> the file holds
    sym__<name>    uint8 [n]        the symbols as the library takes them (0x00 a certain 0, 0xFF a certain 1)
    msg__<name>    uint8 [k, 60]    the k deliveries as gsh_cnav_message records (include/gnss_sdr_hip.h), in order
    state__<name>  uint8 [2480]     the final cnav_msg_decoder_t as a gsh_cnav_channel_state
and `names` lists the cases.  The normalisation case also has raise_at / raise_by: after raise_at symbols the driver adds raise_by to all 128 metrics
of both parts of the live decoder (the only way to come near the 2^30 threshold of viterbi27.c:159 without some two million steps).
The encoder is this script's own: K = 7, 171o / 133o, continuous (no tail, no interleaver), messages of preamble 0x8B + PRN + message id + TOW + alert
+ random payload + CRC-24Q (IS-GPS-200, 30.3.3 and 3.3.3.1.1).
Cases: six messages after a garbage prefix of 0..3 symbols, upright and inverted, at noise sigma 0, 0.5, 0.7 and 1.0 of the amplitude, hard-clipped
and soft-quantised; loss of lock (3 messages, 13 messages' worth of random bits, 5 messages; prefix 0 and 1); a false preamble in every message, after a random
prefix and in a stream that begins inside a message so that the false one is met first; normalisation; noise only.
Checked at minting time (redraw SEED if one fails, never weaken it): the file holds a delivery by part 1, one by part 2, an inverted one, one whose
invert_or is set while the delivering part is upright, a drop of lock followed by a relock, a failed CRC without lock followed by a later lock, a
stream without deliveries and a stream in which normalisation fired; and the counts observed when the cases were designed (clean streams deliver 5,
the first at symbol 703 / 702 for an even / odd prefix; loss of lock delivers 3 + 4; the false preamble costs one message of 5).
--time prints the reference's messages per second on one thread of this host over 256 x 6 000 clean symbols."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0xC9A5
SIGMAS = (0.0, 0.5, 0.7, 1.0)
RAISE_AT, RAISE_BY = 200, (1 << 30) - 1000
MAX_MSGS = 64

DRIVER = r"""
#include "cnav_msg.h"
#include <string.h>

static unsigned flags_of(const cnav_v27_part_t* p)
{
    return (p->preamble_seen ? 1u : 0u) | (p->invert ? 2u : 0u) | (p->message_lock ? 4u : 0u) | (p->crc_ok ? 8u : 0u) | (p->init ? 16u : 0u);
}

/* one part as 32-bit words: old[64] new[64] decisions[128] symbols[128] decoded[64] index n_symbols n_decoded flags n_crc_fail */
static void export_part(const cnav_v27_part_t* p, uint32_t* out)
{
    int i;
    for (i = 0; i < 64; i++) *out++ = p->dec.old_metrics[i];
    for (i = 0; i < 64; i++) *out++ = p->dec.new_metrics[i];
    for (i = 0; i < 64; i++)
        {
            *out++ = p->decisions[i].w[0];
            *out++ = p->decisions[i].w[1];
        }
    for (i = 0; i < 128; i++) *out++ = p->symbols[i];
    for (i = 0; i < 64; i++) *out++ = p->decoded[i];
    *out++ = p->dec.decisions_index;
    *out++ = (uint32_t)p->n_symbols;
    *out++ = (uint32_t)p->n_decoded;
    *out++ = flags_of(p);
    *out++ = (uint32_t)p->n_crc_fail;
}

/* meta per delivery: index delay tow prn msg_id alert part inv1 inv2 lock1 lock2; raw: 64 bytes.
 * events: [0] a CRC failed in a part without lock, [1] ... and that part or its twin locked later, [2] locks dropped, [3] locks gained after a drop,
 * [4] normalisations seen.  Returns the number of deliveries. */
int drv_run(const uint8_t* sym, uint32_t n, uint32_t raise_at, uint32_t raise_by, uint32_t* meta, uint8_t* raw, int max_msgs, uint32_t* state,
    uint32_t* events)
{
    cnav_msg_decoder_t dec;
    cnav_msg_t msg;
    uint32_t delay = 0;
    uint32_t k;
    int count = 0;
    int p;
    cnav_msg_decoder_init(&dec);
    memset(events, 0, 5 * sizeof(uint32_t));
    for (k = 0; k < n; k++)
        {
            cnav_v27_part_t* parts[2] = {&dec.part1, &dec.part2};
            bool lock_before[2], seen_before[2];
            size_t dec_before[2], sym_before[2];
            uint32_t m0_before[2];
            if (raise_by && k == raise_at)
                {
                    int i;
                    for (p = 0; p < 2; p++)
                        for (i = 0; i < 64; i++)
                            {
                                parts[p]->dec.metrics1[i] += raise_by;
                                parts[p]->dec.metrics2[i] += raise_by;
                            }
                }
            for (p = 0; p < 2; p++)
                {
                    lock_before[p] = parts[p]->message_lock;
                    seen_before[p] = parts[p]->preamble_seen;
                    dec_before[p] = parts[p]->n_decoded;
                    sym_before[p] = parts[p]->n_symbols;
                    m0_before[p] = parts[p]->dec.old_metrics[0];
                }
            memset(&msg, 0, sizeof(msg));
            if (cnav_msg_decoder_add_symbol(&dec, sym[k], &msg, &delay))
                {
                    if (count < max_msgs)
                        {
                            uint32_t* m = meta + 11 * count;
                            m[0] = k;
                            m[1] = delay;
                            m[2] = msg.tow;
                            m[3] = msg.prn;
                            m[4] = msg.msg_id;
                            m[5] = msg.alert ? 1u : 0u;
                            m[6] = dec.part1.message_lock ? 1u : 2u;
                            m[7] = dec.part1.invert ? 1u : 0u;
                            m[8] = dec.part2.invert ? 1u : 0u;
                            m[9] = dec.part1.message_lock ? 1u : 0u;
                            m[10] = dec.part2.message_lock ? 1u : 0u;
                            memcpy(raw + 64 * count, msg.raw_msg, 64);
                        }
                    count++;
                }
            for (p = 0; p < 2; p++)
                {
                    const bool decoded_now = sym_before[p] + 1 >= 64 && parts[p]->n_symbols == 0 && !lock_before[1 - p];
                    if (decoded_now && !lock_before[p] && seen_before[p] && dec_before[p] + 32 >= 300 && !parts[p]->message_lock) events[0]++;
                    if (!lock_before[p] && parts[p]->message_lock)
                        {
                            if (events[0]) events[1]++;
                            if (events[2]) events[3]++;
                        }
                    if (lock_before[p] && !parts[p]->message_lock) events[2]++;
                    if (m0_before[p] > (1u << 30) && parts[p]->dec.old_metrics[0] < (1u << 29)) events[4]++;
                }
        }
    export_part(&dec.part1, state);
    export_part(&dec.part2, state + 453);
    return count;
}
"""

MESSAGE = np.dtype([("bits", "<u4", 10), ("symbol_index", "<u4"), ("delay", "<u4"), ("tow", "<u4"), ("prn", "u1"), ("msg_id", "u1"), ("alert", "u1"),
                    ("part", "u1"), ("invert", "u1"), ("invert_or", "u1"), ("reserved", "u1", 2)])
PART = np.dtype([("decisions", "<u8", 64), ("old_metrics", "<u4", 64), ("new_metrics", "<u4", 64), ("symbols", "u1", 128), ("decoded", "<u4", 16),
                 ("decisions_index", "<u4"), ("n_symbols", "<u4"), ("n_decoded", "<u4"), ("flags", "<u4"), ("n_crc_fail", "<u4"), ("reserved", "<u4")])
assert MESSAGE.itemsize == 60 and PART.itemsize == 1240


def build_reference(reference):
    libs = os.path.join(reference, "src", "algorithms", "telemetry_decoder", "libs", "libswiftcnav")
    tmp = tempfile.mkdtemp(prefix="golden_cnav_")
    with open(os.path.join(tmp, "driver.c"), "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libcnav_ref.so")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I" + libs, os.path.join(tmp, "driver.c")] +
                   [os.path.join(libs, name) for name in ("cnav_msg.c", "viterbi27.c", "bits.c", "edc.c")] + ["-o", so], check=True)
    lib = C.CDLL(so)
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    lib.drv_run.argtypes = [u8, C.c_uint32, C.c_uint32, C.c_uint32, u32, u8, C.c_int, u32, u32]
    return lib


def run_reference(lib, sym, raise_at=0, raise_by=0):
    """-> (messages as MESSAGE records, state bytes, events, lock flags per delivery)"""
    sym = np.ascontiguousarray(sym, np.uint8)
    meta = np.zeros((MAX_MSGS, 11), np.uint32)
    raw = np.zeros((MAX_MSGS, 64), np.uint8)
    state = np.zeros(2 * 453, np.uint32)
    events = np.zeros(5, np.uint32)
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    n = lib.drv_run(sym.ctypes.data_as(u8), len(sym), raise_at, raise_by, meta.ctypes.data_as(u32), raw.ctypes.data_as(u8), MAX_MSGS,
                    state.ctypes.data_as(u32), events.ctypes.data_as(u32))
    assert n <= MAX_MSGS
    msgs = np.zeros(n, MESSAGE)
    for i in range(n):
        m = meta[i]
        bits = np.unpackbits(raw[i])[:300]
        msgs[i]["bits"] = np.packbits(np.concatenate([bits, np.zeros(20, np.uint8)])).view(">u4").astype("<u4")
        msgs[i]["symbol_index"], msgs[i]["delay"], msgs[i]["tow"] = m[0], m[1], m[2]
        msgs[i]["prn"], msgs[i]["msg_id"], msgs[i]["alert"], msgs[i]["part"] = m[3], m[4], m[5], m[6]
        msgs[i]["invert"] = m[7] if m[6] == 1 else m[8]
        msgs[i]["invert_or"] = m[7] | m[8]
    parts = np.zeros(2, PART)
    for p in range(2):
        s = state[453 * p:453 * (p + 1)]
        parts[p]["old_metrics"], parts[p]["new_metrics"] = s[0:64], s[64:128]
        parts[p]["decisions"] = s[128:256:2].astype(np.uint64) | (s[129:256:2].astype(np.uint64) << np.uint64(32))
        parts[p]["symbols"] = s[256:384].astype(np.uint8)
        parts[p]["decoded"] = s[384:448].astype(np.uint8).view(">u4").astype("<u4")
        for k, name in enumerate(("decisions_index", "n_symbols", "n_decoded", "flags", "n_crc_fail")):
            parts[p][name] = s[448 + k]
    return msgs, parts.view(np.uint8).copy(), events, meta[:n, 9:11].copy()


def parity(w):
    return bin(w).count("1") & 1


def crc24q(bits):
    reg = 0
    for b in bits:
        top = (reg >> 23) & 1
        reg = (reg << 1) & 0xFFFFFF
        if top ^ int(b):
            reg ^= 0x864CFB
    return reg


def field(value, width):
    return [(value >> (width - 1 - i)) & 1 for i in range(width)]


def message(rng, prn, msg_id, tow, alert, false_preamble=False):
    payload = rng.integers(0, 2, 238).tolist()
    if false_preamble:
        payload[2:10] = field(0x8B, 8)  # message bit 40
    bits = field(0x8B, 8) + field(prn, 6) + field(msg_id, 6) + field(tow, 17) + [alert] + payload
    assert len(bits) == 276
    return bits + field(crc24q(bits), 24)


def encode(bits):
    """171o / 133o with the newest bit in the register's lowest place, where those generators read 0x4F / 0x6D; -> one 0/1 symbol pair per bit"""
    sr, out = 0, []
    for b in bits:
        sr = ((sr << 1) | int(b)) & 0x7F
        out += [parity(sr & 0x4F), parity(sr & 0x6D)]
    return np.array(out, np.uint8)


def stream(rng, n_good, prefix, inverted, tow0=1000, false_preamble=False, gap_bits=0, n_after=0, cut=0):
    bits = []
    for k in range(n_good):
        bits += message(rng, 1 + (tow0 + k) % 32, 10 + k % 6, tow0 + k, k & 1, false_preamble)
    if gap_bits:
        bits += rng.integers(0, 2, gap_bits).tolist()
        for k in range(n_after):
            bits += message(rng, 7, 30 + k % 4, tow0 + 100 + k, 0)
    if cut:
        bits = bits[cut:]
    elif false_preamble:
        bits = rng.integers(0, 2, 37).tolist() + bits
    chips = encode(bits)
    if inverted:
        chips = 1 - chips
    return np.concatenate([rng.integers(0, 2, prefix).astype(np.uint8), chips]).astype(np.float64) * 2.0 - 1.0


def hard(x):
    return ((x > 0) * 255).astype(np.uint8)


def soft(x):
    return np.rint(np.float32(127.5) + np.float32(127.5) * np.clip(x.astype(np.float32), np.float32(-1), np.float32(1))).astype(np.uint8)


def timing(lib):
    rng = np.random.default_rng(SEED)
    sym = hard(stream(rng, 10, 0, False))
    assert len(sym) == 6000
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        n = sum(len(run_reference(lib, sym)[0]) for _ in range(256))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print(f"reference, one host thread: 256 x 6000 symbols in {best * 1e3:.1f} ms, {n} messages, {n / best:.0f} messages/s, {256 * 6000 / best / 1e6:.2f} Msym/s")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit("usage: make_golden_cnav.py <path to the reference tree> [--time]")
    lib = build_reference(args[0])
    if "--time" in sys.argv:
        timing(lib)
        return
    rng = np.random.default_rng(SEED)
    cases = {}   # name -> (symbols, raise_at, raise_by)
    for prefix in range(4):
        for inverted in (False, True):
            base = stream(rng, 6, prefix, inverted)
            for sigma in SIGMAS:
                x = base + sigma * rng.standard_normal(len(base))
                tag = f"p{prefix}_{'inv' if inverted else 'up'}_s{int(sigma * 10):02d}"
                cases["hard_" + tag] = (hard(x), 0, 0)
                cases["soft_" + tag] = (soft(x), 0, 0)
    for prefix in (0, 1):
        cases[f"loss_p{prefix}"] = (hard(stream(rng, 3, prefix, False, gap_bits=13 * 300, n_after=5)), 0, 0)
    cases["false_preamble"] = (hard(stream(rng, 5, 0, False, false_preamble=True)), 0, 0)
    # the stream begins at bit 38 of a message, so the first preamble the decoder meets is the false one: 300 bits, a failed CRC, a rescan
    cases["false_preamble_first"] = (hard(stream(rng, 6, 0, False, false_preamble=True, cut=38)), 0, 0)
    cases["normalise"] = (hard(stream(rng, 6, 0, False)), RAISE_AT, RAISE_BY)
    cases["noise"] = (rng.integers(0, 256, 4000).astype(np.uint8), 0, 0)

    out = {"names": np.array(list(cases)), "raise_at": np.uint32(RAISE_AT), "raise_by": np.uint32(RAISE_BY)}
    seen = dict(part1=0, part2=0, inverted=0, stale_or=0, relock=0, rescan_lock=0, empty=0, normalised=0)
    for name, (sym, at, by) in cases.items():
        msgs, state, events, locks = run_reference(lib, sym, at, by)
        out["sym__" + name], out["msg__" + name], out["state__" + name] = sym, msgs.view(np.uint8).reshape(len(msgs), 60), state
        seen["part1"] += int(np.sum(msgs["part"] == 1))
        seen["part2"] += int(np.sum(msgs["part"] == 2))
        seen["inverted"] += int(np.sum(msgs["invert"] == 1))
        seen["stale_or"] += int(np.sum((msgs["invert_or"] == 1) & (msgs["invert"] == 0)))
        seen["relock"] += int(events[2] > 0 and events[3] > 0)
        seen["rescan_lock"] += int(events[0] > 0 and events[1] > 0)
        seen["empty"] += int(len(msgs) == 0)
        seen["normalised"] += int(events[4] > 0)
        assert all(l1 != l2 for l1, l2 in locks), name  # exactly one part holds the lock at a delivery
        print(f"{name:24s} {len(sym):6d} symbols, {len(msgs)} messages, first at {msgs['symbol_index'][0] if len(msgs) else '-'}, events {events.tolist()}")
        clean = name.endswith("_s00")
        if clean or name.endswith("_s05") and name.startswith("hard_"):
            assert len(msgs) == 5, name
        if clean:
            odd = int(name.split("_")[1][1]) & 1
            assert msgs["symbol_index"][0] == (702 if odd else 703) and np.all(msgs["part"] == (2 if odd else 1)), name
            assert np.all(msgs["invert"] == ("_inv_" in name)) and msgs["tow"].tolist() == list(range(1000, 1005)), name
        if name.endswith("_s10") and name.startswith("hard_"):
            assert len(msgs) == 0, name
        if name.startswith("loss_"):
            assert len(msgs) == 7 and events[2] > 0 and events[3] > 0, name
        if name == "false_preamble":
            assert len(msgs) == 4, name
        if name == "false_preamble_first":
            assert len(msgs) >= 3 and events[0] > 0 and events[1] > 0, name
        if name == "normalise":
            assert events[4] > 0 and len(msgs) == 5, name
        if name == "noise":
            assert len(msgs) == 0, name
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    path = os.path.join(HERE, "cnav.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
