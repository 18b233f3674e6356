#!/usr/bin/env python3
"""Mint tests/golden/viterbi.npz from the REFERENCE ITSELF: Viterbi_Decoder (src/algorithms/telemetry_decoder/libs/viterbi_decoder.cc), compiled in a
temporary directory from where it lies in the reference tree, against a small stand-in for volk_gnsssdr_32f_index_max_32u (first maximum wins).
Run in the build container only:

    python tests/golden/make_golden_viterbi.py [path to the reference tree]

For each of the three Galileo page lengths (I/NAV part 114, F/NAV 238, C/NAV 486 information bits) the file holds PAGES pages at every pair of
amplitude (1, 2500) and noise sigma (0, 0.3, 0.6, 1.0 times the amplitude), in that order:
    <name>__sym     float32 [n, symbols]  the symbols after the preamble as received (interleaved, G2 inverted)
    <name>__tx      uint8   [n, bits]     the transmitted information bits
    <name>__fresh   uint8   [n, bits]     the reference's output, a fresh Viterbi_Decoder per page
    <name>__reused  uint8   [n, bits]     the reference's output, ONE Viterbi_Decoder over the n pages in sequence (how the block uses it)
    <name>__ml      uint8   [n, bits]     a float64 both-symbol maximum-likelihood decoder (this script's own code)
    <name>__amp, <name>__sigma  float64 [n]
and the CRC-24Q known answer (crc_message = ASCII "123456789", crc_value = 0xCDE703, checked here against this script's bit-serial CRC).
The encoder is this script's own: convolutional code 171o / 133o with G2 inverted, tail of 6 zeros, 8-row block interleaver (Galileo OS SIS ICD 4.1.4).
Checked at minting time: on every page with sigma <= 0.3 the float64 decoder recovers the transmitted bits (redraw SEED if not)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x71B17
PAGES = 4
LENGTHS = {"inav": (114, 30), "fnav": (238, 61), "cnav": (486, 123)}  # information bits, interleaver columns (8 rows)
AMPS = (1.0, 2500.0)
SIGMAS = (0.0, 0.3, 0.6, 1.0)

VOLK_STANDIN = r"""
#pragma once
#include <cstdint>
static inline void volk_gnsssdr_32f_index_max_32u(uint32_t* target, const float* src0, uint32_t num_points)
{
    uint32_t index = 0;
    for (uint32_t i = 1; i < num_points; i++)
        if (src0[i] > src0[index]) index = i;
    *target = index;
}
"""

DRIVER = r"""
#include "viterbi_decoder.h"
extern "C" void* vd_new(int info_bits) { return new Viterbi_Decoder(7, 2, info_bits, std::array<int32_t, 2>{{121, 91}}); }
extern "C" void vd_delete(void* p) { delete static_cast<Viterbi_Decoder*>(p); }
extern "C" void vd_decode(void* p, const float* soft, int n_soft, int32_t* bits, int n_bits)
{
    std::vector<float> in(soft, soft + n_soft);
    std::vector<int32_t> out(n_bits);
    static_cast<Viterbi_Decoder*>(p)->decode(out, in);
    for (int i = 0; i < n_bits; i++) bits[i] = out[i];
}
"""


def build_reference(reference):
    libs = os.path.join(reference, "src", "algorithms", "telemetry_decoder", "libs")
    tmp = tempfile.mkdtemp(prefix="golden_viterbi_")
    os.makedirs(os.path.join(tmp, "volk_gnsssdr"))
    with open(os.path.join(tmp, "volk_gnsssdr", "volk_gnsssdr.h"), "w") as f:
        f.write(VOLK_STANDIN)
    with open(os.path.join(tmp, "driver.cc"), "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libviterbi_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + tmp, "-I" + libs, os.path.join(tmp, "driver.cc"),
                    os.path.join(libs, "viterbi_decoder.cc"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.vd_new.restype = C.c_void_p
    lib.vd_new.argtypes = [C.c_int]
    lib.vd_delete.argtypes = [C.c_void_p]
    lib.vd_decode.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int32), C.c_int]
    return lib


def parity(w):
    return bin(w).count("1") & 1


def encode(info, cols):
    out, state = [], 0
    for b in list(info) + [0] * 6:
        word = (int(b) << 6) ^ state
        out += [parity(word & 0o171), parity(word & 0o133) ^ 1]
        state = word >> 1
    coded = np.array(out, np.uint8)
    return (2.0 * coded.reshape(cols, 8).T.reshape(-1) - 1.0)  # written by columns, sent by rows; +1 for a 1


def receiver_soft(sym, cols):
    """what galileo_telemetry_decoder_gs hands to Viterbi_Decoder::decode (:352-377)"""
    soft = np.asarray(sym, np.float32).reshape(8, cols).T.reshape(-1).copy()
    soft[1::2] = -soft[1::2]
    return soft


def ml_decode(soft, n_bits):
    """plain float64 Viterbi over both symbols of every pair, from state 0 to state 0"""
    soft = np.asarray(soft, np.float64)
    steps = len(soft) // 2
    s = np.arange(64)
    pred = 2 * (s & 31)
    sym = [np.array([[parity((((k >> 5) << 6) ^ p) & 0o171), parity((((k >> 5) << 6) ^ p) & 0o133)] for k, p in zip(s, pred + d)], np.float64) for d in (0, 1)]
    metric = np.full(64, -np.inf)
    metric[0] = 0.0
    dec = np.zeros((steps, 64), np.uint8)
    for t in range(steps):
        r = soft[2 * t:2 * t + 2]
        cand = [metric[pred + d] + sym[d] @ r for d in (0, 1)]
        dec[t] = cand[1] > cand[0]
        metric = np.maximum(cand[0], cand[1])
    bits, state = np.zeros(n_bits, np.uint8), 0
    for t in range(steps - 1, -1, -1):
        if t < n_bits:
            bits[t] = state >> 5
        state = 2 * (state & 31) + int(dec[t, state])
    return bits


def crc24q(bits):
    reg = 0
    for b in bits:
        top = (reg >> 23) & 1
        reg = (reg << 1) & 0xFFFFFF
        if top ^ int(b):
            reg ^= 0x864CFB
    return reg


def ref_decode(lib, obj, soft, n_bits):
    soft = np.ascontiguousarray(soft, np.float32)
    out = np.zeros(n_bits, np.int32)
    lib.vd_decode(obj, soft.ctypes.data_as(C.POINTER(C.c_float)), len(soft), out.ctypes.data_as(C.POINTER(C.c_int32)), n_bits)
    return out.astype(np.uint8)


def main():
    reference = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    lib = build_reference(reference)
    rng = np.random.default_rng(SEED)
    store = {}
    for name, (n_bits, cols) in LENGTHS.items():
        sym, tx, fresh, reused, ml, amps, sigmas = [], [], [], [], [], [], []
        one = lib.vd_new(n_bits)
        for amp in AMPS:
            for sigma in SIGMAS:
                for _ in range(PAGES):
                    info = rng.integers(0, 2, n_bits).astype(np.uint8)
                    page = (amp * (encode(info, cols) + sigma * rng.standard_normal(8 * cols))).astype(np.float32)
                    soft = receiver_soft(page, cols)
                    obj = lib.vd_new(n_bits)
                    fresh.append(ref_decode(lib, obj, soft, n_bits))
                    lib.vd_delete(obj)
                    reused.append(ref_decode(lib, one, soft, n_bits))
                    ml.append(ml_decode(soft, n_bits))
                    if sigma <= 0.3:
                        assert np.array_equal(ml[-1], info), f"{name}: the float64 decoder misses a page at sigma {sigma}: redraw SEED"
                    sym.append(page)
                    tx.append(info)
                    amps.append(amp)
                    sigmas.append(sigma)
        lib.vd_delete(one)
        for key, val in (("sym", np.array(sym, np.float32)), ("tx", np.array(tx)), ("fresh", np.array(fresh)), ("reused", np.array(reused)),
                         ("ml", np.array(ml)), ("amp", np.array(amps)), ("sigma", np.array(sigmas))):
            store[f"{name}__{key}"] = val
        tx_a, sg = np.array(tx), np.array(sigmas)
        for s_ in SIGMAS:
            m = sg == s_
            print(f"{name} sigma {s_}: bit errors of {tx_a[m].size}: fresh {int((np.array(fresh)[m] != tx_a[m]).sum())} reused "
                  f"{int((np.array(reused)[m] != tx_a[m]).sum())} float64 ML {int((np.array(ml)[m] != tx_a[m]).sum())}")
    message = np.frombuffer(b"123456789", np.uint8)
    assert crc24q(np.unpackbits(message)) == 0xCDE703
    store["crc_message"] = message
    store["crc_value"] = np.array([0xCDE703], np.uint32)
    store["names"] = np.array(list(LENGTHS))
    out = os.path.join(HERE, "viterbi.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
