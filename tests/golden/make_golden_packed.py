"""Mint tests/golden/packed_formats.npz: the raw outputs of the reference's own unpack blocks (src/algorithms/signal_source/gnuradio_blocks/
unpack_2bit_samples.cc, unpack_byte_2bit_cpx_samples.cc, unpack_byte_4bit_samples.cc, unpack_byte_2bit_samples.cc, unpack_ntlab_2bit_samples.cc)
for every byte value 0..255 and, for unpack_2bit_samples with 16-bit items, every item value 0..65535 (little-endian in memory), in every
option the signal sources use.  The blocks are compiled from the reference tree in a temporary directory against the GNU Radio stand-ins of
tests/host/mock_gnuradio/ (sync_interpolator.h); nothing compiled stays.  No test runs this script: tests/test_packed_formats.py checks
tests/packed_reference.py against what it wrote.

    python tests/golden/make_golden_packed.py [/path/to/gnss-sdr]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

DRIVER = r"""
#include "unpack_2bit_samples.h"
#include "unpack_byte_2bit_cpx_samples.h"
#include "unpack_byte_2bit_samples.h"
#include "unpack_byte_4bit_samples.h"
#include "unpack_ntlab_2bit_samples.h"
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

static void save(const std::string& dir, const std::string& name, const void* p, size_t bytes)
{
    FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

template <typename OUT, typename BLK>
static std::vector<OUT> run(BLK blk, const std::vector<uint8_t>& in, int nout, int nch = 1)
{
    std::vector<OUT> out(static_cast<size_t>(nout) * nch);
    gr_vector_const_void_star ins{in.data()};
    gr_vector_void_star outs;
    for (int c = 0; c < nch; c++) outs.push_back(out.data() + static_cast<size_t>(c) * nout);
    blk->work(nout, ins, outs);
    return out;
}

int main(int, char** argv)
{
    const std::string dir = argv[1];
    std::vector<uint8_t> bytes(256), items(2 * 65536);
    for (int i = 0; i < 256; i++) bytes[i] = static_cast<uint8_t>(i);
    for (int v = 0; v < 65536; v++)
        {
            items[2 * v] = static_cast<uint8_t>(v & 0xff);  // little-endian in memory
            items[2 * v + 1] = static_cast<uint8_t>(v >> 8);
        }
    for (int beb = 0; beb < 2; beb++)
        for (int rev = 0; rev < 2; rev++)
            {
                auto b = run<int8_t>(make_unpack_2bit_samples(beb, 1, true, rev), bytes, 4 * 256);
                save(dir, "u2_byte_beb" + std::to_string(beb) + "_rev" + std::to_string(rev), b.data(), b.size());
                auto s = run<int8_t>(make_unpack_2bit_samples(beb, 2, true, rev), items, 4 * 2 * 65536);
                save(dir, "u2_short_beb" + std::to_string(beb) + "_rev" + std::to_string(rev), s.data(), s.size());
            }
    auto cpx = run<int16_t>(make_unpack_byte_2bit_cpx_samples(), bytes, 4 * 256);
    save(dir, "u2cpx", cpx.data(), cpx.size() * 2);
    auto four = run<int16_t>(make_unpack_byte_4bit_samples(), bytes, 2 * 256);
    save(dir, "u4", four.data(), four.size() * 2);
    auto nsr = run<float>(make_unpack_byte_2bit_samples(), bytes, 4 * 256);
    save(dir, "nsr", nsr.data(), nsr.size() * 4);
    auto nt = run<float>(make_unpack_ntlab_2bit_samples(1, 4), bytes, 256, 4);
    save(dir, "ntlab", nt.data(), nt.size() * 4);
    return 0;
}
"""


def main(reference="/root/reference"):
    blk = os.path.join(reference, "src", "algorithms", "signal_source", "gnuradio_blocks")
    srcs = [os.path.join(blk, n + ".cc") for n in ("unpack_2bit_samples", "unpack_byte_2bit_cpx_samples", "unpack_byte_4bit_samples",
                                                   "unpack_byte_2bit_samples", "unpack_ntlab_2bit_samples")]
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cc")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "mint")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DGNURADIO_USES_STD_POINTERS=1", "-I" + os.path.join(ROOT, "tests", "host", "mock_gnuradio"),
                        "-I" + blk, "-I" + os.path.join(reference, "src", "core", "interfaces"), "-o", exe, drv] + srcs, check=True)
        subprocess.run([exe, tmp], check=True)
        rd = lambda name, dt: np.fromfile(os.path.join(tmp, name + ".bin"), dt)
        out = {}
        for beb in (0, 1):
            for rev in (0, 1):
                out[f"u2_byte_beb{beb}_rev{rev}"] = rd(f"u2_byte_beb{beb}_rev{rev}", np.int8)
                out[f"u2_short_beb{beb}_rev{rev}"] = rd(f"u2_short_beb{beb}_rev{rev}", np.int8)
        out["u2cpx"] = rd("u2cpx", np.int16)
        out["u4"] = rd("u4", np.int16)
        out["nsr"] = rd("nsr", np.float32)
        out["ntlab"] = rd("ntlab", np.float32).reshape(4, 256)
    path = os.path.join(HERE, "packed_formats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
