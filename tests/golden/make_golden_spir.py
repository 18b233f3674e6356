"""Mint tests/golden/spir_1bit.npz: the raw output of the reference's own unpack_intspir_1bit_samples block
(src/algorithms/signal_source/gnuradio_blocks/unpack_intspir_1bit_samples.cc) over every value of the low byte (the other bytes zero), the words 0 and
0xFFFFFFFF, and 1 024 random words.  The block is compiled from the reference tree in a temporary directory against the GNU Radio stand-ins of
tests/host/mock_gnuradio/ (sync_interpolator.h); nothing compiled stays.  No test runs this script: tests/test_labsat_formats.py checks
tests/labsat_reference.py against what it wrote.

    python tests/golden/make_golden_spir.py /path/to/gnss-sdr"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

DRIVER = r"""
#include "unpack_intspir_1bit_samples.h"
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

int main(int, char** argv)
{
    const std::string dir = argv[1];
    std::vector<int32_t> words;
    {
        FILE* f = std::fopen((dir + "/words.bin").c_str(), "rb");
        int32_t w;
        while (std::fread(&w, 4, 1, f) == 1) words.push_back(w);
        std::fclose(f);
    }
    const int nout = 2 * static_cast<int>(words.size());  // the block writes two floats (I, Q) per input int
    std::vector<float> out(nout);
    gr_vector_const_void_star ins{words.data()};
    gr_vector_void_star outs{out.data()};
    make_unpack_intspir_1bit_samples()->work(nout, ins, outs);
    std::vector<int16_t> iq(nout);
    for (int k = 0; k < nout; k++)
        {
            iq[k] = static_cast<int16_t>(out[k]);
            if (static_cast<float>(iq[k]) != out[k]) return 2;  // not a 16-bit integer
        }
    FILE* f = std::fopen((dir + "/out.bin").c_str(), "wb");
    std::fwrite(iq.data(), 2, iq.size(), f);
    std::fclose(f);
    return 0;
}
"""


def input_words() -> np.ndarray:
    low = np.arange(256, dtype=np.uint32)
    rnd = np.random.default_rng(1337).integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([low, np.array([0, 0xFFFFFFFF], np.uint32), rnd]).astype(np.uint32)


def main(reference):
    blk = os.path.join(reference, "src", "algorithms", "signal_source", "gnuradio_blocks")
    words = input_words()
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cc")
        with open(drv, "w") as f:
            f.write(DRIVER)
        words.astype("<u4").tofile(os.path.join(tmp, "words.bin"))
        exe = os.path.join(tmp, "mint")
        subprocess.run(["g++", "-O1", "-std=c++17", "-DGNURADIO_USES_STD_POINTERS=1", "-I" + os.path.join(ROOT, "tests", "host", "mock_gnuradio"),
                        "-I" + blk, "-I" + os.path.join(reference, "src", "core", "interfaces"), "-o", exe, drv,
                        os.path.join(blk, "unpack_intspir_1bit_samples.cc")], check=True)
        subprocess.run([exe, tmp], check=True)
        iq = np.fromfile(os.path.join(tmp, "out.bin"), "<i2").reshape(-1, 2)
    path = os.path.join(HERE, "spir_1bit.npz")
    np.savez_compressed(path, words=words, iq=iq)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
