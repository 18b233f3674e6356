"""Mint tests/golden/beamformer.npz: the output of the reference's own beamformer block (src/algorithms/input_filter/gnuradio_blocks/beamformer.cc,
eight inputs, weights (1, 0)) for 8 streams x 4 099 complex samples whose parts span 41 binades.  The block is compiled from the reference tree in
a temporary directory against the GNU Radio stand-ins of tests/host/mock_gnuradio/ (sync_block.h); nothing compiled stays.  No test runs this
script: tests/test_beamformer_reference.py checks tests/beamformer_reference.py against what it wrote.  The npz holds numeric arrays only:
x float32 [8, 4099, 2] (I, Q) and y float32 [4099, 2].

    python tests/golden/make_golden_beamformer.py /path/to/gnss-sdr"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_STREAMS, N_SAMPLES = 8, 4099

DRIVER = r"""
#include "beamformer.h"
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

int main(int, char** argv)
{
    const std::string dir = argv[1];
    const int n = std::stoi(argv[2]);
    std::vector<std::vector<std::complex<float>>> in(GNSS_SDR_BEAMFORMER_CHANNELS, std::vector<std::complex<float>>(n));
    FILE* f = std::fopen((dir + "/x.bin").c_str(), "rb");
    for (auto& v : in)
        if (std::fread(v.data(), sizeof(std::complex<float>), n, f) != static_cast<size_t>(n)) return 2;
    std::fclose(f);
    std::vector<std::complex<float>> out(n);
    gr_vector_const_void_star ins;
    for (auto& v : in) ins.push_back(v.data());
    gr_vector_void_star outs{out.data()};
    if (make_beamformer_sptr()->work(n, ins, outs) != n) return 3;
    f = std::fopen((dir + "/y.bin").c_str(), "wb");
    std::fwrite(out.data(), sizeof(std::complex<float>), n, f);
    std::fclose(f);
    return 0;
}
"""


def input_streams() -> np.ndarray:
    """float32 [8, 4099, 2]: normal mantissas times 2^k, k = -20 .. 20 drawn per value, a few exact zeros of either sign"""
    rng = np.random.default_rng(819)
    shape = (N_STREAMS, N_SAMPLES, 2)
    x = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, shape))).astype(np.float32)
    z = rng.random(shape) < 0.002
    x[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return x


def main(reference):
    blk = os.path.join(reference, "src", "algorithms", "input_filter", "gnuradio_blocks")
    x = input_streams()
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.cc")
        with open(drv, "w") as f:
            f.write(DRIVER)
        x.astype("<f4").tofile(os.path.join(tmp, "x.bin"))
        exe = os.path.join(tmp, "mint")
        subprocess.run(["g++", "-O2", "-std=c++17", "-DGNURADIO_USES_STD_POINTERS=1", "-I" + os.path.join(ROOT, "tests", "host", "mock_gnuradio"),
                        "-I" + blk, "-I" + os.path.join(reference, "src", "core", "interfaces"), "-o", exe, drv, os.path.join(blk, "beamformer.cc")],
                       check=True)
        subprocess.run([exe, tmp, str(N_SAMPLES)], check=True)
        y = np.fromfile(os.path.join(tmp, "y.bin"), "<f4").reshape(N_SAMPLES, 2)
    path = os.path.join(HERE, "beamformer.npz")
    np.savez_compressed(path, x=x, y=y)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
