"""Rate of the device signal generator (a tool, not a test; needs the GPU): gsh_gen_time_generate -- the launch between two device events, after
three warm-up launches -- for one block of 2^22 samples at 4 Msps, GPS L1 C/A satellites (one table each) and Galileo-E5a-shaped ones (two tables),
noise off and on.  Each figure is the average of `--reps` launches; every shape is timed three times, the range is printed.  The first figures this
unit has: the base a later change is measured against.

    python profiles/siggen_rate.py [--out profiles/siggen_rate.txt] [--reps 50]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd import SignalGenerator
from gnss_sdr_amd.signal_generator import Satellite, gps_l1_ca_satellite

N = 1 << 22
FS = 4000000


def satellites(n_sats, two_tables):
    sats = []
    for k in range(n_sats):
        s = gps_l1_ca_satellite(1 + k % 32, FS, delay_chips=37 * k, doppler_hz=-5000.0 + 300.0 * k, cn0_db=44.0)
        if two_tables:   # the E5a shape on the same period: A = (Re, 0), B = (0, Im), both signed
            t = (s.table_a + s.table_a * 1j).astype(np.complex64)
            s = Satellite(t.real.astype(np.complex64), (1j * t.imag).astype(np.complex64), s.delay_samples, np.ones(20, np.int8), np.ones(100, np.int8),
                          s.doppler_hz)
        sats.append(s)
    return sats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    lines = [f"gsh_gen_time_generate, {N} samples per launch, {a.reps} launches per figure, three figures per shape (min - max); one MI355X",
             f"{'shape':<34}{'us per launch':>22}{'Msamples/s':>16}{'sat-samples/ns':>16}"]
    for two in (False, True):
        for n_sats in (1, 8, 32):
            for noise in (False, True):
                gen = SignalGenerator(FS, n_sats)
                try:
                    for i, s in enumerate(satellites(n_sats, two)):
                        gen.set_satellite(i, s)
                    gen.set_noise(noise, 1)
                    ms = [gen.time_generate(N, a.reps) for _ in range(3)]
                finally:
                    gen.close()
                name = f"{'two tables' if two else 'one table'}, S = {n_sats:2d}, noise {'on' if noise else 'off'}"
                lines.append(f"{name:<34}{1e3 * min(ms):>11.1f} - {1e3 * max(ms):<8.1f}{N / (1e3 * min(ms)):>16.0f}{n_sats * N / (1e6 * min(ms)):>16.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
