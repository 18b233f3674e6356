"""Rate of the LabSat 3 Wideband three-ring push against the GSS6450 three-band push (a tool, not a test; needs the GPU).

One device-resident block of N = 10 000 000 samples per RF channel into the same three rings (capacity N: every push starts at ring position 0 and is
one launch), in one process on one device:
  LS3W     gsh_stream_push_packed_multi_device of a (QUA 2, CHN 3) LabSat 3 Wideband block: 5 samples of every channel per 64-bit register, 16 MB
  GSS6450  the same call on a 3-band 2-bit GSS6450 block: 8 samples per 32-bit word, words dealt round-robin over the bands, 15 MB: the yardstick
           (same tree, same output bytes, an existing kernel)
Each push is queued on a stream of the tool's between two device events (the unpack kernel, the three mirror copies and the rings' bookkeeping of the
push: the same for both); a warm-up of 5 pushes each, then `--runs` pushes each, alternating, so that drift hits both alike.  Mean, standard
deviation, min and max over the runs; the output rate is 3 N x 8 bytes over the mean.

    python profiles/labsat_rate.py [--out profiles/labsat_rate.txt] [--runs 30]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd.sample_stream import PackedFormat, SampleStream, packed_bytes, push_packed_multi_device

N = 10_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    ls3w = PackedFormat(PackedFormat.LS3W_2BIT, PackedFormat.IQ, 8, rf_channels=3)
    gss = PackedFormat.from_signal_source("Spir_GSS6450_File_Signal_Source", adc_bits=2, total_channels=3)
    rng = np.random.default_rng(3)
    blocks = {}
    for name, fmt in (("LS3W QUA 2 CHN 3", ls3w), ("GSS6450 2-bit 3 bands", gss)):
        nb = packed_bytes(fmt, N)
        blocks[name] = (fmt, nb, torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).to(dev))
    rings = [SampleStream(N, 1024, device=0) for _ in range(3)]
    stream = torch.cuda.Stream(device=dev)
    chans = [0, 1, 2]

    def push(name):
        fmt, _, d = blocks[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        push_packed_multi_device(rings, chans, fmt, d.data_ptr(), N, False, hip_stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(5):
        for name in blocks:
            push(name)
    us = {name: [] for name in blocks}
    for _ in range(a.runs):
        for name in blocks:
            us[name].append(push(name))
    say("three-ring push of one device-resident block, %d samples per RF channel (%d MB out), device events around the push; %d runs each, alternating"
        % (N, 3 * N * 8 // 1_000_000, a.runs))
    say("%-24s %10s %10s %10s %10s %10s %12s" % ("", "packed MB", "mean us", "std us", "min us", "max us", "output GB/s"))
    stat = {}
    for name, v in us.items():
        v = np.array(v)
        stat[name] = (v.mean(), v.std(ddof=1))
        say("%-24s %10.1f %10.1f %10.1f %10.1f %10.1f %12.0f" % (name, blocks[name][1] / 1e6, v.mean(), v.std(ddof=1), v.min(), v.max(), 3 * N * 8 / v.mean() / 1e3))
    (m_l, s_l), (m_g, s_g) = stat["LS3W QUA 2 CHN 3"], stat["GSS6450 2-bit 3 bands"]
    spread = max(s_l, s_g)
    say("LS3W over GSS6450: %.2fx (%+.1f us; twice the larger standard deviation: %.1f us) -> %s" %
        (m_l / m_g, m_l - m_g, 2 * spread, "slower than the yardstick beyond the spread" if m_l - m_g > 2 * spread else "not slower than the yardstick beyond the spread"))
    for r in rings:
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
