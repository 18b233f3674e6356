"""Rate of the table-driven ION_GSMS three-ring push against the specialised GSS6450 push of the same bytes (a tool, not a test; needs the GPU).

One device-resident block of N = 10 000 000 samples per band, 30 MB, into the same three rings (capacity N: every push starts at ring position 0
and is one launch), in one process on one device:
  ION_GSMS  gsh_stream_push_ion_device with the layout that expresses GSS6450 4-bit, endian 0, three bands: one chunk of three 32-bit
            little-endian words, three streams of packed_bits 32 and rate_factor 4, 4-bit TC, format QI (unpack_ion_kernel)
  GSS6450   gsh_stream_push_packed_multi_device of the same bytes as GSH_PACKED_GSS6450_4BIT: the yardstick (same tree, same output, bit for bit:
            checked below before anything is timed)
Each push is queued on a stream of the tool's between two device events (the unpack kernel, the three mirror copies and the rings' bookkeeping of the
push: the same for both); a warm-up of 5 pushes each, then `--runs` pushes each, alternating, so that drift hits both alike.  Mean, standard
deviation, min and max over the runs; the output rate is 3 N x 8 bytes over the mean.

    python profiles/ion_gsms_rate.py [--out profiles/ion_gsms_rate.txt] [--runs 30]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd.ion_gsms import IonLayout
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
    gss = PackedFormat(PackedFormat.GSS6450_4BIT, PackedFormat.IQ, 4, rf_channels=3)
    lay = IonLayout([dict(size_word=4, count_words=3, n_streams=3)],
                    [dict(packed_bits=32, rate_factor=4, quantization=4, encoding="TC", format="qi", name=f"band{b}") for b in range(3)])
    nb = packed_bytes(gss, N)
    assert nb == lay.bytes_for(0, N) == 3 * N
    d = torch.from_numpy(np.random.default_rng(3).integers(0, 256, nb, dtype=np.uint8)).to(dev)
    rings = [SampleStream(N, 1024, device=0) for _ in range(3)]
    stream = torch.cuda.Stream(device=dev)
    chans = [0, 1, 2]
    pushes = {
        "ION_GSMS layout (generic)": lambda: lay.push_device(rings, chans, d.data_ptr(), N, False, hip_stream=stream.cuda_stream),
        "GSS6450 4-bit 3 bands": lambda: push_packed_multi_device(rings, chans, gss, d.data_ptr(), N, False, hip_stream=stream.cuda_stream),
    }

    def push(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        pushes[name]()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    # the two pushes leave the same samples: the last 100 000 of every ring, read back after each
    tails = {}
    for name in pushes:
        for r in rings:
            r.seek(0)
        push(name)
        tails[name] = [r.read(N - 100_000, 100_000) for r in rings]
    names = list(pushes)
    for x, y in zip(tails[names[0]], tails[names[1]]):
        if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            raise RuntimeError("the ION_GSMS push and the GSS6450 push of the same bytes left different samples")
    for _ in range(5):
        for name in pushes:
            push(name)
    us = {name: [] for name in pushes}
    for _ in range(a.runs):
        for name in pushes:
            us[name].append(push(name))
    say("three-ring push of one device-resident block, %d samples per band (%d MB packed, %d MB out), device events around the push; %d runs each, alternating"
        % (N, nb // 1_000_000, 3 * N * 8 // 1_000_000, a.runs))
    say("%-28s %10s %10s %10s %10s %12s" % ("", "mean us", "std us", "min us", "max us", "output GB/s"))
    stat = {}
    for name, v in us.items():
        v = np.array(v)
        stat[name] = (v.mean(), v.std(ddof=1))
        say("%-28s %10.1f %10.1f %10.1f %10.1f %12.0f" % (name, v.mean(), v.std(ddof=1), v.min(), v.max(), 3 * N * 8 / v.mean() / 1e3))
    (m_i, s_i), (m_g, s_g) = stat[names[0]], stat[names[1]]
    say("generic over specialised: %.2fx the time (%+.1f us; twice the larger standard deviation: %.1f us); the generic kernel runs at %.0f %% of the specialised rate"
        % (m_i / m_g, m_i - m_g, 2 * max(s_i, s_g), 100 * m_g / m_i))
    for r in rings:
        r.close()
    lay.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
