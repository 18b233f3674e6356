"""Rate of the fused signal conditioner against the loose chain it replaces (a tool, not a test; needs the GPU).

For each shape the device work of one push -- gsh_cond_time_push: the fused launch and the history update -- and the loose chain on the same block --
gsh_convert_samples_device -> gsh_fir_process_device -> gsh_direct_resample_device, queued on one stream between two device events -- are timed
alternately, three pairs after a warm-up, in the same process on the same device.  Before any time is taken the two forms' outputs on the timed block
are compared bit for bit.  Prints a table; --out FILE also writes it there.

    python profiles/conditioner_rate.py [--out profiles/conditioner_rate.txt] [--reps 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd import SignalConditioner
from gnss_sdr_amd.sample_stream import FirFilter, SampleStream, convert_samples_device, direct_resample_device

N = 1 << 22
# name, taps, decimation, IF, filter rate, resampler (rate after the filter, rate out) or None
SHAPES = (("ibyte 2^22, K=65, D=1, 25 -> 4 Msps", 65, 1, 3.1e6, 25e6, (25e6, 4e6)),
          ("ibyte 2^22, K=33, D=2, no resampler", 33, 2, 1.2e6, 8e6, None))


def taps_of(K, D):
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (2.5 * D))).astype(np.float32)
    return t / t.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    raw = np.random.default_rng(11).integers(-100, 101, (N, 2)).astype(np.int8)
    d_raw = torch.from_numpy(raw).to(dev)
    d_x = torch.zeros(N, dtype=torch.complex64, device=dev)
    d_y = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    d_z = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    say("fused conditioner push vs the loose chain, one block of %d ibyte samples; device events, %d launches per figure" % (N, a.reps))
    say("%-40s %10s %10s %8s %12s %14s %14s" % ("shape", "fused us", "loose us", "ratio", "outputs", "fused GB/s", "loose GB/s"))
    for name, K, D, fc, fs, rs in SHAPES:
        taps = taps_of(K, D)
        fir = FirFilter(taps, D, fc, fs, "gr_complex", device=0)
        n_f = (N + D - 1) // D

        def loose(hip_stream=st.cuda_stream):
            convert_samples_device(0, d_raw.data_ptr(), "ibyte", d_x.data_ptr(), N, hip_stream=hip_stream)
            got = fir.process_device(d_x.data_ptr(), N, d_y.data_ptr(), d_y.numel(), hip_stream=hip_stream)
            assert got >= n_f - 1
            if rs is None:
                return n_f, d_y
            n_z, _cons = direct_resample_device(0, d_y.data_ptr(), 0, n_f, rs[0], rs[1], 0, d_z.data_ptr(), d_z.numel(), hip_stream=hip_stream)
            return n_z, d_z

        # ---- the two forms agree on the timed block before any ratio is quoted (the filter handle is fresh: stream position 0 on both sides)
        n_out, d_out = loose()
        st.synchronize()
        want = d_out.cpu().numpy()[:n_out].copy()
        ring = SampleStream(max(n_out, 2048), 1024, device=0)
        kw = dict(input_kind="ibyte", taps=taps, decimation=D, center_freq_hz=fc, sampling_freq_hz=fs, device=0)
        if rs is not None:
            kw.update(fs_in=rs[0], fs_out=rs[1])
        cond = SignalConditioner(ring, **kw)
        first, n_c = cond.push_device(d_raw.data_ptr(), N)
        same = n_c == n_out and np.array_equal(ring.read(first, n_c).view(np.uint32), want.view(np.uint32))
        cond.close()
        ring.close()
        if not same:
            say("%s: the fused push and the loose chain DIFFER: not timed" % name)
            fir.close()
            continue
        cond = SignalConditioner(None, **kw)   # position 0 again: the timed push is the one compared above
        # algorithmic HBM bytes: fused 2 in + 8 out per kept sample (the inputs between kept samples are read too: 2 N in all);
        # loose convert 2 + 8, FIR 8 + 8 / D, gather 8 + 8 per output
        fused_bytes = 2 * N + 8 * n_out
        loose_bytes = 10 * N + 8 * N + 8 * n_f + (16 * n_out if rs is not None else 0)
        cond.time_push(d_raw.data_ptr(), N, 3)
        for _ in range(3):
            loose()
        st.synchronize()
        pairs = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.reps):
                loose()
            e1.record(st)
            e1.synchronize()
            t_l = e0.elapsed_time(e1) / a.reps * 1e3
            t_f = cond.time_push(d_raw.data_ptr(), N, a.reps) * 1e3
            pairs.append((t_f, t_l))
        for k, (t_f, t_l) in enumerate(pairs):
            say("%-40s %10.1f %10.1f %8.2f %12d %14.0f %14.0f" % ("%s #%d" % (name, k + 1), t_f, t_l, t_l / t_f, n_out, fused_bytes / (t_f * 1e-6) / 1e9,
                                                                  loose_bytes / (t_l * 1e-6) / 1e9))
        faster = all(t_f < t_l for t_f, t_l in pairs)
        say("%s: outputs equal bit for bit; MACs per block fused %.3g, loose %.3g; fused %s in all three pairs" % (
            name, float(K) * n_out, float(K) * n_f, "FASTER" if faster else "NOT faster"))
        cond.close()
        fir.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
